"""The batched env front-end with an fp16 learner acting in fp16 (dqnhip_set_act_precision) beside a twin acting in fp32.

Two fp16 learners with identical weights and replay, envs of the same seed, epsilon = 0.  The synthetic state stream, the status and
the reward do not depend on the action (env.hip.h: env_feature, game_update), so everything but the actor outputs is bit-identical
between the twins, and the fp16 twin's actor outputs are the emulation's (tower16 + heads32 of tests/test_gpu_fp16.py) under close16.
5 and 64 workers: the heads ride in the step kernel; 600: a separate head launch, rows not a multiple of 64."""
import numpy as np
import pytest

from helpers import make_pair
from test_gpu_fp16 import close16, heads32, tower16, unpack

pytestmark = pytest.mark.gpu

B, S, HID = 128, 59, (256, 128)
ENV = dict(max_steps=8, unum=7, p_end=0.2, p_goal=0.4, seed=11)
WORKERS = [5, 64, 600]


def twins(pkg, workers, second="fp32"):
    """(fp16-acting learner, its env, the twin acting in `second`, its env, emulation of the greedy actor)"""
    out = []
    for prec in ("fp16", second):
        dqn, orc, data, rng = make_pair(pkg, B=B, S=S, hidden=HID, n_replay=100, capacity=40000, wscale=5.0, precision="fp16", use_graph=True)
        orc.close()
        dqn.set_act_precision(prec)
        out += [dqn, pkg.EnvFrontEnd(dqn, workers, **ENV)]
    p = unpack(out[0].get_params(0), S, HID, (4, 6))
    np.testing.assert_array_equal(out[0].get_params(0), out[2].get_params(0))
    return out + [lambda x: heads32(tower16(x, p, len(HID))[1], p, len(HID))]


def get_action(ao):
    """GetAction (src/dqn.cpp:196-208) of one ActorOutput: (action, arg1, arg2); TACKLE (index 2) is never chosen"""
    c = np.array([ao[0], ao[1], -99999.0, ao[3]], np.float32)
    best = int(np.argmax(c))                       # first maximum, as the strict > chain
    o1 = {0: 0, 1: 2, 2: 3, 3: 4}[best]
    o2 = {0: 1, 3: 5}.get(best, -1)
    return best, ao[4 + o1], np.float32(0) if o2 < 0 else ao[4 + o2]


def close_all(*things):
    for t in things:
        t.close()


@pytest.mark.parametrize("workers", WORKERS)
def test_step_by_step(pkg, gpu, workers):
    d16, e16, d32, e32, emu = twins(pkg, workers)
    for step in range(12):
        state = e16.debug_read("state")
        np.testing.assert_array_equal(state, e32.debug_read("state"))
        e16.step(0.0); e32.step(0.0)
        for name in ("state", "reward", "episode_len"):
            np.testing.assert_array_equal(e16.debug_read(name), e32.debug_read(name), err_msg="%s at step %d" % (name, step))
        ao = e16.debug_read("actor_out")
        close16(ao, emu(state), "actor_out at step %d" % step)
        act, a1, a2 = e16.debug_read("action"), e16.debug_read("arg1"), e16.debug_read("arg2")
        want = [get_action(row) for row in ao]
        np.testing.assert_array_equal(act.astype(np.int32), [w[0] for w in want])
        np.testing.assert_array_equal(a1, np.array([w[1] for w in want], np.float32))
        np.testing.assert_array_equal(a2, np.array([w[2] for w in want], np.float32))
    close_all(e16, e32, d16, d32)


@pytest.mark.parametrize("workers", WORKERS)
def test_one_call_of_33_steps(pkg, gpu, workers):
    """two 16-step graphs and one single-step remainder"""
    d16, e16, d32, e32, emu = twins(pkg, workers)
    e16.step(0.0, 33); e32.step(0.0, 33)
    s16, s32 = e16.stats(), e32.stats()
    assert s16 == s32 and s16[0] == 33 * workers and s16[1] > 0
    n = d16.memory_size()
    assert n == d32.memory_size() and n > 100
    a, b = d16.read_memory(0, n), d32.read_memory(0, n)
    for k in (0, 2, 3, 4, 5):                      # states, rewards, on-policy targets, next states, terminal flags
        np.testing.assert_array_equal(a[k], b[k])
    close16(a[1][100:], emu(a[0][100:]), "stored actor outputs")       # (the first 100 transitions are make_pair's synthetic replay)
    close_all(e16, e32, d16, d32)


@pytest.mark.parametrize("workers", WORKERS)
def test_switch_mid_life(pkg, gpu, workers):
    """16 steps in fp32 capture the fp32 step graph; the switch drops it and the next 17 steps act in fp16"""
    d16, e16, dsw, esw, emu = twins(pkg, workers, second="fp32")
    e16.step(0.0, 16); esw.step(0.0, 16)
    n16 = d16.memory_size()                        # transitions of the episodes that ended within the first 16 steps
    assert n16 == dsw.memory_size()
    dsw.set_act_precision("fp16")
    assert dsw.act_precision == "fp16"
    state = esw.debug_read("state")
    np.testing.assert_array_equal(state, e16.debug_read("state"))
    esw.step(0.0, 1); e16.step(0.0, 1)
    close16(esw.debug_read("actor_out"), emu(state), "first step after the switch")
    np.testing.assert_array_equal(esw.debug_read("actor_out"), e16.debug_read("actor_out"))
    esw.step(0.0, 16); e16.step(0.0, 16)
    np.testing.assert_array_equal(esw.debug_read("actor_out"), e16.debug_read("actor_out"))
    assert esw.stats() == e16.stats()
    n = d16.memory_size()
    assert n == dsw.memory_size() and n > n16
    a, b = d16.read_memory(0, n), dsw.read_memory(0, n)
    for k in (0, 2, 3, 4, 5):
        np.testing.assert_array_equal(a[k], b[k])
    # actor outputs: identical but for those chosen during the first 16 steps (in the ring: everything flushed by then, plus the
    # head of each episode that was open at the switch — at most max_steps - 1 transitions per worker)
    diff = np.flatnonzero(np.any(a[1] != b[1], axis=1))
    assert diff.size > 0 and diff.max() < n16 + workers * (ENV["max_steps"] - 1)
    late = np.arange(n16 + workers * (ENV["max_steps"] - 1), n)
    if late.size:
        close16(b[1][late], emu(b[0][late]), "stored actor outputs after the switch")
    close_all(e16, esw, d16, dsw)
