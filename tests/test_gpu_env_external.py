"""The external kind of env handle (include/dqnhip_env.h: dqnhip_env_create_external / _act / _observe / _read_episodes): the batched
step on caller-supplied states.

1. an arbitrary state stream (tests/env_ref.walk_stream, not the synthetic generator) against HostExternalEnv on the CPU oracle;
2. fed a synthetic handle's own stream, an external handle is that handle's twin (fp32 and fp16 acting);
3. record=False (PlayOneEpisode(update = false)) never touches the replay memory, and its records are the per-step rewards' sums;
4. the protocol: refusals, SERVER_DOWN, the max_steps rule, read_episodes' cap, the _device variants;
5. an observe between two dqnhip_update_chained calls ends the chain.
Bounds are those of tests/test_gpu_env.py: action indices exact, action parameters 1e-4, rewards 2e-5, on-policy targets 2e-4."""
import ctypes as C

import numpy as np
import pytest

import env_ref
from helpers import make_pair
from synth import synth_replay

pytestmark = pytest.mark.gpu

S, HID, T, UNUM = 59, (128, 64, 64, 64), 12, 7


def pair(pkg, capacity=20000, **kw):
    return make_pair(pkg, B=32, S=S, hidden=HID, n_replay=100, capacity=capacity, wscale=10.0, **kw)


def assert_replay(a, b):
    """two read_memory results: states, next states and terminal flags are copies of the input"""
    eq = np.testing.assert_array_equal
    eq(a[0], b[0]); eq(a[4], b[4]); eq(a[5], b[5])
    np.testing.assert_allclose(a[1], b[1], atol=1e-4)          # actor outputs
    np.testing.assert_allclose(a[2], b[2], atol=2e-5)          # rewards
    np.testing.assert_allclose(a[3], b[3], atol=2e-4)          # Monte-Carlo labels


def whole_memory(d):
    return d.read_memory(0, d.memory_size())


@pytest.mark.parametrize("workers,steps", [(5, 40), (64, 40), (600, 15)])     # 600: the unfused heads and the separate commit
def test_arbitrary_stream_matches_host_env(pkg, gpu, workers, steps):
    dqn, orc, data, rng = pair(pkg)
    first, stream = env_ref.walk_stream(1, workers, S, steps, unum=UNUM)
    env = pkg.ExternalEnv(dqn, workers, first, max_steps=T, unum=UNUM, seed=11)
    ref = env_ref.HostExternalEnv(orc, workers, first, max_steps=T, unum=UNUM, seed=11)
    np.testing.assert_array_equal(env.debug_read("state"), first)
    records = []
    for step, (nx, status, pob) in enumerate(stream):
        act, args, ao = env.act(0.0, actor_out=True)
        ract, rargs = ref.act(0.0)
        np.testing.assert_array_equal(act, ract, err_msg="step %d" % step)                 # indices exact
        np.testing.assert_allclose(args, rargs, atol=1e-4)
        np.testing.assert_allclose(ao, ref.actor_out, atol=1e-4)
        np.testing.assert_array_equal(env.debug_read("action").astype(np.int32), ract)
        env.observe(nx, status, pob); ref.observe(nx, status, pob)
        np.testing.assert_allclose(env.debug_read("reward"), ref.reward, atol=2e-5, err_msg="step %d" % step)
        np.testing.assert_array_equal(env.debug_read("episode_len").astype(np.int32), ref.episode_len())
        np.testing.assert_array_equal(env.debug_read("state"), nx)
        if step % 4 == 3:
            records += env.episodes()              # (a worker's ring holds 8 records: at most 4 can end in 4 steps)
    records += env.episodes()
    # the stream holds every kind of event the reward and the episode logic distinguish
    assert ref.truncated > 0 and ref.goals_own > 0 and ref.goals_other > 0 and ref.kickable_rewards > 0
    assert env.dropped == 0 and env.debug_read("truncated") == ref.truncated
    s1, s2 = env.stats(), ref.stats()
    assert s1[0] == s2[0] == steps * workers and s1[1] == s2[1] > 0 and s1[3] == s2[3]
    assert abs(s1[2] - s2[2]) < 2e-5 * steps * workers
    assert dqn.memory_size() == orc.memory_size() > 100
    assert_replay(whole_memory(dqn), orc.read_memory(0, orc.memory_size()))
    assert [(r.worker, r.steps, r.status, r.step_index) for r in records] == [(r.worker, r.steps, r.status, r.step_index) for r in ref.records]
    for got, want in zip(records, ref.records):
        assert abs(got.total_reward - want.total_reward) <= 2e-5 * want.steps
        assert got.extrinsic_reward == want.extrinsic_reward
    loss, q = dqn.UpdateActorCritic()                         # the learner keeps working on what the workers produced
    assert np.isfinite(loss) and np.isfinite(q)
    env.close(); dqn.close(); orc.close()


def run_twins(pkg, eps, steps, make):
    """A: a synthetic handle stepped one step at a time; B: an external handle fed A's states and the Philox twin's draws"""
    kw = dict(max_steps=T, unum=UNUM, p_end=0.08, p_goal=0.4, seed=11)
    workers = 64
    da, db = make(), make()
    a = pkg.EnvFrontEnd(da, workers, **kw)
    b = pkg.ExternalEnv(db, workers, a.debug_read("state"), max_steps=T, unum=UNUM, seed=11)
    g = np.ones(workers, np.uint64)
    for step in range(steps):
        status, pob = env_ref.synthetic_status_pob(11, g, kw["p_end"], kw["p_goal"], UNUM)
        len_before = a.debug_read("episode_len")
        a.step(eps)
        act, args = b.act(eps)
        b.observe(a.debug_read("state"), status, pob)
        np.testing.assert_array_equal(act, a.debug_read("action").astype(np.int32), err_msg="step %d" % step)
        np.testing.assert_allclose(args[:, 0], a.debug_read("arg1"), atol=1e-4)
        np.testing.assert_allclose(b.debug_read("reward"), a.debug_read("reward"), atol=2e-5)
        np.testing.assert_array_equal(b.debug_read("episode_len"), a.debug_read("episode_len"))
        ended = (status != 0) | (len_before + 1 >= T)
        g += np.where(ended, 2, 1).astype(np.uint64)
    sa, sb = a.stats(), b.stats()
    assert sa[0] == sb[0] == steps * workers and sa[1] == sb[1] > 0 and sa[3] == sb[3] > 0
    assert da.memory_size() == db.memory_size() > 100
    assert_replay(whole_memory(da), whole_memory(db))
    a.close(); b.close(); da.close(); db.close()


@pytest.mark.parametrize("eps", [0.3, 1.0])
def test_twin_of_the_synthetic_handle(pkg, gpu, eps):
    def make():
        dqn, orc, _, _ = pair(pkg)
        orc.close()
        return dqn
    run_twins(pkg, eps, 60, make)


def test_twin_of_the_synthetic_handle_fp16_acting(pkg, gpu):
    def make():
        dqn, orc, _, _ = make_pair(pkg, B=128, S=S, hidden=(128, 128), n_replay=100, capacity=20000, wscale=5.0, precision="fp16")
        orc.close()
        dqn.set_act_precision("fp16")
        return dqn
    run_twins(pkg, 0.3, 60, make)


def test_no_record_leaves_the_replay_alone(pkg, gpu):
    workers, steps = 16, 30
    first, stream = env_ref.walk_stream(2, workers, S, steps, unum=UNUM)
    dqn, orc, _, _ = pair(pkg, capacity=150)                  # (no workers*max_steps < capacity condition for an evaluation handle)
    before = whole_memory(dqn)
    ev = pkg.ExternalEnv(dqn, workers, first, max_steps=T, unum=UNUM, seed=5, record=False)
    sums, want, records = np.zeros(workers, np.float64), [], []
    for step, (nx, status, pob) in enumerate(stream):
        ev.act(0.1); ev.observe(nx, status, pob)
        sums += ev.debug_read("reward").astype(np.float64)
        ended = (status != 0) | (ev.debug_read("episode_len") == 0)
        for w in np.flatnonzero(ended):
            want.append((step + 1, int(w), float(sums[w]))); sums[w] = 0.0
        if step % 4 == 3:
            got = ev.episodes() if step > 3 else ev.episodes(cap=1) + ev.episodes()
            assert [(r.step_index, r.worker, r.total_reward) for r in got] == want      # the records are the double sums, exactly
            want = []; records += got
    assert ev.stats()[1] == len(records) + len(want) > workers and ev.dropped == 0
    assert dqn.memory_size() == 100
    for x, y in zip(before, whole_memory(dqn)):
        np.testing.assert_array_equal(x, y)
    summary = pkg.evaluation_summary(records)
    assert summary["goals"] == sum(r.status == 1 for r in records) > 0 and summary["goal_perc"] == float(np.float32(summary["goals"]) / np.float32(len(records)))
    ev.close(); dqn.close(); orc.close()


def test_evaluation_handle_beside_a_recording_one(pkg, gpu):
    workers, steps = 16, 30
    first, stream = env_ref.walk_stream(3, workers, S, steps, unum=UNUM)
    first_ev, stream_ev = env_ref.walk_stream(4, workers, S, steps, unum=UNUM)
    mem = []
    for with_eval in (False, True):
        dqn, orc, _, _ = pair(pkg)
        orc.close()
        rec = pkg.ExternalEnv(dqn, workers, first, max_steps=T, unum=UNUM, seed=5)
        ev = pkg.ExternalEnv(dqn, workers, first_ev, max_steps=T, unum=UNUM, seed=6, record=False) if with_eval else None
        for (nx, status, pob), (nx2, status2, pob2) in zip(stream, stream_ev):
            rec.act(0.2)
            if ev:
                ev.act(0.0)
            rec.observe(nx, status, pob)
            if ev:
                ev.observe(nx2, status2, pob2)
        assert rec.stats()[1] > 0 and (ev is None or ev.stats()[1] > 0)
        mem.append(whole_memory(dqn))
        rec.close(); dqn.close()
        if ev:
            ev.close()
    assert len(mem[0][2]) > 100
    for x, y in zip(*mem):
        np.testing.assert_array_equal(x, y)


def test_protocol(pkg, gpu):
    dqn, orc, _, _ = pair(pkg)
    orc.close()
    first, stream = env_ref.walk_stream(5, 4, S, 8, unum=UNUM)
    nx = stream[0][0]
    zero, pob = np.zeros(4, np.int32), np.full(4, -1, np.int32)
    synthetic = pkg.EnvFrontEnd(dqn, 4, max_steps=T)
    with pytest.raises(pkg.DQNFatal, match="dqnhip_env_step"):
        pkg.ExternalEnv.act(synthetic, 0.0)
    with pytest.raises(pkg.DQNFatal, match="dqnhip_env_step"):
        pkg.ExternalEnv.observe(synthetic, nx, zero, pob)
    synthetic.close()
    env = pkg.ExternalEnv(dqn, 4, first, max_steps=T, unum=UNUM)
    with pytest.raises(pkg.DQNFatal, match="dqnhip_env_act"):
        env.step(0.0)
    with pytest.raises(pkg.DQNFatal, match="no dqnhip_env_act"):
        env.observe(nx, zero, pob)
    env.act(0.0)
    with pytest.raises(pkg.DQNFatal, match="has not been answered"):
        env.act(0.0)
    other = pkg.ExternalEnv(dqn, 4, first, max_steps=T)
    with pytest.raises(pkg.DQNFatal, match="epsilon"):
        other.act(1.5)
    other.close()
    env.observe(nx, zero, pob)
    assert env.stats()[0] == 4
    env.act(0.0); env.observe(nx, np.array([0, 5, 0, 0], np.int32), pob)
    with pytest.raises(pkg.DQNFatal, match="Server Down!"):
        env.stats()
    with pytest.raises(pkg.DQNFatal, match="Server Down!"):      # sticky
        env.episodes()
    env.close()
    env = pkg.ExternalEnv(dqn, 4, first, max_steps=T, unum=UNUM)
    env.act(0.0); env.observe(nx, np.array([0, 0, -2, 0], np.int32), pob)
    with pytest.raises(pkg.DQNFatal, match="status out of range"):
        env.stats()
    env.close()
    small = pkg.DQN(S, minibatch=32, hidden=(64,), memory=40)
    with pytest.raises(pkg.DQNFatal, match="capacity"):
        pkg.ExternalEnv(small, 4, first, max_steps=T, unum=UNUM)             # a recording handle keeps workers*max_steps < capacity
    pkg.ExternalEnv(small, 4, first, max_steps=T, unum=UNUM, record=False).close()
    dqn.close(); small.close()


def test_max_steps_closes_the_episode_as_out_of_time(pkg, gpu):
    dqn, orc, _, _ = pair(pkg)
    orc.close()
    first, stream = env_ref.walk_stream(6, 1, S, 7, unum=UNUM, p_end=0.0)
    env = pkg.ExternalEnv(dqn, 1, first, max_steps=5, unum=UNUM)
    for nx, status, pob in stream:                            # seven IN_GAME steps
        assert status[0] == 0
        env.act(0.0); env.observe(nx, status, pob)
    assert env.stats()[:2] == (7, 1) and env.debug_read("truncated") == 1
    assert dqn.memory_size() == 105
    m = dqn.read_memory(100, 5)
    np.testing.assert_array_equal(m[5], [0, 0, 0, 0, 1])
    np.testing.assert_array_equal(m[0], np.concatenate([first, *[s[0] for s in stream[:4]]]))
    np.testing.assert_array_equal(m[4][:4], m[0][1:])
    (ep,) = env.episodes()
    assert (ep.steps, ep.status, ep.worker, ep.step_index) == (6, 4, 0, 5)
    assert env.debug_read("episode_len")[0] == 2
    env.close(); dqn.close()


def test_read_episodes_hands_out_the_rest_on_the_next_call(pkg, gpu):
    dqn, orc, _, _ = pair(pkg)
    orc.close()
    first, stream = env_ref.walk_stream(7, 8, S, 3, unum=UNUM)
    env = pkg.ExternalEnv(dqn, 8, first, max_steps=T, unum=UNUM, record=False)
    for k, (nx, status, pob) in enumerate(stream):
        env.act(0.0); env.observe(nx, np.full(8, 1 + k, np.int32), pob)      # every worker's episode ends at every step
    a = env.episodes(cap=5); b = env.episodes(cap=100); c = env.episodes()
    assert len(a) == 5 and len(b) == 19 and c == [] and env.dropped == 0
    assert [(r.step_index, r.worker, r.status) for r in a + b] == [(k + 1, w, k + 1) for k in range(3) for w in range(8)]
    for k in range(10):                                       # ten more per worker: the rings keep the last eight
        env.act(0.0); env.observe(stream[0][0], np.full(8, 2, np.int32), stream[0][2])
    d = env.episodes()
    assert len(d) == 64 and env.dropped == 16 and d[0].step_index == 6
    env.close(); dqn.close()


def test_device_variants_equal_host_variants(pkg, gpu):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    workers, steps = 16, 20
    first, stream = env_ref.walk_stream(8, workers, S, steps, unum=UNUM)

    def dev(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), nbytes) == 0
        return p
    bufs = dict(action=dev(workers * 4), args=dev(workers * 8), ao=dev(workers * 40), nx=dev(workers * S * 4), status=dev(workers * 4), pob=dev(workers * 4))
    out = []
    for device in (False, True):
        dqn, orc, _, _ = pair(pkg)
        orc.close()
        env = pkg.ExternalEnv(dqn, workers, first, max_steps=T, unum=UNUM, seed=9)
        acts = []
        for nx, status, pob in stream:
            if device:
                env.act_device(0.2, bufs["action"], bufs["args"], bufs["ao"])
                for name, arr in (("nx", nx), ("status", status), ("pob", pob)):
                    assert hip.hipMemcpy(bufs[name], arr.ctypes.data_as(C.c_void_p), arr.nbytes, 1) == 0
                env.observe_device(bufs["nx"], bufs["status"], bufs["pob"])
                assert hip.hipDeviceSynchronize() == 0
                act, args, ao = np.empty(workers, np.int32), np.empty((workers, 2), np.float32), np.empty((workers, 10), np.float32)
                for name, arr in (("action", act), ("args", args), ("ao", ao)):
                    assert hip.hipMemcpy(arr.ctypes.data_as(C.c_void_p), bufs[name], arr.nbytes, 2) == 0
            else:
                act, args, ao = env.act(0.2, actor_out=True)
                env.observe(nx, status, pob)
            acts.append((act, args, ao))
        out.append((acts, whole_memory(dqn), env.stats(), env.episodes()))
        env.close(); dqn.close()
    for p in bufs.values():
        hip.hipFree(p)
    assert out[0][2] == out[1][2] and out[0][3] == out[1][3] and out[0][2][1] > 0
    for x, y in zip(out[0][0], out[1][0]):
        for u, v in zip(x, y):
            np.testing.assert_array_equal(u, v)
    for x, y in zip(out[0][1], out[1][1]):
        np.testing.assert_array_equal(x, y)


def test_observe_ends_an_update_chain(pkg, gpu):
    B, hidden, Sc = 64, (256, 128, 64, 64), 58
    idx = np.random.default_rng(5).integers(0, 3000, size=(12, B)).astype(np.int32)
    first, stream = env_ref.walk_stream(9, 8, Sc, 12, unum=UNUM)
    state = []
    for chained in (False, True):
        d = pkg.DQN(Sc, minibatch=B, hidden=hidden, memory=4096, seed=11, use_graph=True)
        d.add_transitions_arrays(*synth_replay(np.random.default_rng(2), 3000, Sc))
        env = pkg.ExternalEnv(d, 8, first, max_steps=T, unum=UNUM, seed=3)
        res = []
        for t in range(12):
            nxt = idx[t + 1] if t + 1 < 12 else None
            res.append(d.UpdateActorCriticChained(idx[t], nxt) if chained else d.UpdateActorCritic(idx[t]))
            if t % 3 != 2:                                    # (every third pair of updates stays chained)
                env.act(0.1); env.observe(*stream[t])
        assert env.stats()[1] > 0 and d.memory_size() > 3000
        state.append((res, [d.get_params(n) for n in range(4)], whole_memory(d)))
        env.close(); d.close()
    assert state[0][0] == state[1][0]
    for x, y in zip(state[0][1] + list(state[0][2]), state[1][1] + list(state[1][2])):
        np.testing.assert_array_equal(x, y)
