"""N-step returns on memories the other paths fill: the contiguity invariant (a non-terminal transition's stored next state is its
logical successor's state) checked on the device after the env front-end's flushes and after a `.replaymemory` round trip, the
windows an n-step update takes there against tests/nstep_ref.py, and a learner that reads another learner's replay memory."""
import numpy as np
import pytest

import nstep_ref as R
from synth import det_indices, synth_replay

pytestmark = pytest.mark.gpu

B, S, HID = 32, 58, (64, 64)
GAMMA = 0.99


def _check_windows(d, idx, n):
    size = d.memory_size()
    s, a, r, mc, nx, term = d.read_memory(0, size)
    d.UpdateActorCritic(idx)
    want = R.gather(r, term, idx, n, GAMMA)
    assert np.array_equal(d.n_step_debug_read("steps"), want["steps"])
    assert np.array_equal(d.n_step_debug_read("reward").view(np.uint32), want["reward"].view(np.uint32))
    assert np.array_equal(d.n_step_debug_read("disc").view(np.uint64), want["disc"].view(np.uint64))
    assert np.array_equal(d.debug_read("terminal"), want["terminal"])
    return want


def test_env_front_end_appends_whole_episodes(pkg, gpu):
    """64 workers, episodes of at most 12 steps, a ring small enough to evict: every flush appends whole episodes, so the invariant
    holds wherever the ring's head has moved to, and an n-step learner trains on it"""
    d = pkg.DQN(S, minibatch=B, hidden=HID, memory=1500, seed=3)
    d.enable_n_step(4)
    env = pkg.EnvFrontEnd(d, 64, max_steps=12, unum=7, p_end=0.1, p_goal=0.4, seed=11)
    seen_full = False
    for burst in range(4):
        env.step(0.3, 12)
        size = d.memory_size()
        assert size > B
        assert d.validate_memory() == (0, -1), burst
        seen_full |= size >= 1400
        want = _check_windows(d, det_indices(31 + burst, 1, B, size)[0], 4)
        assert want["steps"].max() > 1
    assert seen_full, "the ring never filled: nothing was evicted"
    assert all(np.isfinite(d.read_stats()))
    env.close(); d.close()


def test_replaymemory_file_round_trip_keeps_the_invariant(pkg, gpu, tmp_path):
    rp = synth_replay(np.random.default_rng(5), 700, S, mean_len=10)
    a = pkg.DQN(S, minibatch=B, hidden=HID, memory=512, seed=3)
    a.add_transitions_arrays(*[x[:350] for x in rp])
    a.add_transitions_arrays(*[x[350:] for x in rp])          # evicts: the window starts inside an episode
    f = str(tmp_path / "mem.replaymemory")
    a.SnapshotReplayMemory(f)
    b = pkg.DQN(S, minibatch=B, hidden=HID, memory=512, seed=3)
    b.LoadReplayMemory(f)
    assert b.memory_size() == a.memory_size() and a.validate_memory() == (0, -1) and b.validate_memory() == (0, -1)
    a.enable_n_step(3); b.enable_n_step(3)
    idx = det_indices(37, 1, B, a.memory_size())[0]
    wa, wb = _check_windows(a, idx, 3), _check_windows(b, idx, 3)
    assert np.array_equal(wa["steps"], wb["steps"]) and np.array_equal(wa["reward"], wb["reward"])
    a.close(); b.close()


def test_a_sharer_walks_the_owners_ring(pkg, gpu):
    rp = synth_replay(np.random.default_rng(5), 1024, S, mean_len=10)
    owner = pkg.DQN(S, minibatch=B, hidden=HID, memory=2048, seed=3)
    owner.add_transitions_arrays(*rp)
    sharer = pkg.DQN(S, minibatch=B, hidden=HID, memory=2048, seed=3)
    alone = pkg.DQN(S, minibatch=B, hidden=HID, memory=2048, seed=3)
    alone.add_transitions_arrays(*rp)
    owner.ShareReplayMemory(sharer)
    sharer.enable_n_step(3); alone.enable_n_step(3)
    assert owner.n_step() == 0 and sharer.validate_memory() == (0, -1)
    idx = det_indices(41, 2, B, 1024)
    for u in range(2):
        want, got = alone.UpdateActorCritic(idx[u]), sharer.UpdateActorCritic(idx[u])
        assert np.array_equal(np.asarray(got, np.float32).view(np.uint32), np.asarray(want, np.float32).view(np.uint32))
        assert np.array_equal(sharer.n_step_debug_read("steps"), R.gather(rp[2], rp[5], idx[u], 3, GAMMA)["steps"])
        for net in range(4):
            assert np.array_equal(sharer.get_params(net).view(np.uint32), alone.get_params(net).view(np.uint32))
    owner.UpdateActorCritic(idx[0])                           # the owner stays a 1-step learner on the same ring
    assert all(np.isfinite(owner.read_stats()))
    sharer.close(); alone.close(); owner.close()
