"""Prioritized replay: the device sum tree follows the ring (k_per_sync, dqnhip_clear_memory, LoadReplayMemory, the env front-end).
cap = 5000 gives three levels above the leaves: 79 level-1 nodes, 2 level-2 nodes, the root.  After every step the invariants of
tests/per_ref.py hold: every level read back equals the reference's recomputation from the leaves read back, bit for bit; leaves
outside the window are 0; new leaves equal p_max; total > 0 iff size > 0.

No reference counterpart: the reference samples its deque uniformly (SampleTransitionsFromMemory, src/dqn.cpp:501-509)."""
import numpy as np
import pytest

import per_ref as R
from synth import synth_replay

pytestmark = pytest.mark.gpu

CAP, B, S, HID = 5000, 32, 58, (64, 64)


def _make(pkg, **kw):
    d = pkg.DQN(S, minibatch=B, hidden=HID, memory=CAP, seed=3, **kw)
    d.enable_prioritized_replay(seed=11)
    return d


def _levels(d):
    st = d.per_state()
    assert st["levels"] == 3
    lv = [d.per_debug_read("level%d" % k) for k in range(4)]
    assert [len(l) for l in lv] == [CAP, 79, 2, 1]
    return lv, st


class Mirror:
    """host mirror of the deque arithmetic (AddTransitions: while size + n >= cap pop_front, src/dqn.cpp:768-781)"""

    def __init__(self):
        self.head, self.size = 0, 0

    def add(self, n):
        pops = max(0, min(self.size + n - CAP + 1, self.size))
        self.head = (self.head + pops) % CAP
        self.size += n - pops


def _check(d, head, size, fresh=None):
    lv, st = _levels(d)
    R.check_tree(lv)
    R.check_window(lv[0], head, size, lv[-1][0])
    assert st["size"] == size and st["total"] == lv[-1][0]
    if fresh:
        R.check_fresh(lv[0], head, size - fresh, fresh, st["p_max"])
    return lv, st


def test_tree_follows_appends_evictions_clear_and_reload(pkg, gpu, tmp_path):
    rng = np.random.default_rng(1)
    d = _make(pkg)
    m = Mirror()
    lv, st = _check(d, 0, 0)
    assert st["p_max"] == 1.0 and st["enabled"] == 1
    # 5 x 1500 with updates in between: eviction and wrap-around
    for k in range(5):
        d.add_transitions_arrays(*synth_replay(rng, 1500, S, mean_len=10))
        m.add(1500)
        _check(d, m.head, m.size, fresh=1500)
        d.UpdateActorCritic()
        d.UpdateActorCritic(rng.integers(0, m.size, B))
        lv, st = _check(d, m.head, m.size)
        assert st["p_max"] >= max(1.0, lv[0].max())              # the running maximum (its transition may be gone)
    assert m.head != 0 and (m.head + m.size) % CAP < m.head          # the window wraps
    syncs = d.per_state()["syncs"]
    # 3 x 2000 with no update in between: more than cap between two syncs, the host's bound enqueues syncs of its own
    for k in range(3):
        d.add_transitions_arrays(*synth_replay(rng, 2000, S, mean_len=10))
        m.add(2000)
    lv, st = _check(d, m.head, m.size, fresh=2000)
    assert st["syncs"] >= syncs + 2
    # clear: the tree is zero, p_max stays
    p_max = st["p_max"]
    path = str(tmp_path / "m.replaymemory")
    d.SnapshotReplayMemory(path)
    d.ClearReplayMemory()
    lv, st = _check(d, 0, 0)
    assert st["p_max"] == p_max and not lv[0].any()
    # reload: files carry no priorities, every loaded transition gets p_max
    d.LoadReplayMemory(path)
    lv, st = _check(d, 0, m.size, fresh=m.size)
    d.UpdateActorCritic()
    _check(d, 0, m.size)
    d.close()


def test_enable_on_a_filled_memory_gives_every_transition_p_max(pkg, gpu):
    rng = np.random.default_rng(2)
    d = pkg.DQN(S, minibatch=B, hidden=HID, memory=CAP, seed=3)
    m = Mirror()
    for n in (3000, 3000):
        d.add_transitions_arrays(*synth_replay(rng, n, S, mean_len=10))
        m.add(n)
    d.enable_prioritized_replay()
    _check(d, m.head, m.size, fresh=m.size)
    with pytest.raises(pkg.DQNFatal, match="already enabled"):
        d.enable_prioritized_replay()
    d.close()


def test_tree_follows_the_env_front_end(pkg, gpu):
    """8 workers, max_steps 20: appends (and evictions) are decided on the device, the host only knows a bound"""
    d = _make(pkg)
    env = pkg.EnvFrontEnd(d, 8, max_steps=20, seed=5)
    total_steps = 0
    for it in range(12):
        env.step(0.3, n_steps=60)
        total_steps += 8 * 60
        size = d.memory_size()
        if size < 1:
            continue
        d.UpdateActorCritic()
        lv, st = _levels(d)
        R.check_tree(lv)
        assert st["size"] == size
        # the window: `size` consecutive slots (mod cap) hold all the non-zero leaves
        nz = np.nonzero(lv[0])[0]
        assert len(nz) == size, (len(nz), size)
        assert (np.diff(nz) > 1).sum() <= 1 and (nz[-1] - nz[0] == size - 1 or (nz[0] == 0 and nz[-1] == CAP - 1))
        assert lv[-1][0] > 0
    assert total_steps > CAP and size > CAP // 2                # more went in than fits: evictions happened
    env.close(); d.close()
