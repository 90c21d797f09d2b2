"""dqnhip_update_indexed_n / dqnhip_collect_stats: n updates on the CALLER's indices, enqueued as graphs of 16 / 8 / 4 / 2 / 1 updates
without waiting, every update's (critic_loss, avg_q) handed back afterwards — the reference's bursts of `dqn->Update()`
(src/dqn_main.cpp:340-343, 359-361) whose results the driver discards (src/dqn.cpp:799-826 only logs and snapshots).  Whatever the
grouping, state and pairs must be exactly what n blocking dqnhip_update calls on the same indices leave and return."""
import numpy as np
import pytest

from synth import synth_replay

pytestmark = pytest.mark.gpu

SHAPES = {
    "riders": ("fp32", 64, (256, 128, 64, 64), 58),          # riders in both optimiser launches
    "reference": ("fp32", 32, (1024, 512, 256, 128), 59),    # the reference's shape
    "late_gather": ("fp32", 64, (256, 128), 68),             # riders do not fit: late-gather form
    "fp16": ("fp16", 128, (256, 128, 128), 59),
    "baseline": ("fp32", 256, (1024, 1024, 1024, 1024), 58),
}
NS = (1, 2, 15, 16, 17, 35, 48)


def _state(d, pkg):
    out = [d.get_params(n) for n in range(4)]
    out += [d.get_params(n, k) for n in (0, 1) for k in (pkg.KIND_M, pkg.KIND_V)]
    return out, (d.actor_iter(), d.critic_iter())


def _mk(pkg, shape, use_graph=True, replay=None, **kw):
    precision, B, hidden, S = SHAPES[shape]
    d = pkg.DQN(S, minibatch=B, hidden=hidden, memory=4096, seed=11, use_graph=use_graph, precision=precision, **kw)
    d.add_transitions_arrays(*(replay if replay is not None else synth_replay(np.random.default_rng(2), 3000, S)))
    return d


def _idx(shape, n=48, seed=5):
    return np.random.default_rng(seed).integers(0, 3000, size=(n, SHAPES[shape][1])).astype(np.int32)


def _same(sa, sb):
    assert sa[1] == sb[1]
    for x, y in zip(sa[0], sb[0]):
        np.testing.assert_array_equal(x, y)


_REF = {}


def _reference(pkg, shape, use_graph, ns):
    """the blocking twin, once per (shape, use_graph): pairs of all updates and the state after each n of `ns`"""
    key = (shape, use_graph)
    if key not in _REF:
        idx = _idx(shape)
        d = _mk(pkg, shape, use_graph)
        pairs, states = [], {}
        for t in range(max(ns)):
            pairs.append(d.UpdateActorCritic(idx[t]))
            if t + 1 in ns:
                states[t + 1] = _state(d, pkg)
        d.close()
        _REF[key] = (pairs, states)
    return _REF[key]


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("shape", ["riders", "reference", "late_gather", "fp16"])
@pytest.mark.parametrize("n", NS)
def test_indexed_burst_equals_blocking_calls(pkg, gpu, shape, use_graph, n):
    pairs, states = _reference(pkg, shape, use_graph, NS)
    d = _mk(pkg, shape, use_graph)
    d.update_indexed_n(_idx(shape)[:n])
    got = d.collect_stats()
    sd = _state(d, pkg); d.close()
    assert got == pairs[:n]
    assert sd[1] == (n, n)
    _same(sd, states[n])


@pytest.mark.parametrize("use_graph", [True, False])
def test_indexed_burst_baseline_tower(pkg, gpu, use_graph):
    pairs, states = _reference(pkg, "baseline", use_graph, (35,))
    d = _mk(pkg, "baseline", use_graph)
    d.update_indexed_n(_idx("baseline")[:35])
    got = d.collect_stats()
    sd = _state(d, pkg); d.close()
    assert got == pairs[:35] and sd[1] == (35, 35)
    _same(sd, states[35])


def test_split_calls_and_collection_in_pieces(pkg, gpu):
    pairs, states = _reference(pkg, "riders", True, NS)
    idx = _idx("riders")
    d = _mk(pkg, "riders")
    at = 0
    for k in (5, 16, 1, 26):
        d.update_indexed_n(idx[at:at + k]); at += k
    got, pieces = [], 0
    while True:
        part = d.collect_stats(cap=10)
        if not part:
            break
        assert len(part) <= 10
        got += part; pieces += 1
    assert pieces == 5 and got == pairs
    assert d.read_stats() == pairs[-1]
    _same(_state(d, pkg), states[48]); d.close()


def test_interleaving_with_other_entry_points(pkg, gpu):
    """one script on both twins; only the bursts differ (indexed + collected later, against blocking calls)"""
    idx = _idx("riders", 60, seed=8)
    extra = synth_replay(np.random.default_rng(9), 500, 58)
    res = []
    for indexed in (False, True):
        d = _mk(pkg, "riders")
        out, seen = [], []

        def burst(lo, hi):
            if indexed:
                d.update_indexed_n(idx[lo:hi])
            else:
                out.extend(d.UpdateActorCritic(i) for i in idx[lo:hi])

        burst(0, 5)
        d.update_async(None)
        burst(5, 22)
        seen.append(d.read_stats())                      # the burst's last pair; consumes nothing
        d.update_async_n(19)
        d.add_transitions_arrays(*extra)
        burst(22, 38)
        w = d.get_params(0); d.set_params(0, w * 1.01)
        burst(38, 41)
        d.CloneNet(0)
        if indexed:
            out.extend(d.collect_stats())
        c0 = d.UpdateActorCriticChained(idx[41], idx[42])    # after a burst: a fresh chain
        c1 = d.UpdateActorCriticChained(idx[42], None)
        burst(43, 60)
        seen.append(d.read_stats())
        if indexed:
            out.extend(d.collect_stats())
        assert seen[1] == out[-1]
        res.append((out, seen, c0, c1, _state(d, pkg))); d.close()
    assert res[0][0] == res[1][0] and len(res[0][0]) == 58
    assert res[0][1:4] == res[1][1:4]
    assert res[0][4][1] == (80, 80)
    _same(res[0][4], res[1][4])


def test_validation_and_refusals(pkg, gpu):
    d = pkg.DQN(59, minibatch=32, hidden=(64, 64), memory=4096, seed=1, use_graph=True)
    ok = np.tile(np.arange(32, dtype=np.int32), (3, 1))
    with pytest.raises(pkg.DQNFatal, match="replay memory is empty"):
        d.update_indexed_n(ok)
    d.add_transitions_arrays(*synth_replay(np.random.default_rng(2), 3000, 59))
    bad = ok.copy(); bad[1, 3] = 5000
    with pytest.raises(pkg.DQNFatal, match=r"update 1: sampled index 3 = 5000 out of range \[0,3000\)"):
        d.update_indexed_n(bad)
    assert (d.actor_iter(), d.critic_iter()) == (0, 0) and d.collect_stats() == []
    with pytest.raises(pkg.DQNFatal, match="n must be >= 0"):
        d._ck(d.lib.dqnhip_update_indexed_n(d.h, None, -1))
    d.update_indexed_n(ok[:0])                           # n == 0: no-op
    assert d.actor_iter() == 0
    d.update_phase(0, None)
    with pytest.raises(pkg.DQNFatal, match="phased update is in progress"):
        d.update_indexed_n(ok)
    d.update_abort()
    d.update_indexed_n(ok)
    assert len(d.collect_stats()) == 3 and d.actor_iter() == 3
    d.close()
    g = pkg.DQN(59, minibatch=32, hidden=(64, 64), memory=256, seed=1, dp_world=1, dp_rank=0)
    g.add_transitions_arrays(*synth_replay(np.random.default_rng(2), 100, 59))
    g.dp_init(pkg.DQN.dp_unique_id(), half_grads=True)
    with pytest.raises(pkg.DQNFatal, match="dqnhip_dp_update"):
        g.update_indexed_n(ok)
    g.close()


def test_flags_travel_with_their_update(pkg, gpu):
    """NaN arithmetic on valid memory: one transition's reward is NaN and only the third of four index vectors holds it"""
    replay = list(synth_replay(np.random.default_rng(2), 3000, 58))
    replay[2] = replay[2].copy(); replay[2][7] = np.nan
    idx = np.random.default_rng(3).integers(8, 3000, size=(4, 64)).astype(np.int32)
    idx[2, 11] = 7
    d = _mk(pkg, "riders", replay=replay)
    d.update_indexed_n(idx)
    got = []
    with pytest.raises(pkg.DQNFatal, match=r"collected update 2: Target not finite"):
        d.collect_stats(out=got)
    assert len(got) == 4
    assert d.collect_stats() == []
    d.close()
    b = _mk(pkg, "riders", replay=replay)
    ref = [b.UpdateActorCritic(idx[0]), b.UpdateActorCritic(idx[1])]
    with pytest.raises(pkg.DQNFatal, match="Target not finite"):
        b.UpdateActorCritic(idx[2])
    b.close()
    assert got[:2] == ref


def test_sixteen_update_indexed_graph_launch_count(pkg, gpu):
    """an indexed graph has the launch sequence of a sampled one (dqnhip_get_update_plan): counted on the captured graph's kernel nodes"""
    d = _mk(pkg, "riders")
    assert int(d.debug_read("indexed_graph_launches")[0]) == 0
    d.update_indexed_n(_idx("riders")[:16])
    d.collect_stats()
    plan = d.update_plan()
    assert plan["updates_per_graph"] == 16
    assert int(d.debug_read("indexed_graph_launches")[0]) == plan["launches_graph_first"] + 15 * plan["launches_in_graph"]
    d.close()


def test_blocking_benchmark_deferred_form_runs(pkg, gpu):
    d = _mk(pkg, "riders")
    ms = d.BenchmarkBlocking(70, 9, seed=3, pipelined=3)
    assert ms > 0 and d.actor_iter() == 79 and d.collect_stats() == []
    d.close()
