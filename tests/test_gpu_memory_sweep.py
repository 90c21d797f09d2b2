"""The replay sweep on the device (dqnhip_evaluate_memory / dqnhip_per_refresh, DQN.evaluate_memory() / per_refresh()).

Shapes: S = 59, hidden (64, 64), capacity 128 with 150 transitions added in two calls (100, then 50): the ring is wrapped, head = 23,
127 transitions are left (AddTransitions keeps one slot free) and the last logical one is terminal.  B = 32 (a 32-row block is less
than one wave of the row kernel; 3 full chunks and a 31-row tail) and B = 256 (four waves; fewer rows than one chunk).
The four nets hold four different parameter sets, so a target net taken for its online net shows.

Bit identity: at these shapes the default plan forms q, y and q_target in k_head_q_train (the plan moves that arithmetic into the
critic's top-layer dgrad launch only from 512 hidden units up), which is the launch the sweep issues; the update it is compared with
runs on a learner created with DQNHIP_TUNE_SEPARATE_Q_TRAIN, the flag that selects that form at every shape.

Accuracy: q, y, q_policy against oracle/torch_ref.py's float64 forward on the same weights, 1e-4 absolute per element — the project's
Q bound (tests/test_gpu_multiseed_parity.py).  Everything else is exact, or under tests/sweep_ref.py's comparator."""
import ctypes as C
import functools

import numpy as np
import pytest

import per_ref
import sweep_ref as W
from synth import det_params, det_replay

pytestmark = pytest.mark.gpu

F = np.float32
S, HID, CAP, ADDED, SIZE, HEAD = 59, (64, 64), 128, 150, 127, 23
GAMMA, BETA = 0.99, 0.5
Q_BOUND = 1e-4
WINDOWS = [(0, -1), (5, 70), (0, 0)]


def _params(net):
    return det_params(31 + net, S, HID, actor=net in (0, 2), wscale=10.0)


def _replay(nan_reward_at=None):
    rp = [a.copy() for a in det_replay(7, ADDED, S)]
    if nan_reward_at is not None:
        rp[2][ADDED - SIZE + nan_reward_at] = np.nan            # logical index -> position in what was added
    return rp


def _make(pkg, B, per=None, replay=None, **kw):
    kw.setdefault("use_graph", True)
    d = pkg.DQN(S, minibatch=B, hidden=HID, memory=CAP, seed=3, gamma=GAMMA, beta=BETA, **kw)
    for net in range(4):
        d.set_params(net, _params(net))
    rp = replay or _replay()
    d.add_transitions_arrays(*[a[:100] for a in rp])
    d.add_transitions_arrays(*[a[100:] for a in rp])
    assert d.memory_size() == SIZE
    if per is not None:
        d.enable_prioritized_replay(**per)
    return d


@functools.lru_cache(maxsize=None)
def _reference():
    """float64 forward of the four nets over the 127 transitions the memory holds, logical order; computed once, never modified"""
    import torch
    from oracle import torch_ref
    s, a, r, mc, nx, term = (x[ADDED - SIZE:] for x in _replay())
    ref = torch_ref.TorchRef(B=32, S=S, hidden=HID, gamma=GAMMA, beta=BETA)
    w = [torch.as_tensor(_params(net), dtype=torch.float64) for net in range(4)]
    t = lambda x: torch.as_tensor(x, dtype=torch.float64)
    with torch.no_grad():
        mu = ref.actor(w[0], t(s))
        q = ref.critic(w[1], t(s), t(a))
        qp = ref.critic(w[1], t(s), mu)
        qt = ref.critic(w[3], t(nx), ref.actor(w[2], t(nx)))
        y = BETA * t(mc) + (1 - BETA) * torch.where(torch.as_tensor(term.astype(bool)), t(r), t(r) + GAMMA * qt)
    out = {"q": q.numpy(), "y": y.numpy(), "q_policy": qp.numpy(), "mu": mu.numpy(), "stored": a, "mc": mc, "reward": r, "terminal": term}
    for v in out.values():
        v.setflags(write=False)
    return out


def _window(first, n):
    return (first, SIZE - first) if n < 0 else (first, n)


def _chunk_indices(first, n, B, c):
    return np.minimum(first + c * B + np.arange(B), first + n - 1).astype(np.int32)


def _state(d, memory=True):
    """everything a sweep must leave as it was, as bytes"""
    out = [d.get_params(net).tobytes() for net in range(4)]
    out += [d.get_params(net, kind).tobytes() for net in (0, 1) for kind in (1, 2, 3)]
    out += [(d.actor_iter(), d.critic_iter()), tuple(sorted(d.per_state().items())), np.asarray(d.read_stats(), F).tobytes(), d.memory_size()]
    if memory:
        out += [a.tobytes() for a in d.read_memory(0, SIZE)]
    return out


def test_reference_has_no_tied_action(pkg):
    """the seed is chosen so that no row's two best unmasked logits lie within 1e-5, in mu(s) of the float64 reference or as stored:
    the device's float32 mu(s), within 1e-4 of it on values this size, cannot legitimately pick another action"""
    ref = _reference()
    for ao in (ref["mu"], ref["stored"]):
        top = np.sort(np.asarray(ao, np.float64)[:, [0, 1, 3]], axis=1)
        assert (top[:, 2] - top[:, 1]).min() > 1e-5
    m = W.get_action(ref["mu"]) == W.get_action(ref["stored"])
    assert 0 < m.sum() < SIZE                                     # both outcomes occur
    assert ref["terminal"][-1] == 1


@pytest.mark.parametrize("B", [32, 256])
@pytest.mark.parametrize("first,n", WINDOWS)
def test_rows_and_report(pkg, gpu, B, first, n):
    ref = _reference()
    d = _make(pkg, B)
    assert d.per_state()["enabled"] == 0
    out = d.evaluate_memory(first, n, rows=True)
    first, n = _window(first, n)
    rows, w = out["rows"], slice(first, first + n)
    assert out["n"] == n and out["first"] == first and out["n_chunks"] == (n + B - 1) // B
    assert all(len(rows[k]) == n for k in rows)
    if n == 0:
        assert out["n_terminal"] == out["n_action_match"] == 0 and int(out["td_hist"].sum()) == 0
        assert all(out[k] == {"min": 0.0, "max": 0.0, "sum": 0.0, "sum_sq": 0.0, "n_nonfinite": 0} for k in W.QUANTITIES)
        d.close()
        return
    for k in ("q", "y", "q_policy"):
        err = np.abs(rows[k].astype(np.float64) - ref[k][w]).max()
        print("B = %d window (%d, %d) %s: largest error %.3g, values up to %.3g" % (B, first, n, k, err, np.abs(ref[k][w]).max()))
        assert err <= Q_BOUND, (k, err)
    assert np.array_equal(rows["td"].view(np.uint32), (rows["q"] - rows["y"]).view(np.uint32))
    assert np.array_equal(rows["action_match"], (W.get_action(ref["mu"]) == W.get_action(ref["stored"]))[w].astype(np.int32))
    # the report from the device's own per-row arrays
    full = {k: np.zeros(SIZE, F) for k in ("q", "y", "q_policy")}
    for k in full:
        full[k][w] = rows[k]
    host = W.rows_of(full["q"], full["y"], full["q_policy"], ref["mc"], ref["reward"], ref["terminal"], ref["mu"], ref["stored"])
    W.compare(out, W.report(host, first, n, B, (0, 0)))
    assert out["n_terminal"] > 0 and out["td"]["sum_sq"] > 0
    d.close()


@pytest.mark.parametrize("B", [32, 256])
def test_chunks_match_the_update_bit_for_bit(pkg, gpu, B):
    """every chunk — the padded tail included — against dqnhip_update on the same B indices on a fresh identical learner
    (DQNHIP_TUNE_SEPARATE_Q_TRAIN: see the module's docstring), read back with debug_read"""
    d = _make(pkg, B)
    rows = d.evaluate_memory(0, -1, rows=True)["rows"]
    n_chunks = (SIZE + B - 1) // B
    last_q_target = d.debug_read("q_target")                      # what the last chunk left
    for c in range(n_chunks):
        idx = _chunk_indices(0, SIZE, B, c)
        e = _make(pkg, B, tuning=pkg.capi.TUNE_SEPARATE_Q_TRAIN)
        e.UpdateActorCritic(idx)
        valid = min(B, SIZE - c * B)
        for name, key in (("q_train", "q"), ("y", "y")):
            got, want = rows[key][c * B:c * B + valid], e.debug_read(name)[:valid]
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (B, c, name)
        if c == n_chunks - 1:
            assert valid < B                                      # a padded tail at both sizes
            assert np.array_equal(last_q_target.view(np.uint32), e.debug_read("q_target").view(np.uint32)), (B, c)
            assert np.array_equal(d.debug_read("idx"), idx)
        e.close()
    d.close()


@pytest.mark.parametrize("B", [32, 256])
def test_sweeps_are_byte_identical_with_and_without_graphs(pkg, gpu, B):
    def sweep(d, first, n):
        cnt = _window(first, n)[1]
        arr = [np.zeros(cnt, F) for _ in range(4)] + [np.zeros(cnt, np.int32)]
        sr = pkg.capi.SweepRows()
        sr.struct_size = C.sizeof(pkg.capi.SweepRows)
        for k, a in zip(("q", "y", "td", "q_policy"), arr):
            setattr(sr, k, a.ctypes.data_as(pkg.capi.fp))
        sr.action_match = arr[4].ctypes.data_as(pkg.capi.ip)
        r = d.evaluate_memory_raw(first, n, sr)
        return [bytes(r)] + [a.tobytes() for a in arr]

    graph, eager = _make(pkg, B, use_graph=True), _make(pkg, B, use_graph=False)
    for first, n in WINDOWS:
        a = sweep(graph, first, n)
        assert sweep(graph, first, n) == a, (B, first, n)
        assert sweep(eager, first, n) == a, (B, first, n)
    graph.close(); eager.close()


@pytest.mark.parametrize("per", [False, True])
def test_a_sweep_leaves_the_learner_untouched(pkg, gpu, per):
    B = 32
    swept, plain = (_make(pkg, B, per=dict() if per else None) for _ in range(2))
    for d in (swept, plain):
        d.update_async_n(3)
    before = _state(swept)
    assert before == _state(plain)
    for first, n in WINDOWS:
        swept.evaluate_memory(first, n)
    assert _state(swept) == before
    # ... and what follows does not see that a sweep ran
    for d in (swept, plain):
        d.update_async_n(4)
    assert _state(swept) == _state(plain)
    swept.close(); plain.close()


def test_a_sweep_ends_a_chain(pkg, gpu):
    B = 32
    idx = [_chunk_indices(0, SIZE, B, c) for c in (1, 2)]
    chained, plain = _make(pkg, B), _make(pkg, B)
    got = [chained.UpdateActorCriticChained(idx[0], idx[1])]
    chained.evaluate_memory()                                     # overwrites the panels the first update gathered ahead
    got.append(chained.UpdateActorCriticChained(idx[1], None))
    want = [plain.UpdateActorCritic(i) for i in idx]
    assert np.array_equal(np.asarray(got, F).view(np.uint32), np.asarray(want, F).view(np.uint32))
    assert _state(chained) == _state(plain)
    chained.close(); plain.close()


def _levels(d):
    return [d.per_debug_read("level%d" % k) for k in range(d.per_state()["levels"] + 1)]


@pytest.mark.parametrize("first,n", [(0, -1), (5, 70)])
def test_refresh_rewrites_the_window(pkg, gpu, first, n):
    B, alpha, eps = 32, 0.6, 1e-6
    d = _make(pkg, B, per=dict(alpha=alpha, eps=eps))
    pr = np.random.default_rng(9).lognormal(0.0, 1.0, SIZE).astype(F)
    d.set_per_priorities(0, pr)
    p_max0 = d.per_state()["p_max"]
    weights = _state(d, memory=False)[:10]
    rep = d.per_refresh(first, n)
    first, n = _window(first, n)
    w = slice(first, first + n)
    assert rep["n"] == n and rep["td"]["n_nonfinite"] == 0
    leaf = d.per_priorities(0, SIZE)
    td = d.evaluate_memory(first, n, rows=True)["rows"]["td"]     # the same nets: the td the refresh saw (sweeps are deterministic)
    ok = W.leaf_matches(leaf[w], td, eps, alpha, ulps=2)
    assert ok.all(), (np.flatnonzero(~ok), leaf[w][~ok], W.refreshed_leaf(td, eps, alpha)[~ok])
    outside = np.ones(SIZE, bool)
    outside[w] = False
    assert np.array_equal(leaf[outside].view(np.uint32), pr[outside].view(np.uint32))
    lv = _levels(d)
    per_ref.check_tree(lv)
    assert np.array_equal(np.roll(lv[0][:CAP], -HEAD)[:SIZE].view(np.uint32), leaf.view(np.uint32))      # leaves sit at their physical slots
    assert d.per_state()["p_max"] == max(p_max0, float(leaf[w].max())) >= p_max0
    assert _state(d, memory=False)[:10] == weights
    d.close()


def test_refresh_leaves_the_leaf_of_a_non_finite_td(pkg, gpu):
    B, at = 32, 40
    d = _make(pkg, B, per=dict(), replay=_replay(nan_reward_at=at))
    pr = np.random.default_rng(9).lognormal(0.0, 1.0, SIZE).astype(F)
    d.set_per_priorities(0, pr)
    p_max0 = d.per_state()["p_max"]
    rep = d.per_refresh()
    assert rep["td"]["n_nonfinite"] == 1 and rep["y"]["n_nonfinite"] == 1 and rep["reward"]["n_nonfinite"] == 1 and rep["q"]["n_nonfinite"] == 0
    leaf = d.per_priorities(0, SIZE)
    assert leaf[at].view(np.uint32) == pr[at].view(np.uint32)
    assert (np.delete(leaf, at) != np.delete(pr, at)).all() and np.isfinite(leaf).all()
    per_ref.check_tree(_levels(d))
    assert d.per_state()["p_max"] >= p_max0
    d.read_stats()                                                # the sweep's non-finite target raised no sticky flag
    d.close()


def test_refusals_leave_the_learner_alone(pkg, gpu):
    B = 32
    idx = _chunk_indices(0, SIZE, B, 0)
    plain = _make(pkg, B)
    before = _state(plain)
    with pytest.raises(pkg.DQNFatal, match="dqnhip_per_refresh.*prioritized replay is not enabled"):
        plain.per_refresh()
    for first, n in ((0, SIZE + 1), (-1, 3), (SIZE + 1, -1), (100, 28), (0, -2)):
        with pytest.raises(pkg.DQNFatal, match="dqnhip_evaluate_memory.*window"):
            plain.evaluate_memory(first, n)
    assert _state(plain) == before
    plain.update_phase(0, idx)
    with pytest.raises(pkg.DQNFatal, match="dqnhip_evaluate_memory.*replay sweep.*phased update is in progress"):
        plain.evaluate_memory()
    plain.update_phase(1); plain.update_phase(2)
    ref = _make(pkg, B)
    ref.update_phase(0, idx); ref.update_phase(1); ref.update_phase(2)
    assert _state(plain) == _state(ref)
    plain.close(); ref.close()
    half = pkg.DQN(58, minibatch=128, hidden=(128, 128), memory=1024, seed=3, precision="fp16")
    half.add_transitions_arrays(*det_replay(7, 300, 58))
    before = [half.get_params(net).tobytes() for net in range(4)]
    with pytest.raises(pkg.DQNFatal, match="dqnhip_evaluate_memory.*replay sweep.*DQNHIP_FP16"):
        half.evaluate_memory()
    with pytest.raises(pkg.DQNFatal, match="dqnhip_per_refresh.*prioritized replay is not enabled"):
        half.per_refresh()
    half.enable_prioritized_replay()
    with pytest.raises(pkg.DQNFatal, match="dqnhip_per_refresh.*replay sweep.*DQNHIP_FP16"):
        half.per_refresh()
    assert [half.get_params(net).tobytes() for net in range(4)] == before
    half.close()


def test_data_parallel_learners_are_refused(pkg, gpu):
    """dp_world > 1 (no group yet) and a one-rank group after dqnhip_dp_init: the message names the sweep, the bits stay"""
    many = pkg.DQN(S, minibatch=32, hidden=HID, memory=CAP, seed=3, dp_world=2, dp_rank=0)
    many.add_transitions_arrays(*[a[:100] for a in _replay()])
    before = [many.get_params(net).tobytes() for net in range(4)]
    with pytest.raises(pkg.DQNFatal, match="dqnhip_evaluate_memory.*replay sweep.*data-parallel"):
        many.evaluate_memory()
    assert [many.get_params(net).tobytes() for net in range(4)] == before
    many.close()
    one = _make(pkg, 32)
    one.evaluate_memory()                                         # (its scratch and captured chunk exist when the group is formed)
    one.dp_init(pkg.DQN.dp_unique_id())
    before = _state(one)
    with pytest.raises(pkg.DQNFatal, match="dqnhip_evaluate_memory.*replay sweep.*data-parallel"):
        one.evaluate_memory()
    with pytest.raises(pkg.DQNFatal, match="dqnhip_per_refresh.*prioritized replay is not enabled"):
        one.per_refresh()
    assert _state(one) == before
    one.dp_destroy()
    one.evaluate_memory()                                         # a plain learner again
    one.close()


def test_a_sharer_that_joins_a_larger_ring_sweeps_all_of_it(pkg, gpu):
    """the sweep's scratch is counted in the ring's transitions: a learner that swept its own small memory and then joins a larger one
    (dqnhip_share_replay_memory) sweeps the whole larger memory, and reports what the owner reports (same nets, same transitions)"""
    B, big_cap, big_n = 32, 1024, 700
    small = _make(pkg, B)
    assert small.evaluate_memory()["n"] == SIZE
    owner = pkg.DQN(S, minibatch=B, hidden=HID, memory=big_cap, seed=3, gamma=GAMMA, beta=BETA, use_graph=True)
    for net in range(4):
        owner.set_params(net, _params(net))
    owner.add_transitions_arrays(*det_replay(9, big_n, S))
    owner.ShareReplayMemory(small)
    assert small.memory_size() == big_n
    want = owner.evaluate_memory(rows=True)
    got = small.evaluate_memory(rows=True)
    assert got["n"] == big_n and got["n_chunks"] == (big_n + B - 1) // B > (CAP + B - 1) // B
    for k in want["rows"]:
        assert np.array_equal(got["rows"][k].view(np.uint32), want["rows"][k].view(np.uint32)), k
    want.pop("rows"); got.pop("rows")
    assert want.pop("td_hist").tolist() == got.pop("td_hist").tolist() and want == got
    small.close(); owner.close()
