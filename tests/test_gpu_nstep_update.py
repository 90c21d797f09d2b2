"""N-step returns through whole updates: an n = 1 learner is the 1-step learner bit for bit; an n-step learner on a replay X equals a
plain learner with discount gamma^n on X relabelled by tests/nstep_ref.py (that pins the arithmetic of k_gather_n and
k_head_q_train_n together); prioritized replay composes; graphs, refusals, the plan, resume.  Every comparison is on bits."""
import numpy as np
import pytest

import nstep_ref as R
from synth import det_indices, synth_replay

pytestmark = pytest.mark.gpu

B, S, HID, CAP, N = 32, 58, (64, 64), 4096, 2048
F = np.float32
GAMMA = 0.99


def _replay():
    return synth_replay(np.random.default_rng(5), N, S, mean_len=10)        # (its last record is terminal)


def _make(pkg, n_step=None, per=None, B=B, hidden=HID, replay=None, **kw):
    d = pkg.DQN(S, minibatch=B, hidden=hidden, memory=CAP, seed=3, **kw)
    d.add_transitions_arrays(*(replay or _replay()))
    if per is not None:
        d.enable_prioritized_replay(**per)
    if n_step is not None:
        d.enable_n_step(n_step)
    return d


def _bits(d):
    """the four weight arenas, then m and v (KIND_M = 1, KIND_V = 2) of the two online nets"""
    out = [d.get_params(net).view(np.uint32) for net in range(4)]
    out += [d.get_params(net, kind).view(np.uint32) for net in (0, 1) for kind in (1, 2)]
    return out


def _same(a, b, what):
    for k, (g, w) in enumerate(zip(_bits(a), _bits(b))):
        assert np.array_equal(g, w), (what, "arena", k)


def _shape(pkg, precision):
    """the two shapes the prioritized learner's tests compare at: fp32 against the DQNHIP_TUNE_SEPARATE_Q_TRAIN form (k_head_q_train in
    a launch of its own), fp16 against the plain fp16 learner"""
    if precision == "fp16":
        return dict(B=128, hidden=(128, 128), precision="fp16"), dict(B=128, hidden=(128, 128), precision="fp16")
    return dict(tuning=pkg.capi.TUNE_SEPARATE_Q_TRAIN), dict()


def _three_updates(plain, other, bsz, what):
    idx = det_indices(11, 3, bsz, N)
    for u in range(3):
        want, got = plain.UpdateActorCritic(idx[u]), other.UpdateActorCritic(idx[u])
        assert np.array_equal(np.asarray(got, F).view(np.uint32), np.asarray(want, F).view(np.uint32)), (what, u, got, want)
        _same(other, plain, (what, u))


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_n_1_is_bit_identical_to_a_plain_learner(pkg, gpu, precision):
    kw_plain, kw = _shape(pkg, precision)
    plain, one = _make(pkg, **kw_plain), _make(pkg, n_step=1, **kw)
    _three_updates(plain, one, kw.get("B", B), precision)
    assert (one.n_step_debug_read("steps") == 1).all() and (one.n_step_debug_read("disc") == GAMMA).all()
    plain.close(); one.close()


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("n", [3, 5])
def test_n_step_equals_a_plain_learner_on_the_relabelled_replay(pkg, gpu, precision, n):
    """X ends on a terminal record, so every window either ends on a terminal transition (no bootstrap) or has m = n (discount
    gamma^n, the plain learner's gamma — the same float64 products)"""
    X = _replay()
    assert X[5][-1] == 1
    g = R.gather(X[2], X[5], np.arange(N), n, GAMMA)
    assert ((g["terminal"] == 1) | (g["steps"] == n)).all() and (g["steps"] == n).sum() > N // 4
    kw_plain, kw = _shape(pkg, precision)
    plain = _make(pkg, replay=R.relabel(X, n, GAMMA), gamma=float(R.discount(GAMMA, n)), **kw_plain)
    multi = _make(pkg, n_step=n, replay=X, gamma=GAMMA, **kw)
    _three_updates(plain, multi, kw.get("B", B), (precision, n))
    plain.close(); multi.close()


def test_prioritized_replay_composes(pkg, gpu):
    alone, both = _make(pkg, n_step=3), _make(pkg, n_step=3, per=dict(alpha=0.0, beta0=0.0))
    _three_updates(alone, both, B, "uniform priorities")
    assert (both.per_debug_read("w") == 1.0).all()
    alone.close(); both.close()
    # default alpha and beta: what is written back is |q - y_n|
    d = _make(pkg, n_step=3, per=dict())
    idx = det_indices(13, 1, B, N)[0]
    d.UpdateActorCritic(idx)
    q, y, td = d.debug_read("q_train"), d.debug_read("y"), d.per_debug_read("td_abs")
    assert np.array_equal(td.view(np.uint32), np.abs(q - y).view(np.uint32))
    want = R.gather(_replay()[2], _replay()[5], idx, 3, GAMMA)
    assert np.array_equal(d.n_step_debug_read("steps"), want["steps"]) and (want["steps"] > 1).any()
    assert np.array_equal(d.debug_read("y").view(np.uint32),
                          R.target(want["reward"], want["disc"], d.debug_read("q_target"), want["terminal"], _replay()[3][idx], 0.5).view(np.uint32))
    # the sampler feeds the gather: device-sampled updates run, and the rows are the sampler's
    d.UpdateActorCritic()
    assert np.array_equal(d.debug_read("idx").astype(np.int64), (d.per_debug_read("slot") - 0) % CAP)      # head = 0: physical = logical
    d.close()


@pytest.mark.parametrize("use_graph", [True, False])
def test_update_async_n_is_five_single_updates(pkg, gpu, use_graph):
    a, b = _make(pkg, n_step=5, use_graph=use_graph), _make(pkg, n_step=5, use_graph=not use_graph)
    a.update_async_n(5)
    for u in range(5):
        b.UpdateActorCritic()
    _same(a, b, use_graph)
    assert np.array_equal(np.asarray(a.read_stats(), F).view(np.uint32), np.asarray(b.read_stats(), F).view(np.uint32))
    assert np.array_equal(a.debug_read("idx"), b.debug_read("idx")) and np.array_equal(a.n_step_debug_read("steps"), b.n_step_debug_read("steps"))
    assert a.n_step_debug_read("steps").max() > 1
    a.close(); b.close()


def test_refusals_name_n_step_returns(pkg, gpu):
    d = _make(pkg, n_step=3)
    idx = np.arange(B, dtype=np.int32)
    m = "n-step returns"
    with pytest.raises(pkg.DQNFatal, match=m):
        d.UpdateActorCriticChained(idx, idx)
    with pytest.raises(pkg.DQNFatal, match=m):
        d.UpdateActorCriticPipelined(idx)
    with pytest.raises(pkg.DQNFatal, match=m):
        d.update_indexed_n(np.stack([idx, idx]))
    with pytest.raises(pkg.DQNFatal, match=m):
        d.update_phase(0, idx)
    with pytest.raises(pkg.DQNFatal, match=m):
        d.dp_init(pkg.DQN.dp_unique_id())
    with pytest.raises(pkg.DQNFatal, match=m):
        d.evaluate_memory()
    both = _make(pkg, n_step=3, per=dict())                               # (a refresh needs priorities to refresh)
    with pytest.raises(pkg.DQNFatal, match=m):
        both.per_refresh()
    for bad in (0, -1, 65):
        with pytest.raises(pkg.DQNFatal, match=m):
            d.enable_n_step(bad)
    assert d.n_step() == 3
    rank = pkg.DQN(S, minibatch=B, hidden=HID, memory=CAP, seed=3, dp_world=2, dp_rank=0)
    with pytest.raises(pkg.DQNFatal, match=m):
        rank.enable_n_step(3)
    never = _make(pkg)
    with pytest.raises(pkg.DQNFatal, match="not enabled"):
        never.n_step_debug_read("steps")
    for x in (d, both):                                                    # and the learners still work
        x.UpdateActorCritic(idx)
        assert all(np.isfinite(x.read_stats()))
    for x in (never, rank, both, d):
        x.close()


def test_plan_of_an_n_step_learner(pkg, gpu):
    """B = 64 into three 1024-wide layers: a plain learner takes k_dgrad_qtrain and gathers early here; an n-step learner runs the
    DQNHIP_TUNE_SEPARATE_Q_TRAIN form's launches (k_gather_n and k_head_q_train_n in k_gather's and k_head_q_train's places: not one
    launch more), a prioritized one its sampler and write-back on top — the two launches a prioritized learner adds"""
    kw = dict(B=64, hidden=(1024, 1024, 1024), use_graph=True)
    plain, d, both, prio = _make(pkg, **kw), _make(pkg, n_step=3, **kw), _make(pkg, n_step=3, per=dict(), **kw), _make(pkg, per=dict(), **kw)
    sep = _make(pkg, tuning=pkg.capi.TUNE_SEPARATE_Q_TRAIN, **kw)
    pp, pd, pb, ps = plain.update_plan(), d.update_plan(), both.update_plan(), sep.update_plan()
    print(pp, pd, pb)
    assert {"q_train_in_dgrad", "early_gather_l0"} <= set(pp["forms"]) and "n_step" not in pp["forms"]
    assert "n_step" in pd["forms"] and not ({"q_train_in_dgrad", "early_gather_l0", "prioritized"} & set(pd["forms"]))
    assert set(pd["forms"]) - {"n_step"} == set(pp["forms"]) - {"q_train_in_dgrad", "early_gather_l0"}
    assert {"n_step", "prioritized"} <= set(pb["forms"])
    assert pd["launches_single"] == ps["launches_single"]
    assert pd["launches_graph_first"] == pd["launches_in_graph"] == pd["launches_single"]
    assert pb["launches_single"] == prio.update_plan()["launches_single"] == ps["launches_single"] + 2
    assert pb["launches_graph_first"] == pb["launches_in_graph"] == pb["launches_single"]
    for x in (plain, d, both, prio, sep):
        x.close()


def test_resume_continues_bit_for_bit(pkg, gpu, tmp_path):
    path = str(tmp_path / "learner.state")
    a = _make(pkg, n_step=3)
    for u in range(2):
        a.UpdateActorCritic()
    a.save_state(path)
    b = pkg.DQN(S, minibatch=B, hidden=HID, memory=CAP, seed=3)
    b.enable_n_step(3)                           # a hyper-parameter, not state: the file does not hold it
    b.load_state(path)
    assert b.n_step() == 3
    for u in range(2):
        want, got = a.UpdateActorCritic(), b.UpdateActorCritic()
        assert np.array_equal(np.asarray(got, F).view(np.uint32), np.asarray(want, F).view(np.uint32))
        assert np.array_equal(a.debug_read("idx"), b.debug_read("idx"))
        assert np.array_equal(a.n_step_debug_read("reward").view(np.uint32), b.n_step_debug_read("reward").view(np.uint32))
        _same(a, b, ("resumed", u))
    a.close(); b.close()
