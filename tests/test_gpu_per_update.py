"""Prioritized replay: the weighted critic step (k_head_q_train_w), the write-back (k_per_update) and how a prioritized learner's
updates are scheduled.  At uniform priorities (alpha = 0, beta0 = 0) every weight is 1.0f exactly and the learner is bit-identical
to a plain one; with weights the per-element figures are checked from the read-backs against tests/per_ref.py.
No reference counterpart (the reference samples uniformly and weights nothing, src/dqn.cpp:501-509, 892-906).

The two powf results — w = (pmin / prob)^beta and the new leaf (|td| + eps)^alpha — against their float64 values rounded to float32,
measured on this file's inputs on an MI355X: at most 1 ulp (w, 32 values between 0.002 and 1) and 2 ulp (leaf, 32 values).  Asserted:
twice that, 2 and 4 ulp (docs/MEASUREMENTS.md)."""
import numpy as np
import pytest

import per_ref as R
from synth import det_indices, synth_replay

pytestmark = pytest.mark.gpu

B, S, HID, CAP, N = 32, 58, (64, 64), 4096, 2048
F = np.float32
W_ULP, LEAF_ULP = 2, 4          # twice the measured largest distance (see above); never more than 16


def _make(pkg, per=None, B=B, hidden=HID, n=N, replay=None, **kw):
    d = pkg.DQN(S, minibatch=B, hidden=hidden, memory=CAP, seed=3, **kw)
    d.add_transitions_arrays(*(replay or synth_replay(np.random.default_rng(5), n, S, mean_len=10)))
    if per is not None:
        d.enable_prioritized_replay(**per)
    return d


def _bits(d):
    """the four weight arenas, then m and v (KIND_M = 1, KIND_V = 2) of the two online nets"""
    out = [d.get_params(net).view(np.uint32) for net in range(4)]
    out += [d.get_params(net, kind).view(np.uint32) for net in (0, 1) for kind in (1, 2)]
    return out


def _tree(d):
    st = d.per_state()
    return [d.per_debug_read("level%d" % k).view(np.uint32) for k in range(st["levels"] + 1)] + [np.array([st["p_max"]], F).view(np.uint32)]


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_uniform_priorities_are_bit_identical_to_a_plain_learner(pkg, gpu, precision):
    """alpha = 0, beta0 = 0, explicit indices, three updates: weights, m, v, loss and avg_q equal a plain learner's bit for bit —
    fp32 against the DQNHIP_TUNE_SEPARATE_Q_TRAIN form (k_head_q_train in a launch of its own), fp16 against the plain fp16 learner"""
    kw = dict(B=128, hidden=(128, 128), precision="fp16") if precision == "fp16" else dict(tuning=pkg.capi.TUNE_SEPARATE_Q_TRAIN)
    kw_p = dict(kw); kw_p.pop("tuning", None)
    plain = _make(pkg, **kw)
    prio = _make(pkg, per=dict(alpha=0.0, beta0=0.0), **kw_p)
    idx = det_indices(11, 3, kw.get("B", B), N)
    for u in range(3):
        want, got = plain.UpdateActorCritic(idx[u]), prio.UpdateActorCritic(idx[u])
        assert np.array_equal(np.asarray(got, F).view(np.uint32), np.asarray(want, F).view(np.uint32)), (precision, u, got, want)
        assert (prio.per_debug_read("w") == 1.0).all()
        for g, w in zip(_bits(prio), _bits(plain)):
            assert np.array_equal(g, w), (precision, u)
    # alpha = 0: every written leaf is 1
    assert set(np.unique(prio.per_priorities(0, N))) == {F(1.0)}
    plain.close(); prio.close()


def test_weighted_step_per_element(pkg, gpu):
    """beta0 = 1, spread priorities, explicit indices, one update"""
    alpha, eps = 0.6, 1e-6
    d = _make(pkg, per=dict(alpha=alpha, beta0=1.0, eps=eps))
    pr = np.random.default_rng(9).lognormal(0.0, 1.5, N).astype(F)
    d.set_per_priorities(0, pr)
    total = d.per_state()["total"]
    idx = det_indices(13, 1, B, N)[0]
    loss, _ = d.UpdateActorCritic(idx)
    prob, w, td = d.per_debug_read("prob"), d.per_debug_read("w"), d.per_debug_read("td_abs")
    q, y, dq = d.debug_read("q_train"), d.debug_read("y"), d.debug_read("dq")
    assert np.array_equal(prob.view(np.uint32), (pr[idx] / F(total)).view(np.uint32))
    assert np.array_equal(d.per_debug_read("slot"), idx)                 # head = 0: physical = logical
    print("w: largest ulp distance", R.check_weights(w, prob, 1.0, min(W_ULP, 16)), " spread", w.min(), w.max())
    assert w.max() == 1.0 and w.min() < 0.1
    dd = q - y                                                           # float32, as the kernel forms it
    assert np.array_equal(td.view(np.uint32), np.abs(dd).view(np.uint32))
    assert np.array_equal(dq.view(np.uint32), ((F(1.0) / F(B) * dd) * w).view(np.uint32))
    want = float((R.weights(prob, 1.0) * dd.astype(np.float64) ** 2).sum() / (2 * B))
    assert abs(loss - want) <= 1e-4 * max(1.0, abs(want)), (loss, want)
    leaf = d.per_priorities(0, N)
    print("leaf: largest ulp distance", R.check_write_back(leaf[idx], td, F(eps), alpha, min(LEAF_ULP, 16)))
    rest = np.setdiff1d(np.arange(N), idx)
    assert np.array_equal(leaf[rest], pr[rest])
    # p_max is the running maximum
    assert d.per_state()["p_max"] == max(1.0, pr.max(), leaf[idx].max())
    lv = [d.per_debug_read("level%d" % k) for k in range(d.per_state()["levels"] + 1)]
    R.check_tree(lv)
    d.close()


def test_p_max_is_the_running_maximum(pkg, gpu):
    d = _make(pkg, per=dict(alpha=1.0, beta0=0.5))
    seen = 1.0
    for u in range(4):
        d.UpdateActorCritic()
        seen = max(seen, float(d.per_priorities(0, N).max()))
        assert d.per_state()["p_max"] == seen
    # a transition appended now gets it
    d.add_transitions_arrays(*synth_replay(np.random.default_rng(6), 10, S, mean_len=10))
    assert (d.per_priorities(N, 10) == F(seen)).all()
    d.close()


def test_non_finite_td_error_leaves_its_leaf(pkg, gpu):
    replay = list(synth_replay(np.random.default_rng(5), N, S, mean_len=10))
    replay[2] = replay[2].copy(); replay[2][7] = np.inf                 # one transition's reward
    d = _make(pkg, per=dict(), replay=replay)
    idx = np.arange(B, dtype=np.int32)
    before = d.per_priorities(0, B)
    with pytest.raises(pkg.DQNFatal, match="Target not finite!"):
        d.UpdateActorCritic(idx)
    after = d.per_priorities(0, B)
    assert after[7] == before[7] == 1.0 and not np.isfinite(d.per_debug_read("td_abs")[7])
    assert (np.delete(after, 7) != 1.0).all() and np.isfinite(after).all()
    lv = [d.per_debug_read("level%d" % k) for k in range(d.per_state()["levels"] + 1)]
    R.check_tree(lv)
    d.close()


def test_beta_is_annealed_on_the_device(pkg, gpu):
    d = _make(pkg, per=dict(alpha=0.6, beta0=0.4, beta_anneal_iters=4))
    d.set_per_priorities(0, np.random.default_rng(9).lognormal(0.0, 1.0, N).astype(F))
    for it in range(7):
        beta = R.beta_now(0.4, 4, it)                                    # 0.4, 0.55, 0.7 (half way), 0.85, 1, 1, 1
        assert d.critic_iter() == it and abs(d.per_state()["beta_now"] - beta) < 1e-6
        d.UpdateActorCritic()
        R.check_weights(d.per_debug_read("w"), d.per_debug_read("prob"), float(F(beta)), 16)
    assert R.beta_now(0.4, 4, 2) == pytest.approx(0.7) and d.per_state()["beta_now"] == 1.0
    d.close()


@pytest.mark.parametrize("use_graph", [True, False])
def test_update_async_n_is_five_single_updates(pkg, gpu, use_graph):
    a = _make(pkg, per=dict(seed=5), use_graph=use_graph)
    b = _make(pkg, per=dict(seed=5), use_graph=use_graph)
    c = _make(pkg, per=dict(seed=5), use_graph=not use_graph)
    a.update_async_n(5)
    for d in (b, c):
        for u in range(5):
            d.update_async(None)
    want = _bits(a) + _tree(a) + [np.asarray(a.read_stats(), F).view(np.uint32)]
    for d in (b, c):
        for g, w in zip(_bits(d) + _tree(d) + [np.asarray(d.read_stats(), F).view(np.uint32)], want):
            assert np.array_equal(g, w)
    assert a.per_state()["next_counter"] == 5
    for d in (a, b, c):
        d.close()


def test_plan_of_a_prioritized_learner(pkg, gpu):
    """B = 64 into three 1024-wide layers: a plain learner takes k_dgrad_qtrain and gathers early here (tests/test_gpu_kernel_timing.py)"""
    kw = dict(B=64, hidden=(1024, 1024, 1024), use_graph=True)
    plain, d = _make(pkg, **kw), _make(pkg, per=dict(), **kw)
    pp, pd = plain.update_plan(), d.update_plan()
    print(pp, pd)
    assert {"q_train_in_dgrad", "early_gather_l0"} <= set(pp["forms"]) and "prioritized" not in pp["forms"]
    assert "prioritized" in pd["forms"] and not ({"q_train_in_dgrad", "early_gather_l0"} & set(pd["forms"]))
    assert set(pd["forms"]) - {"prioritized"} == set(pp["forms"]) - {"q_train_in_dgrad", "early_gather_l0"}
    sep = _make(pkg, tuning=pkg.capi.TUNE_SEPARATE_Q_TRAIN, **kw)
    # sampler + write-back on top of the DQNHIP_TUNE_SEPARATE_Q_TRAIN form's launches; in a graph: the same sequence back to back
    assert pd["launches_single"] == sep.update_plan()["launches_single"] + 2
    assert pd["launches_graph_first"] == pd["launches_in_graph"] == pd["launches_single"]
    for x in (plain, d, sep):
        x.close()


def test_the_outlier_is_found(pkg, gpu):
    """oracle-free: 256 transitions, one with reward 100, B = 256 on indices 0 .. 255: after one update the outlier's leaf is the
    largest, and 100 sample-only minibatches hit it at about p / total, against about 1 / 256 before"""
    replay = [x[:256].copy() for x in synth_replay(np.random.default_rng(5), 300, S, mean_len=10)]
    replay[2][100] = 100.0; replay[3][100] = 100.0                      # reward and on-policy target
    d = _make(pkg, per=dict(alpha=0.6, beta0=0.4), B=256, replay=replay)
    idx0, _ = d.per_sample(0, 100)
    before = (idx0 == 100).mean()
    assert abs(before - 1 / 256) < 2e-3
    d.UpdateActorCritic(np.arange(256))
    leaf = d.per_priorities(0, 256)
    assert leaf.argmax() == 100
    share = float(leaf[100]) / float(leaf.sum(dtype=np.float64))
    idx1, _ = d.per_sample(1, 100)
    after = (idx1 == 100).mean()
    print("outlier: p / total", share, "hit rate before", before, "after", after)
    assert share > 10 / 256 and abs(after - share) <= 5 * np.sqrt(share / (100 * 256)) + 1 / 256
    d.close()


def test_refusals_name_prioritized_replay(pkg, gpu):
    d = _make(pkg, per=dict())
    other = _make(pkg)
    idx = np.arange(B, dtype=np.int32)
    m = "prioritized replay"
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
        d.ShareReplayMemory(other)
    with pytest.raises(pkg.DQNFatal, match=m):
        other.ShareReplayMemory(d)
    with pytest.raises(pkg.DQNFatal, match="already enabled"):
        d.enable_prioritized_replay()
    # enabling on a learner that already shares a ring, or that is one rank of several
    third = _make(pkg)
    other.ShareReplayMemory(third)
    for x in (other, third):
        with pytest.raises(pkg.DQNFatal, match=m):
            x.enable_prioritized_replay()
    rank = pkg.DQN(S, minibatch=B, hidden=HID, memory=CAP, seed=3, dp_world=2, dp_rank=0)
    with pytest.raises(pkg.DQNFatal, match=m):
        rank.enable_prioritized_replay()
    d.UpdateActorCritic(idx)                                             # and the learner still works
    assert all(np.isfinite(d.read_stats()))
    for x in (rank, third, other, d):
        x.close()
