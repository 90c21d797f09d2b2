"""Update diagnostics on the device (dqnhip_diag_collect / DQN.diagnostics()): every record of the report against tests/diag_ref.py,
the reference always computed from what get_params / debug_read / per_debug_read return right after the collection.  The bounds
are the comparator's (integers, bins, maxima and minima exact; double sums within 2 n 2^-53 sum |term|; step within the float32
roundings of its expression) — tests/test_diag_ref_host.py shows what they reject.

Shapes, the smallest at which each thing can go wrong:
  A  fp32, B = 32, S = 59, hidden (64, 128): odd input widths pad both first layers (59 -> 64, 69 -> 128), layers of different widths,
     blobs 1, 4 and 6 rows long
  B  fp32, B = 64, S = 58, hidden (128, 64, 64), prioritized replay
  C  fp16, B = 128, S = 58, hidden (128, 128)
  E  fp32, B = 32, S = 58, hidden (512, 256): one blob of 131072 elements — many chunks and workgroups for one segment"""
import ctypes as C

import numpy as np
import pytest

import diag_ref as R
from synth import det_indices, synth_replay

pytestmark = pytest.mark.gpu

F = np.float32
CAP, N = 4096, 2048
SHAPES = {"A": dict(S=59, B=32, hidden=(64, 128)),
          "B": dict(S=58, B=64, hidden=(128, 64, 64), per=True),
          "C": dict(S=58, B=128, hidden=(128, 128), precision="fp16"),
          "E": dict(S=58, B=32, hidden=(512, 256))}


def _make(pkg, S, B, hidden, per=False, seed=3, **kw):
    kw.setdefault("use_graph", True)
    d = pkg.DQN(S, minibatch=B, hidden=hidden, memory=CAP, seed=seed, **kw)
    d.add_transitions_arrays(*synth_replay(np.random.default_rng(5), N, S, mean_len=10))
    if per:
        d.enable_prioritized_replay()
    return d


def _reference(d, S, hidden, per=False):
    """from the read-backs, as they are now"""
    c = d.cfg
    cfg = {"lr": (c.actor_lr, c.critic_lr), "beta1": c.momentum, "beta2": c.momentum2, "delta": c.delta, "clip": c.clip_gradients}
    w = {net: d.get_params(net) for net in range(4)}
    g, m, v = ({net: d.get_params(net, kind) for net in (0, 1)} for kind in (3, 1, 2))
    panels = {(p, i): d.debug_read("act%d_%d" % (p, i)) for p in range(5) for i in range(1, len(hidden) + 1)}
    rows = {k: d.debug_read(k) for k in ("q_target", "y", "q_train", "q_policy", "terminal", "actor_out", "dq_da")}
    pr = {k: d.per_debug_read(k) for k in ("w", "prob", "td_abs")} if per else None
    return R.reference(S, hidden, cfg, w, g, m, v, (d.actor_iter(), d.critic_iter()), panels, rows, pr)


def _check(d, S, hidden, per=False):
    dev = d.diagnostics()
    ref = _reference(d, S, hidden, per)
    R.compare(dev, ref)
    return dev, ref


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_record_after_three_updates(pkg, gpu, shape):
    kw = dict(SHAPES[shape])
    d = _make(pkg, **kw)
    S, hidden, per = kw["S"], kw["hidden"], kw.get("per", False)
    idx = det_indices(11, 3, kw["B"], N)
    for u in range(3):
        loss, avg_q = d.UpdateActorCritic(idx[u])
    dev, ref = _check(d, S, hidden, per)
    assert dev["actor_iter"] == dev["critic_iter"] == 3
    assert np.array_equal(np.array([dev["critic_loss"], dev["avg_q"]], F), np.array([loss, avg_q], F))
    assert len(dev["blobs"]) == 4 * len(hidden) + 6 and len(dev["panels"]) == 5 * len(hidden)
    assert [b["layer"] for b in dev["blobs"]] == [b["layer"] for b in ref["blobs"]]
    # something was there to be measured: gradients, steps and lags are not all zero, some units are on the leaky branch
    assert all(b["g"]["sum_sq"] > 0 and b["step"]["sum_abs"] > 0 and b["lag"]["sum_abs"] > 0 for b in dev["blobs"])
    assert all(0 < p["n_negative"] < p["rows"] * p["cols"] for p in dev["panels"])
    assert (dev["loss_scale"] is not None) == (kw.get("precision") == "fp16")
    if shape == "E":
        assert max(b["count"] for b in dev["blobs"]) == 131072
    d.close()


@pytest.mark.parametrize("form", ["async_n", "chained", "no_graph"])
def test_every_record_after_other_update_forms(pkg, gpu, form):
    kw = dict(SHAPES["A"])
    d = _make(pkg, use_graph=form != "no_graph", **kw)
    idx = det_indices(13, 4, kw["B"], N)
    if form == "async_n":
        d.update_async_n(5)
    elif form == "chained":
        d.UpdateActorCriticChained(idx[0], idx[1])
        d.UpdateActorCriticChained(idx[1], idx[2])        # the prediction held: this update's gather rode in the last one
    else:
        for u in range(3):
            d.UpdateActorCritic(idx[u])
    dev, _ = _check(d, kw["S"], kw["hidden"])
    assert dev["critic_iter"] == {"async_n": 5, "chained": 2, "no_graph": 3}[form]
    d.close()


SPECIALS = np.array([0.0, -0.0, 1e-45, 2.0 ** -41, 2.0 ** -40, 2.0 ** -39, 2.0 ** 23, 2.0 ** 24, np.inf, -np.inf, np.nan, -(2.0 ** -40)], F)


def test_planted_values(pkg, gpu):
    """no update in between: what set_params wrote is what the collection reads"""
    kw = dict(SHAPES["A"])
    S, hidden = kw["S"], kw["hidden"]
    d = _make(pkg, **kw)
    d.UpdateActorCritic(det_indices(17, 1, kw["B"], N)[0])
    d.set_iters(3, 3)
    rng = np.random.default_rng(23)
    table = R.blob_table(S, hidden)
    for net in (0, 1):
        n = d.param_count(net)
        k0 = S if net == 0 else S + 10                              # layer 0 is stored 64 / 128 wide: its last LOGICAL column
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-14, 8, n)).astype(F)
        pos = [r * k0 + k0 - 1 for r in (0, 1, 31, 63)] + [0, k0, n - 1, n - 2]
        pos += [e["offset"] for e in table if e["net"] == net] + [e["offset"] + e["count"] - 1 for e in table if e["net"] == net]
        for i, p in enumerate(pos):
            g[p] = SPECIALS[i % SPECIALS.size]
        g[rng.integers(0, n, 200)] = SPECIALS[rng.integers(0, SPECIALS.size, 200)]
        d.set_params(net, g, 3)
        w = (rng.standard_normal(n) * 0.05).astype(F)
        wt = w.copy()
        wt[::3] += (rng.standard_normal(wt[::3].size) * 1e-4).astype(F)
        w[[p for p in pos[:4]]] = SPECIALS[[8, 10, 0, 6]]                 # Inf, NaN, 0, 2^23 in the last logical column
        wt[pos[1]] = 1.0
        m = (rng.standard_normal(n) * 1e-3).astype(F)
        v = rng.uniform(0, 1e-5, n).astype(F)
        m[pos[0]], m[pos[2]], v[pos[3]], v[5], m[7] = np.inf, 0.0, 0.0, np.nan, 1e-45
        d.set_params(net, w, 0); d.set_params(net + 2, wt, 0); d.set_params(net, m, 1); d.set_params(net, v, 2)
    dev, ref = _check(d, S, hidden)
    b0 = dev["blobs"][0]
    assert b0["count"] == 64 * 59 and b0["g"]["n_nonfinite"] >= 1 and b0["g"]["n_zero"] >= 2 and b0["w"]["n_nonfinite"] == 2
    assert b0["g_hist"][0] >= 2 and b0["g_hist"][63] >= 2 and np.isfinite([b0["g"]["sum_sq"], b0["g"]["max_abs"], b0["lag"]["sum_abs"]]).all()
    assert b0["lag"]["n_nonfinite"] == 2 and b0["step"]["n_nonfinite"] >= 1
    assert not np.isfinite(d.get_params(0, 3)).all()
    # the same twice, nothing in between: byte-identical reports (NaN / Inf content included)
    a, b = d.diag_collect_raw(), d.diag_collect_raw()
    assert bytes(a) == bytes(b)
    d.close()


def test_dead_unit(pkg, gpu):
    kw = dict(SHAPES["A"])
    S, hidden = kw["S"], kw["hidden"]
    d = _make(pkg, **kw)
    e = [b for b in R.blob_table(S, hidden) if b["net"] == 1 and b["layer"] == "ip1_layer" and b["is_bias"]][0]
    for net in (1, 3):
        w = d.get_params(net)
        w[e["offset"] + 5] = -10.0
        d.set_params(net, w)
    d.UpdateActorCritic(det_indices(19, 1, kw["B"], N)[0])
    dev, ref = _check(d, S, hidden)
    L = len(hidden)
    for p in (2, 3, 4):
        assert dev["panels"][p * L]["dead_units"] >= 1 and dev["panels"][p * L]["dead_units"] == ref["panels"][p * L]["dead_units"]
        assert (d.debug_read("act%d_1" % p)[:, 5] < 0).all()
    d.close()


def test_two_collections_are_byte_identical(pkg, gpu):
    for shape in ("A", "C"):
        kw = dict(SHAPES[shape])
        d = _make(pkg, **kw)
        d.update_async_n(3)
        a, b = d.diag_collect_raw(), d.diag_collect_raw()
        assert bytes(a) == bytes(b) and a.n_blobs == 4 * len(kw["hidden"]) + 6
        d.close()


def test_collecting_does_not_interfere(pkg, gpu):
    kw = dict(SHAPES["A"])
    a, b = _make(pkg, **kw), _make(pkg, **kw)
    idx = det_indices(29, 6, kw["B"], N)
    for u in range(6):
        ra, rb = a.UpdateActorCritic(idx[u]), b.UpdateActorCritic(idx[u])
        assert np.array_equal(np.asarray(ra, F).view(np.uint32), np.asarray(rb, F).view(np.uint32))
        a.diagnostics()
    for net in range(4):
        assert np.array_equal(a.get_params(net).view(np.uint32), b.get_params(net).view(np.uint32))
    for net in (0, 1):
        for kind in (1, 2, 3):
            assert np.array_equal(a.get_params(net, kind).view(np.uint32), b.get_params(net, kind).view(np.uint32))
    assert a.update_plan() == b.update_plan()
    a.update_async_n(4); b.update_async_n(4)
    a.diagnostics()
    a.update_async_n(4); b.update_async_n(4)
    for net in range(4):
        assert np.array_equal(a.get_params(net).view(np.uint32), b.get_params(net).view(np.uint32))
    a.close(); b.close()


def test_grad_norm_and_clip_scale(pkg, gpu):
    kw = dict(SHAPES["A"])
    idx = det_indices(31, 2, kw["B"], N)
    for clip in (1e-3, -1.0):
        d = _make(pkg, clip_grad=clip, **kw)
        for u in range(2):
            d.UpdateActorCritic(idx[u])
        dev, ref = _check(d, kw["S"], kw["hidden"])
        for net in (0, 1):
            norm = np.sqrt(sum(b["g"]["sum_sq"] for b in dev["blobs"] if b["net"] == net))
            assert norm > 0 and abs(dev["grad_norm"][net] - norm) <= 4 * R.U53 * norm
            # ... and the norm of the gradient as get_params returns it (numpy's pairwise double sum: far inside 1e-12)
            g = d.get_params(net, 3).astype(np.float64)
            assert abs(dev["grad_norm"][net] - np.sqrt((g * g).sum())) <= 1e-12 * norm
            if clip > 0 and norm > clip:
                assert dev["clip_scale"][net] < 1 and abs(dev["clip_scale"][net] - F(clip) / norm) <= 4 * R.U53
            else:
                assert dev["clip_scale"][net] == 1.0
        if clip > 0:
            assert dev["clip_scale"][1] < 1            # the critic's gradient norm of this workload is far above 1e-3
        d.close()


def test_refusals(pkg, gpu):
    kw = dict(SHAPES["A"])
    d = _make(pkg, **kw)
    idx = det_indices(37, 1, kw["B"], N)[0]
    d.update_phase(0, idx)
    with pytest.raises(pkg.DQNFatal) as e:
        d.diagnostics()
    assert "diagnostics" in str(e.value) and "phased update is in progress" in str(e.value)
    d.update_phase(1); d.update_phase(2)
    _check(d, kw["S"], kw["hidden"])
    other = _make(pkg, seed=4, **kw)
    d.ShareParameters(other, 1, 1)
    with pytest.raises(pkg.DQNFatal) as e:
        other.diagnostics()
    assert "diagnostics" in str(e.value) and "another learner's parameters" in str(e.value)
    d.UpdateActorCritic(idx)
    _check(d, kw["S"], kw["hidden"])                    # the owner is fine
    r = pkg.capi.DiagReport()
    assert d.lib.dqnhip_diag_collect(d.h, C.byref(r)) != 0 and b"struct_size" in d.lib.dqnhip_last_error()
    other.close(); d.close()


def test_step_is_zero_at_iteration_zero(pkg, gpu):
    kw = dict(SHAPES["A"])
    d = _make(pkg, **kw)
    rng = np.random.default_rng(41)
    for net in (0, 1):
        n = d.param_count(net)
        d.set_params(net, (rng.standard_normal(n) * 1e-3).astype(F), 1)
        d.set_params(net, rng.uniform(0, 1e-5, n).astype(F), 2)
    dev, _ = _check(d, kw["S"], kw["hidden"])
    assert dev["actor_iter"] == dev["critic_iter"] == 0
    for b in dev["blobs"]:
        assert b["step"]["n_zero"] == b["count"] and b["step"]["sum_abs"] == 0 and b["step"]["max_abs"] == 0
    d.set_iters(1, 1)
    dev, _ = _check(d, kw["S"], kw["hidden"])
    assert all(b["step"]["sum_abs"] > 0 for b in dev["blobs"])
    d.close()
