"""tests/diag_ref.py against known answers worked out by hand, and its comparator against the mistakes a device reduction can make:
each is rejected, on data chosen so that the rejection is by a wide margin (the margins are asserted).  No GPU."""
import copy
import math

import numpy as np
import pytest

import diag_ref as R

F = np.float32


def test_histogram_bins_known_answers():
    # bin k in 1..62 holds 2^(k-40) <= |x| < 2^(k-39); bin 0 everything below 2^-39; bin 63 everything from 2^23 up
    assert R.bin_of(F(2.0 ** -40)) == 0
    assert R.bin_of(np.nextafter(F(2.0 ** -40), F(0))) == 0
    assert R.bin_of(F(2.0 ** -39)) == 1
    assert R.bin_of(np.nextafter(F(2.0 ** -39), F(0))) == 0
    assert R.bin_of(F(1.0)) == 40 and R.bin_of(F(-1.5)) == 40 and R.bin_of(F(2.0)) == 41
    assert R.bin_of(F(2.0 ** 22)) == 62
    assert R.bin_of(F(2.0 ** 23)) == 63
    assert R.bin_of(F(2.0 ** 24)) == 63
    assert R.bin_of(F(1e-45)) == 0                      # the smallest denormal: exponent field 0
    assert R.bin_of(F(3.4e38)) == 63
    x = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 2.0 ** -40, 1e-45, 2.0 ** 24], F)
    h = R.histogram(x)
    assert h.sum() == 4 and h[40] == 1 and h[0] == 2 and h[63] == 1            # +-0, Inf and NaN are not binned
    m = R.moments(x)
    assert (m["count"], m["n_zero"], m["n_nonfinite"]) == (9, 2, 3)
    assert h.sum() + m["n_zero"] + m["n_nonfinite"] == m["count"]
    assert m["max_abs"] == 2.0 ** 24 and m["sum_sq"] == 1.0 + 2.0 ** -80 + float(F(1e-45)) ** 2 + 2.0 ** 48
    assert R.moments(np.array([np.nan, np.inf], F))["max_abs"] == 0.0


def test_invariant_on_random_data():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(5000) * 10.0 ** rng.uniform(-20, 10, 5000)).astype(F)
    x[::97] = 0
    x[5::211] = np.nan
    m = R.moments(x)
    assert R.histogram(x).sum() + m["n_zero"] + m["n_nonfinite"] == m["count"] == 5000


def test_dead_units_on_a_4x3_panel():
    a = np.array([[-1.0, -1.0, 0.5],
                  [-2.0, 0.0, -1.0],
                  [-0.5, -3.0, -1.0],
                  [-1e-30, -1.0, -1.0]], F)
    p = R.panel_record(3, 1, a)
    # column 0: negative in every row -> dead; column 1 holds a zero (not < 0); column 2 a positive value
    assert p["dead_units"] == 1 and p["n_negative"] == 10 and (p["rows"], p["cols"]) == (4, 3)
    assert p["a"]["n_zero"] == 1 and p["a"]["count"] == 12
    assert R.panel_record(0, 1, np.array([[-0.0], [-1.0]], F))["dead_units"] == 0         # -0.0 is not < 0
    assert R.panel_record(0, 1, np.array([[np.nan], [-1.0]], F))["dead_units"] == 0


def test_blob_table_matches_the_parameter_count():
    S, hidden = 59, (64, 128)
    t = R.blob_table(S, hidden)
    a, c = [b for b in t if b["net"] == 0], [b for b in t if b["net"] == 1]
    assert len(a) == 2 * 2 + 4 and len(c) == 2 * 2 + 2
    assert [b["shape"] for b in a] == [(64, 59), (64,), (128, 64), (128,), (4, 128), (4,), (6, 128), (6,)]
    assert [b["shape"] for b in c] == [(64, 69), (64,), (128, 64), (128,), (1, 128), (1,)]
    assert [b["layer"] for b in a][::2] == ["ip1_layer", "ip2_layer", "action_layer", "actionpara_layer"]
    assert [b["layer"] for b in c][::2] == ["ip1_layer", "ip2_layer", "q_values_layer"]
    for net, bl in ((0, a), (1, c)):
        assert bl[-1]["offset"] + bl[-1]["count"] == R.param_count(S, hidden, net)
        assert all(x["offset"] + x["count"] == y["offset"] for x, y in zip(bl, bl[1:]))
    assert R.param_count(S, hidden, 0) == 64 * 59 + 64 + 128 * 64 + 128 + 10 * 128 + 10 == 13450
    assert R.param_count(S, hidden, 1) == 64 * 69 + 64 + 128 * 64 + 128 + 128 + 1 == 12929


# ---- the comparator -----------------------------------------------------------------------------------------------------------
S, HID, B = 59, (64, 128), 32
CFG = {"lr": (1e-5, 1e-3), "beta1": 0.95, "beta2": 0.999, "delta": 1e-8, "clip": 10.0}


def _inputs(seed=0, hidden=HID):
    rng = np.random.default_rng(seed)
    n = [R.param_count(S, hidden, net) for net in (0, 1)]
    w = {net: (rng.standard_normal(n[net & 1]) * 0.05).astype(F) for net in range(4)}
    g = {net: (rng.standard_normal(n[net]) * 10.0 ** rng.uniform(-8, 0, n[net])).astype(F) for net in (0, 1)}
    m = {net: (rng.standard_normal(n[net]) * 1e-3).astype(F) for net in (0, 1)}
    v = {net: (rng.uniform(0, 1e-4, n[net])).astype(F) for net in (0, 1)}
    panels = {}
    for p in range(5):
        for i, wd in enumerate(hidden):
            a = rng.standard_normal((B, wd)).astype(F)
            a[a < 0] *= F(0.01)
            a[:, 3] = -np.abs(a[:, 3]) - F(1e-3)        # a dead unit
            a[5, 7] = 0.0
            panels[(p, i + 1)] = a
    rows = {k: rng.standard_normal(B).astype(F) for k in ("q_target", "y", "q_train", "q_policy")}
    rows["terminal"] = (rng.uniform(size=B) < 0.2).astype(F)
    ao = rng.uniform(-1.2, 1.2, (B, 10)).astype(F)
    ao[:, 4:] *= F(120.0)
    rows["actor_out"] = ao
    rows["dq_da"] = rng.standard_normal((B, 10)).astype(F)
    return dict(w=w, g=g, m=m, v=v, iters=(3, 3), panels=panels, rows=rows)


def _ref(inp, hidden=HID, per=None):
    return R.reference(S, hidden, CFG, inp["w"], inp["g"], inp["m"], inp["v"], inp["iters"], inp["panels"], inp["rows"], per)


def _rejected(dev, ref, what):
    with pytest.raises(R.Mismatch) as e:
        R.compare(dev, ref)
    assert what in str(e.value), str(e.value)
    return str(e.value)


def test_comparator_accepts_the_reference_against_itself():
    ref = _ref(_inputs())
    R.compare(copy.deepcopy(ref), ref)
    assert len(ref["blobs"]) == 14 and len(ref["panels"]) == 10
    assert all(p["dead_units"] == 1 for p in ref["panels"])
    assert 0 < ref["clip_scale"][0] < 1                       # the random gradients are far above the clip
    per = {"w": np.linspace(0.1, 1, B).astype(F), "prob": np.linspace(1e-4, 1e-3, B).astype(F), "td_abs": np.linspace(0, 2, B).astype(F)}
    refp = _ref(_inputs(), per=per)
    R.compare(copy.deepcopy(refp), refp)
    _rejected(copy.deepcopy(ref), refp, "has_per")


def test_comparator_rejects_a_bin_shifted_by_one():
    ref = _ref(_inputs())
    dev = copy.deepcopy(ref)
    dev["blobs"][2]["g_hist"] = np.roll(dev["blobs"][2]["g_hist"], 1)
    _rejected(dev, ref, "g_hist")
    dev = copy.deepcopy(ref)
    dev["panels"][4]["hist"] = np.roll(dev["panels"][4]["hist"], -1)
    _rejected(dev, ref, "hist")


def test_comparator_rejects_counted_pad_columns():
    """layer 0 of S = 59 is stored 64 wide: a reduction over the stored image counts 5 zero pad words per row"""
    inp = _inputs()
    ref = _ref(inp)
    dev = copy.deepcopy(ref)
    for k in ("w", "g", "lag", "step"):
        dev["blobs"][0][k]["count"] += 64 * 5
        dev["blobs"][0][k]["n_zero"] += 64 * 5
    _rejected(dev, ref, "blob 0")
    # ... the sums alone would not notice (zeros add nothing): it is the integer fields that catch it
    dev2 = copy.deepcopy(ref)
    dev2["blobs"][0]["g"]["n_zero"] += 64 * 5
    _rejected(dev2, ref, "n_zero")


def test_comparator_rejects_a_missing_chunk():
    hidden = (512, 256)
    inp = _inputs(1, hidden)
    ref = _ref(inp, hidden)
    e = R.blob_table(S, hidden)[2]                            # ip2 weights: 131072 elements
    assert e["count"] == 131072
    w = inp["w"][0][e["offset"]:e["offset"] + e["count"]]
    part = R.moments(w[4096:])                               # one 4096-element chunk dropped from the sums, counts intact
    dev = copy.deepcopy(ref)
    dev["blobs"][2]["w"]["sum_abs"], dev["blobs"][2]["w"]["sum_sq"] = part["sum_abs"], part["sum_sq"]
    full = ref["blobs"][2]["w"]
    bound = 2 * 131072 * R.U53 * full["sum_abs"]
    assert full["sum_abs"] - part["sum_abs"] > 1e6 * bound   # the margin: the chunk is 3 % of the sum, the bound 3e-11 of it
    _rejected(dev, ref, "sum_abs")


def test_comparator_rejects_a_float32_accumulated_sum():
    rng = np.random.default_rng(2)
    x = rng.uniform(0.5, 1.0, 65536).astype(F)
    ref = R.moments(x)
    acc = F(0)
    for c in x.reshape(-1, 256):                             # a float32 accumulator over 256 partials (better than element-wise)
        acc = F(acc + F(c.astype(np.float64).sum()))
    dev = dict(ref)
    dev["sum_abs"] = float(acc)
    bound = 2 * 65536 * R.U53 * ref["sum_abs"]
    assert abs(dev["sum_abs"] - ref["sum_abs"]) > 100 * bound, (dev["sum_abs"], ref["sum_abs"], bound)
    with pytest.raises(R.Mismatch):
        R.compare_moments("x", dev, ref)
    R.compare_moments("x", dict(ref), ref)


def test_comparator_rejects_max_abs_as_the_signed_maximum():
    x = np.array([0.25, -3.0, 1.5], F)
    ref = R.moments(x)
    assert ref["max_abs"] == 3.0
    dev = dict(ref)
    dev["max_abs"] = float(x.max())
    with pytest.raises(R.Mismatch):
        R.compare_moments("x", dev, ref)


def test_comparator_rejects_dead_units_counting_zero():
    inp = _inputs()
    inp["panels"][(2, 1)][:, 9] = 0.0                          # a column of zeros: <= 0 everywhere, < 0 nowhere
    ref = _ref(inp)
    dev = copy.deepcopy(ref)
    a = inp["panels"][(2, 1)]
    wrong = int((a <= 0).all(axis=0).sum())
    assert wrong == ref["panels"][4]["dead_units"] + 1
    dev["panels"][4]["dead_units"] = wrong
    _rejected(dev, ref, "dead_units")


def test_comparator_rejects_a_lag_formed_in_float32():
    """w and w' one part in 2^10 apart: the float32 difference of values near 1 is exact (Sterbenz), so the data are chosen where it
    is not — w near 1, w' near 1e-3 times random: the float32 subtraction rounds at 2^-24 relative of ~1, the exact one does not"""
    rng = np.random.default_rng(3)
    w = rng.uniform(1.0, 2.0, 4096).astype(F)
    wt = (rng.uniform(1.0, 2.0, 4096) * 1e-3).astype(F)
    exact = w.astype(np.float64) - wt.astype(np.float64)
    rounded = (w - wt).astype(np.float64)
    assert (exact != rounded).mean() > 0.9
    ref, dev = R.moments(exact), R.moments(rounded)
    bound = 2 * 4096 * R.U53 * ref["sum_abs"]
    assert abs(dev["sum_abs"] - ref["sum_abs"]) > 100 * bound or abs(dev["sum_sq"] - ref["sum_sq"]) > 100 * 2 * 4096 * R.U53 * ref["sum_sq"]
    with pytest.raises(R.Mismatch):
        R.compare_moments("lag", dev, ref)
    R.compare_moments("lag", R.moments(exact), ref)


def test_step_is_zero_at_iteration_zero_and_matches_the_expression():
    m, v = np.array([1e-3, -2e-3], F), np.array([1e-6, 4e-6], F)
    assert (R.adam_step(m, v, 1e-3, 0.95, 0.999, 1e-8, 0) == 0).all()
    t = 3
    corr = math.sqrt(1 - float(F(0.999)) ** t) / (1 - float(F(0.95)) ** t)
    want = 1e-3 * corr * np.array([1e-3 / (1e-3 + 1e-8), -2e-3 / (2e-3 + 1e-8)])
    got = R.adam_step(m, v, 1e-3, 0.95, 0.999, 1e-8, t)
    assert np.allclose(got, want, rtol=1e-6)
