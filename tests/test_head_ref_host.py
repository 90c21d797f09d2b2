"""The head layers' float64 reference and comparator (tests/head_ref.py) against numpy-made "device read-backs": on the case list of
tests/test_gpu_head_layers.py it accepts a plain float32 evaluation of every quantity, and it rejects each fault the GPU test relies
on it to catch.  No GPU."""
import numpy as np
import pytest

import gemm_ref as G
import head_ref as R

F32 = np.float32


def kp0_of(case):
    """the critic's first-layer panel width (in_dim rounded up to 64): what the (kp0 + 8) u s rule of act2_1 counts; fp32 learners below
    1024 rows take the merged first layers"""
    return (case.S + R.NO + 63) // 64 * 64 if case.precision == "fp32" and case.B < 1024 and not case.tuning & R.SEP_CRITIC_L0 else None


_sim = {}


def sim(name):
    """the float32 evaluation of a case, computed once; callers copy what they change"""
    if name not in _sim:
        case = R.CASE_BY_NAME[name]
        inp = R.make_inputs(case)
        _sim[name] = (case, inp, R.simulate(case, inp))
    case, inp, o = _sim[name]
    return case, inp, dict(o)


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_comparator_accepts_the_float32_evaluation(name):
    case, inp, o = sim(name)
    stats = R.check_all(case, o, kp0=kp0_of(case))
    for key, v in stats.items():
        if key != "act2_1_branch_share":
            assert 0 < v[0] == v[1], (key, v)          # the "kernel" IS the yardstick here
    assert ("act2_1" in stats) == (kp0_of(case) is not None)
    # the edges are in the data: exact zeros at the tower tops, mu(s) outside its range on both sides, terminal and bootstrapping rows
    assert (o["act1"][:, list(R.ZERO_UNITS)] == 0).all() and (o["act3"][:, list(R.ZERO_UNITS)] == 0).all()
    assert (o["actor_out"][:, 1] > 1).any() and (o["actor_out"][:, 4] < 0).any()
    assert 0 < o["term"].sum() < case.B
    assert (o["dxc"] < 0).any() and (o["dxc"] > 0).any()


def test_branch_excuses_of_act2_1_on_the_seeds_used():
    """K ~ 128: the bound is ~1e-5 of the scale, so the reference alone should excuse a few 1e-5 of the elements.  A case has as few as
    2048 of them (one excused element is 4.9e-4 of that: below the cap of 1e-3, which check_all asserts per case), so the share is
    confirmed over all merged cases together."""
    near = total = 0
    for c in R.CASES:
        if kp0_of(c) is not None:
            case, inp, o = sim(c.name)
            n = case.B * case.hidden[0]
            share = R.check_all(case, o, kp0=kp0_of(case))["act2_1_branch_share"]
            assert share <= G.MAX_BRANCH_SHARE
            near += round(share * n); total += n
    assert total > 1e5 and near / total <= 1e-4, (near, total)


def test_a_fused_case_is_checked_through_its_twin():
    case, inp, o = sim("b32_h128")
    twin = dict(o)
    del o["dxc"]
    R.check_all(case, o, twin=twin)
    with pytest.raises(AssertionError, match="no twin"):
        R.check_all(case, o)
    o["dq_da"] = o["dq_da"].copy()
    o["dq_da"][7, 2] = np.nextafter(o["dq_da"][7, 2], F32(np.inf))
    with pytest.raises(AssertionError, match=r"dq_da \(against the twin.*\[7\]\[2\]"):
        R.check_all(case, o, twin=twin)


def test_what_does_not_survive_a_whole_update_may_be_absent():
    case, inp, o = sim("b32_h128_graph")
    for k in ("dz_c0", "g1", "act2_1", "act0", "actor_target_out", "loss"):
        del o[k]
    stats = R.check_all(case, o)
    assert "dz_a" in stats and "actor_head_dW|db" in stats and "critic_head_dW|db" not in stats


# ---- injected faults: one per rule ----------------------------------------------------------------------------------------------------------
FAULT_CASES = ["b32_h128", "b1408_h128_ticket", "h16_b1024_h128_ticket"]


def small_row(o):
    """a minibatch row whose tower top is among the smallest (transition rows are scaled by 2**-6 .. 2**6)"""
    return int(np.argmin(np.abs(o["act1"]).max(1)))


@pytest.mark.parametrize("name", FAULT_CASES)
def test_rejects_one_wrong_element_in_a_small_row(name):
    case, inp, o = sim(name)
    r = small_row(o)
    big = np.abs(o["dz_a"]).max()
    assert 0 < abs(o["dz_a"][r, 3]) < big * 2.0 ** -5    # (dz_a does not scale with the row; a unit at x == 0 carries the slope 0.01)
    o["dz_a"] = o["dz_a"].copy()
    o["dz_a"][r, 3] += F32(big * 2.0 ** -12)            # invisible in a norm, or against the panel's largest element
    with pytest.raises(AssertionError, match=r"dz_a\[%d\]\[3\]" % r):
        R.check_all(case, o)
    case, inp, o = sim(name)
    o["q_train"] = o["q_train"].copy()
    o["q_train"][r] *= F32(1 + 2.0 ** -12)
    with pytest.raises(AssertionError, match=r"q_train\[%d\]\[0\]" % r):
        R.check_all(case, o)


@pytest.mark.parametrize("name", FAULT_CASES)
def test_rejects_a_mask_of_one_at_zero(name):
    case, inp, o = sim(name)
    sc = R.static_scales(case)[0] if case.precision == "fp16" else 1.0
    wq = R.head_of(o["w1"], case.S + R.NO, case.hidden, False)[0][0]
    dz = (o["dq"][:, None] * wq[None, :]).astype(F32) * np.where(o["act3"] >= 0, F32(1), G.SLOPE32)      # y < 0 in place of y <= 0
    o["dz_c0"] = (dz * F32(sc)).astype(np.float16).astype(F32) if case.precision == "fp16" else dz.astype(F32)
    with pytest.raises(AssertionError, match=r"dz_c\(step1\)\[0\]\[3\]"):
        R.check_all(case, o)
    case, inp, o = sim(name)
    o["dz_c1"] = o["dz_c1"].copy()
    o["dz_c1"][:, 17] *= F32(100)
    with pytest.raises(AssertionError, match=r"dz_c\(seed\)\[0\]\[17\]"):
        R.check_all(case, o)


@pytest.mark.parametrize("name", FAULT_CASES)
def test_rejects_swapped_inversion_factors_in_one_column(name):
    case, inp, o = sim(name)
    o["dq_da"] = R.invert32(o["dxc"], o["actor_out"], swap_col=9)
    with pytest.raises(AssertionError, match=r"dq_da\[\d+\]\[9\]"):
        R.check_all(case, o)


@pytest.mark.parametrize("name", FAULT_CASES)
def test_rejects_a_missing_row_chunk_in_dW(name):
    case, inp, o = sim(name)
    H, B = case.hidden[-1], case.B
    keep = slice(0, B - B // 16)
    dW = (o["dq_da"][keep].T @ o["act1"][keep]).astype(F32)
    o["g0"] = o["g0"].copy()
    tail = o["g0"][-(R.NO * H + R.NO):]
    tail[:R.NA * H] = dW[:R.NA].ravel()
    tail[R.NA * H + R.NA:R.NA * H + R.NA + R.NP_ * H] = dW[R.NA:].ravel()
    with pytest.raises(AssertionError, match=r"actor_head_dW\|db\[0\]\[\d+\]"):
        R.check_all(case, o)
    case, inp, o = sim(name)
    o["g1"] = o["g1"].copy()
    o["g1"][-(H + 1):-1] = (o["dq"][None, keep] @ o["act3"][keep]).astype(F32)[0]
    with pytest.raises(AssertionError, match=r"critic_head_dW\|db\[0\]\[\d+\]"):
        R.check_all(case, o)


@pytest.mark.parametrize("name", FAULT_CASES)
def test_rejects_db_of_the_wrong_head(name):
    case, inp, o = sim(name)
    H = case.hidden[-1]
    o["g0"] = o["g0"].copy()
    tail = o["g0"][-(R.NO * H + R.NO):]
    ba, bp = tail[R.NA * H:R.NA * H + R.NA], tail[-R.NP_:]
    ba[2] = bp[3]                                      # action_layer's db[2] takes actionpara_layer's db[3]
    with pytest.raises(AssertionError, match=r"actor_head_dW\|db\[2\]\[%d\]" % H):
        R.check_all(case, o)


@pytest.mark.parametrize("name", FAULT_CASES)
def test_rejects_a_terminal_row_that_bootstraps(name):
    case, inp, o = sim(name)
    t = int(np.argmax(o["term"] != 0))
    o["y"] = o["y"].copy()
    o["y"][t] = R.td_target(o["q_target"], o["reward"], o["mc"], np.zeros_like(o["term"]))[t]
    with pytest.raises(AssertionError, match=r" y\[%d\]\[0\]" % t):
        R.check_all(case, o)


@pytest.mark.parametrize("name", FAULT_CASES)
def test_rejects_gamma_q_formed_in_float(name):
    case, inp, o = sim(name)
    off = np.where(o["term"] != 0, o["reward"], (o["reward"] + F32(R.GAMMA) * o["q_target"]).astype(F32))
    o["y"] = (R.BETA * o["mc"].astype(np.float64) + (1 - R.BETA) * off.astype(np.float64)).astype(F32)
    with pytest.raises(AssertionError, match=r" y\[\d+\]\[0\]"):
        R.check_all(case, o)


def test_rejects_a_wrong_first_layer_epilogue_and_a_wrong_loss():
    case, inp, o = sim("b32_h128")
    o["act2_1"] = o["act2_1"].copy()
    r = small_row(o)
    o["act2_1"][r, 5] += F32(np.abs(o["act2_1"]).max() * 2.0 ** -12)
    with pytest.raises(AssertionError, match=r"act2_1\[%d\]\[5\]" % r):
        R.check_all(case, o, kp0=kp0_of(case))
    case, inp, o = sim("b32_h128")
    o["loss"] *= 1 + 1e-4
    with pytest.raises(AssertionError, match="loss"):
        R.check_all(case, o)
    case, inp, o = sim("b32_h128")
    o["dq"] = (o["dq"] * F32(1 + 2.0 ** -20)).astype(F32)
    with pytest.raises(AssertionError, match=r" dq\[\d+\]\[0\]"):
        R.check_all(case, o)


def test_the_tight_rule_rejects_a_sloppy_but_bounded_product():
    """a head dot product evaluated with an 11-bit mantissa operand stays inside (H + 8) u s at H = 1024 but not inside 4 x the yardstick"""
    case, inp, o = sim("b32_h1024_qtrain")
    W, b = R.head_of(o["w0"], case.S, case.hidden, True)
    x = o["act1"]
    lo = (x.astype(np.float64) @ W.astype(np.float64).T) * (1 + 200 * R.U) + b
    o["actor_out"] = lo.astype(F32)
    o["dq_da"] = R.invert32(o["dxc"], o["actor_out"])
    with pytest.raises(AssertionError, match=r"tight bound: .* actor_out"):
        R.check_all(case, o)
