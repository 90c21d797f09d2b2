"""The float64 reference and comparator of the fp16 launches (tests/hgemm_ref.py) against numpy-made "kernel outputs", on exactly
the case lists and seeds of tests/test_gpu_hgemm_forms.py: it accepts the float32 yardstick written into the output panels (C16,
C32, CS16, the partials, db and the head sums, the converted panels), no case's reference plus bound reaches fp16's 65504, and it
rejects each fault the GPU tests rely on it to catch.  No GPU."""
import numpy as np
import pytest

import hgemm_ref as H

SINGLE = H.single_cases()
GROUPED = H.grouped_cases()


def filled(pr, outs=None):
    pr.reset_outputs()
    pr.write_outputs(pr.float32_product() if outs is None else outs)
    return pr


# ---- accepts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", H.PADS)
@pytest.mark.parametrize("regime", H.REGIMES)
def test_accepts_the_float32_yardstick_on_every_gemm_case(regime, pad):
    worst = 0.0
    for name, form, fn in SINGLE + GROUPED:
        for i, pr in enumerate(fn(regime, pad)):
            tag = f"{name} {regime} pad {pad} problem {i}"
            pr.assert_no_overflow(tag)
            st = filled(pr).check(tag)
            assert 0 < st["yard_r"] <= pr.K + H.EXTRA_ROUNDINGS, (tag, st)
            # C32: the yardstick's own r over the columns below n_valid32; C16: the smallest r consistent with the rounded values
            assert st["kernel_r"] <= st["yard_r"], (tag, st)
            worst = max(worst, st["yard_r"])
    print(f"yardstick max r over all cases, {regime} pad {pad}: {worst:.3f}")


@pytest.mark.parametrize("pad", H.PADS)
@pytest.mark.parametrize("regime", H.REGIMES)
def test_accepts_the_float32_riders(regime, pad):
    for form, rows, nh in H.GROUP_CASES:
        wg, db, head = H.group_case(form, rows, nh, regime, pad)
        tag = f"{H.FORM_NAME[form]} rows {rows} nh {nh} {regime} pad {pad}"
        for pr in wg:
            filled(pr).check(tag)
        filled(db, db.float32_outputs()).check(tag)
        if head is not None:
            filled(head, head.float32_outputs()).check(tag)
    for rows in H.DB16_ROWS:
        for widths in H.DB16_WIDTHS:
            db = H.db16_case(rows, widths, regime, pad)
            filled(db, db.float32_outputs()).check(f"db16 rows {rows}")
    cv = H.cvt_case(regime, pad)
    filled(cv, cv.float32_outputs()).check("cvt16")


# ---- rejects -------------------------------------------------------------------------------------------------------------------------
def fwd(regime="scaled", pad=64, **kw):
    return H.make(H.NT_SMALL_FWD, H.FWD, 128, 192, 256, regime, pad, "host", **kw)


def wgrad(regime="scaled", pad=64, **kw):
    return H.make(H.NT_SMALL_WGRAD, H.WGRAD, 128, 192, 256, regime, pad, "host", **kw)


def test_rejects_an_unwritten_element_and_a_nan():
    pr = filled(fwd())
    pr.out["C16"].bitview()[37, 5] = H.SENT16
    with pytest.raises(AssertionError, match=r"not finite: .*C16\[37\]\[5\]"):
        pr.check("case")
    pr = filled(wgrad())
    pr.out["C32"].view()[3, 63] = np.nan
    with pytest.raises(AssertionError, match=r"not finite: .*C32\[3\]\[63\]"):
        pr.check()
    pr = filled(wgrad())
    pr.out["sumsq_partial"].bitview()[0, 4] = H.SENT32                     # one tile's slot never written
    with pytest.raises(AssertionError, match=r"not finite: .*sumsq_partial\[0\]\[4\]"):
        pr.check()


def test_rejects_touched_guard_pad_and_n_valid32_words():
    pr = filled(fwd())
    p = pr.out["C16"]
    p.buf[p.offset + p.rows * p.ld + 3] = 0.0                              # first guard row behind the output
    with pytest.raises(AssertionError, match=r"C16 guard row, buffer row 128 col 3"):
        pr.check()
    pr = filled(fwd(seed_w=True))
    p = pr.out["CS16"]
    p.buf[p.offset + 7 * p.ld + p.cols] = 0.0                              # row 7, first pad column
    with pytest.raises(AssertionError, match=r"CS16 pad column, buffer row 7 col 192"):
        pr.check()
    # a column at n_valid32 in a row other than 0 (the test this replaces read row 0 only): dense pitch, so that the word is no pad
    # of the buffer but a column the kernel owns and must not write
    pr = filled(wgrad(pad=0, n_valid32=128))
    p = pr.out["C32"]
    assert p.ld == 192 and p.cols == 128
    p.buf[p.offset + 77 * p.ld + 128] = 0.0
    with pytest.raises(AssertionError, match=r"C32 pad column, buffer row 77 col 128"):
        pr.check()


@pytest.mark.parametrize("kind", ["C16", "C32"])
def test_rejects_a_dropped_term_in_a_small_row(kind):
    """row 0 and column 0 carry the scale 2**-4 each: element (0, 0) is 2**-16 of the largest elements' size.  The global figure the old test
    used (2e-5 max|ref| after forgiving one fp16 ulp) cannot see its largest term missing; the per-element rule does."""
    pr = fwd() if kind == "C16" else wgrad()
    A = pr.Aop.copy()
    kk = int(np.abs(A[0].astype(np.float32) * pr.Bop[0].astype(np.float32)).argmax())
    A[0, kk] = 0
    outs = pr.float32_product()
    short = pr.float32_product(Aop=A)
    ref = pr.reference()["ref"]
    scale = pr.scale32 if kind == "C32" else 1.0
    assert abs(float(short["y"][0, 0]) - ref[0, 0]) * scale <= 2e-5 * np.abs(ref).max() * scale      # what the global figure allows
    outs[kind][0, 0] = short[kind][0, 0]
    filled(pr, outs)
    with pytest.raises(AssertionError, match=rf"outside the derived (bound|interval): .*{kind}\[0\]\[0\]"):
        pr.check()


def truncate16(y):
    """float32 -> fp16 rounded toward zero"""
    h = y.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(y)
    h[over] = np.nextafter(h[over], np.float16(0))
    return h


@pytest.mark.parametrize("regime", H.REGIMES)
@pytest.mark.parametrize("fault", ["twice", "truncated"])
def test_rejects_a_wrongly_rounded_fp16_output(fault, regime):
    """a second rounding (the fp32 value cut to bf16's 8 bits first) and truncation in place of round-to-nearest"""
    pr = fwd(regime=regime)
    outs = pr.float32_product()
    y = outs["y"]
    if fault == "twice":
        outs["C16"] = (y.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float16)
    else:
        outs["C16"] = truncate16(y)
    assert (outs["C16"].view(np.uint16) != y.astype(np.float16).view(np.uint16)).any()
    filled(pr, outs)
    with pytest.raises(AssertionError, match=r"outside the derived interval: .*C16\["):
        pr.check()


def test_rejects_a_head_seed_from_the_float64_sign():
    """an element whose pre-activation is positive and rounds to fp16 zero: the kernel's CS16 follows the C16 it wrote (factor 0.01), a
    seed taken from the sign of the exact pre-activation (factor 1) is wrong"""
    pr = fwd(regime="uniform", seed_w=True)
    pr.Aop[0, :] = 0
    pr.bias[0] = np.float32(1e-8)
    pr.refresh()
    outs = pr.float32_product()
    assert pr.reference()["pre"][0, 0] > 0 and outs["C16"][0, 0] == 0
    filled(pr, outs).check()
    fac = np.where(pr.reference()["pre"] > 0, np.float32(1), H.SLOPE32)
    outs["CS16"] = (((-pr.seed_w)[None, :] * fac) * np.float32(pr.seed_scale)).astype(np.float16)
    filled(pr, outs)
    with pytest.raises(AssertionError, match=r"head seed: .*CS16\[0\]\[0\]"):
        pr.check()


def test_rejects_a_wrong_sum_of_squares():
    pr = filled(wgrad())
    pr.out["sumsq_partial"].view()[0, 3] = 0.0
    with pytest.raises(AssertionError, match=r"sum-of-squares partials"):
        pr.check()
    pr = filled(wgrad())
    pr.out["sumsq_partial"].view()[0, 3] *= -1
    with pytest.raises(AssertionError, match=r"negative sum-of-squares slot"):
        pr.check()


@pytest.mark.parametrize("nh", [1, 10])
def test_rejects_a_head_sum_without_one_row_group(nh):
    hd = H.HeadRider(384, 192, nh, seed=5, regime="scaled")
    filled(hd, hd.float32_outputs()).check()
    dy = hd.dy.copy()
    dy[32:64] = 0                                                        # one 32-row step of the tail loop left out
    outs = hd.float32_outputs()
    outs["dW"] = hd.float32_outputs(dy)["dW"]
    filled(hd, outs)
    with pytest.raises(AssertionError, match=r"outside the derived bound: .*dW\["):
        hd.check()


def test_rejects_a_column_sum_without_its_tail_rows():
    db = H.DbRider(192, [128], seed=6, regime="scaled", pad=64)
    outs = db.float32_outputs()
    outs["db0"] = (db.dy[0][:160].astype(np.float32).sum(0, dtype=np.float32) * np.float32(db.scale))
    filled(db, outs)
    with pytest.raises(AssertionError, match=r"outside the derived bound: .*db0\[0\]"):
        db.check()
    outs = db.float32_outputs()
    outs["db_sumsq"][1] = 0
    filled(db, outs)
    with pytest.raises(AssertionError, match=r"sum-of-squares partials: .*db_sumsq\[1\]"):
        db.check()


def test_rejects_cvt16_faults():
    cv = H.cvt_case("scaled", 64)
    filled(cv, cv.float32_outputs())
    cv.out["dst0"].bitview()[5, 100] = 0x8000                            # a pad column holding -0
    with pytest.raises(AssertionError, match=r"cvt16: .*dst0\[5\]\[100\].*pad column"):
        cv.check()
    filled(cv, cv.float32_outputs())
    cv.out["dst0"].bitview()[5, 3] ^= 1                                  # one ulp off
    with pytest.raises(AssertionError, match=r"cvt16: .*dst0\[5\]\[3\]"):
        cv.check()
    filled(cv, cv.float32_outputs())
    p = cv.out["dst2"]
    p.raw[p.offset + 96 * p.ld] = 0                                      # the first row beyond `rows`
    with pytest.raises(AssertionError, match=r"dst2 guard row, buffer row 96 col 0"):
        cv.check()
