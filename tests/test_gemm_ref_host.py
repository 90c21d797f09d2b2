"""The float64 GEMM reference and comparator (tests/gemm_ref.py) against numpy-made "kernel outputs": it accepts the plain
float32 product of every mode and epilogue, and rejects each fault the GPU tests rely on it to catch.  No GPU."""
import numpy as np
import pytest

import gemm_ref as G

REGIMES = ["uniform", "scaled"]


def filled(pr, **subst):
    """the problem with its outputs written by the float32 numpy product"""
    pr.reset_outputs()
    G.write_outputs(pr, G.float32_product(pr, **subst))
    return pr


def problems(regime, pad):
    yield G.Problem(G.FWD, 128, 96, 512, seed=11, regime=regime, pad=pad, seed_w=True, dot_w=True)
    yield G.Problem(G.FWD, 64, 32, 64, seed=12, regime=regime, pad=pad, bias=False, relu=0, xcopy=(58, 10), p_width=128)
    yield G.Problem(G.DGRAD, 128, 48, 320, seed=13, regime=regime, pad=pad)
    yield G.Problem(G.DGRAD, 16, 32, 64, seed=14, regime=regime, pad=pad, col0=16, panel_w=64)
    yield G.Problem(G.WGRAD, 128, 192, 96, seed=15, regime=regime, pad=pad, bq=64)
    yield G.Problem(G.WGRAD, 64, 48, 32, seed=16, regime=regime, pad=pad, bq=16)


@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("regime", REGIMES)
def test_comparator_accepts_the_float32_product(regime, pad):
    for pr in problems(regime, pad):
        st = G.check(filled(pr))
        assert 0 < st["kernel_r"] == st["yard_r"] <= pr.red + G.EXTRA_ROUNDINGS


def fwd(regime="scaled", pad=64, k=512):
    return G.Problem(G.FWD, 128, 96, k, seed=21, regime=regime, pad=pad)


def test_rejects_an_element_left_as_sentinel():
    pr = filled(fwd())
    pr.out["C"].view().view(np.uint32)[37, 5] = G.SENTINEL_BITS
    with pytest.raises(AssertionError, match=r"not finite: .*C\[37\]\[5\]"):
        G.check(pr, "case")


def test_rejects_one_nan():
    pr = filled(G.Problem(G.WGRAD, 128, 64, 32, seed=22, pad=64, bq=64))
    pr.out["db"].view()[0, 63] = np.nan
    with pytest.raises(AssertionError, match=r"not finite: .*db\[0\]\[63\]"):
        G.check(pr)


def test_rejects_an_overwritten_guard_word():
    pr = filled(fwd())
    panel = pr.out["C"]
    panel.buf[panel.offset + panel.rows * panel.ld + 3] = 0.0          # first guard row behind the output, column 3
    with pytest.raises(AssertionError, match=r"guard row, buffer row 96 col 3"):
        G.check(pr)
    pr = filled(fwd())
    pr.out["C"].buf[pr.out["C"].offset - 1] = 1.0                       # the last word of the guard row in front (a pad column of it)
    with pytest.raises(AssertionError, match=r"guard row, buffer row -1"):
        G.check(pr)


def test_rejects_an_overwritten_pad_column():
    pr = filled(fwd())
    panel = pr.out["C"]
    panel.buf[panel.offset + 7 * panel.ld + panel.cols] = 0.0           # row 7, first pad column
    with pytest.raises(AssertionError, match=r"pad column, buffer row 7 col 128"):
        G.check(pr)
    # dgrad_narrow's addressing: a neighbouring column of the wider panel
    pr = filled(G.Problem(G.DGRAD, 16, 32, 64, seed=23, col0=16, panel_w=64))
    panel = pr.out["C"]
    panel.buf[panel.offset + 2 * panel.ld - 1] = 0.0                    # row 2, the column in front of the tile
    with pytest.raises(AssertionError, match=r"pad column, buffer row 2 col -1"):
        G.check(pr)


@pytest.mark.parametrize("k", [64, 512])
def test_rejects_a_dropped_term_in_a_small_row(k):
    """row 0 x column 0 carry the scale 2**-12: the error is far below what a max-abs figure scaled by the global maximum (the old
    yardstick: 4e-7 sqrt(K) max|ref|) can see, and outside the per-element bound"""
    pr = fwd(k=k)
    Q = pr.Q.copy()
    kk = int(np.abs(Q[0] * pr.P[0, :k]).argmax())
    Q[0, kk] = 0.0
    got = G.float32_product(pr)
    got["C"][0, 0] = G.float32_product(pr, Q=Q)["C"][0, 0]                # element (0, 0) alone lacks its largest term
    ref = G.reference(pr)["C"]
    err = np.abs(got["C"].astype(np.float64) - ref)
    allowed = 4e-7 * k ** 0.5 * np.abs(ref).max()                       # what the global figure allows
    assert err.max() <= allowed and err[0, 0] <= 0.01 * allowed         # the whole output passes it, the faulty element a hundred times over
    G.write_outputs(pr, got)
    with pytest.raises(AssertionError, match=r"outside the derived bound: .*C\[0\]\[0\]"):
        G.check(pr)


def round_to_11_bits(a):
    """round-to-nearest to an 11-bit significand (fp16's), exponent range untouched"""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((b + np.uint32(0x1000)) & np.uint32(0xFFFFE000)).view(np.float32)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("mode", [G.FWD, G.DGRAD, G.WGRAD])
def test_rejects_a_reduced_precision_product(mode, regime):
    pr = {G.FWD: lambda: G.Problem(G.FWD, 128, 96, 512, seed=31, regime=regime),
          G.DGRAD: lambda: G.Problem(G.DGRAD, 128, 96, 512, seed=32, regime=regime),
          G.WGRAD: lambda: G.Problem(G.WGRAD, 128, 128, 96, seed=33, regime=regime, bq=64)}[mode]()
    filled(pr, P=round_to_11_bits(pr.P), Q=round_to_11_bits(pr.Q))
    with pytest.raises(AssertionError, match=r"tight bound|outside the derived bound"):
        G.check(pr)


def test_rejects_wrong_epilogue_extras():
    mk = lambda: G.Problem(G.FWD, 128, 96, 512, seed=41, pad=64, seed_w=True, dot_w=True)
    pr = filled(mk())
    pr.out["C2"].view()[5, 9] *= np.float32(100.0) if abs(pr.out["C2"].view()[5, 9]) < 0.011 else np.float32(0.01)   # the other branch
    with pytest.raises(AssertionError, match=r"head seed: .*C2\[5\]\[9\]"):
        G.check(pr)
    pr = filled(mk())
    pr.out["dot_out"].view()[7, 3] -= pr.out["C"].view()[7, 3 * 16 + 15] * pr.dot_w[3 * 16 + 15]      # one column short
    with pytest.raises(AssertionError, match=r"outside the derived bound: .*dot_out\[7\]\[3\]"):
        G.check(pr)
    pr = filled(G.Problem(G.FWD, 64, 32, 64, seed=42, bias=False, relu=0, xcopy=(58, 10), p_width=128))
    v = pr.out["xcopy_dst"].view()
    v[[2, 3]] = v[[3, 2]]                                               # two columns swapped
    with pytest.raises(AssertionError, match=r"transposed copy: .*xcopy_dst\[2\]\[0\]"):
        G.check(pr)
    pr = filled(G.Problem(G.WGRAD, 128, 128, 32, seed=43, bq=64))
    pr.out["partial"].view()[0, 3] = 0.0                                # one tile's sum of squares missing
    with pytest.raises(AssertionError, match=r"sum-of-squares partials"):
        G.check(pr)


@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", G.HEAD_CASES)
def test_relu_branch_share_of_the_gpu_cases(case, regime, pad):
    """the problems test_gpu_gemm_forms.py runs with seed_w, same seeds: the reference alone puts fewer than 0.1 % of the pre-activations
    within the derived bound of the ReLU kink (K = 512 uniform: sigma ~ 7.5 against a bound of 520 u s ~ 4e-3, expected share ~ 4e-4)"""
    pr = G.head_problem(*case, regime, pad)
    ref = G.reference(pr)
    share = (np.abs(ref["pre"]) <= (pr.red + G.EXTRA_ROUNDINGS) * G.U * ref["s"]).mean()
    assert share <= G.MAX_BRANCH_SHARE, (case, regime, share)
