"""Every GEMM form learner.hip launches for the fp32 tower, one launch each through the product's own launchers
(dqnhip_test_gemm_form, tests/csrc/gemm_forms.hip), judged per element against a float64 reference (tests/gemm_ref.py).

What each case checks, in this order: every output element is finite (outputs arrive as one NaN bit pattern, so an unwritten
element shows); guard rows, pad columns and the rest of a wider panel still hold that pattern bit for bit (the kernel stayed
inside its tiles and indexed with the leading dimensions); |got - ref| <= (red + 8) u s_ij for EVERY element; the kernel's
max |got - ref| / (u s_ij) is at most 4 x that of the plain float32 numpy product; a second run is bit-identical (fixed
reduction order); forward forms: a problem inside a grouped launch comes out bit-identical to its single launch.

Shapes are the smallest at which a form can still go wrong: two or more tiles in each output direction; per body, reductions
that take only the tail steps, the primed ring without a loop trip, one trip, and two trips of the steady-state ring loop plus
tail steps (the in-loop refill carries the chain at the product's sizes; the trip counts are worked out beside each case list);
dense operands, and every leading dimension 64 larger
than its width; uniform data, and the same data with rows scaled by 2**-6 .. 2**6 so that the bound bites on small rows.

max r = |y - ref| / (u s_ij) measured on the MI355X, worst case over the cases of a form (each assertion message and, under
`pytest -s`, a MAXR line per problem carry both figures):

    form                       yardstick max r   kernel max r   worst kernel / yardstick of one problem
    fwd_direct<2,2>                 3.46             1.22            0.53
    fwd_direct<4,2>                 3.23             1.40            0.56
    fwd_lds<1,1,true>               2.22             1.32            0.81
    fwd_lds<2,2,true>               2.37             1.14            0.81
    fwd_lds<4,2,true>               1.74             1.08            0.76
    fwd_lds<4,2,true,1>             2.27             1.09            0.68
    dgrad_direct<1,1>               3.85             1.38            0.47
    dgrad_lds<1,1>                  2.50             1.43            0.87
    dgrad_narrow                    2.65             1.24            0.56
    wgrad_narrow<1>                 4.01             1.36            0.51
    bwd_seq<false>                  3.42             1.58            0.59
    bwd_seq<true>                   3.58             1.69            0.57
    bwd_pair_direct<1,false>        3.75             1.47            0.49
    bwd_pair_direct<1,true>         4.61             1.48            0.60
    wgrad_tail<1>                   3.51             1.47            0.47
    wgrad_tail<kNO>                 4.02             1.42            0.57

(Taken before the 512-column cases that switch on the XCD-interleaved tile map were added; those pass the same assertions.)
The kernels' four short chains per element come out closer to the float64 value than the BLAS product on every problem, so
the factor of 4 (gemm_ref.TIGHT_FACTOR) has a margin of about five; the derived bound allows r up to red + 8 (72 .. 776).
"""
import ctypes as C

import numpy as np
import pytest

import gemm_ref as G
import testlib

pytestmark = pytest.mark.gpu

(FWD_DIRECT_2x2, FWD_DIRECT_4x2, FWD_LDS_1x1, FWD_LDS_2x2, FWD_LDS_4x2, FWD_LDS_4x2_ONE_IMAGE, DGRAD_DIRECT, DGRAD_LDS, DGRAD_NARROW,
 WGRAD_NARROW, BWD_SEQ, BWD_SEQ_LDS, BWD_PAIR, BWD_PAIR_LDS, WGRAD_TAIL_1, WGRAD_TAIL_NO) = range(16)
FORM_NAME = ["fwd_direct<2,2>", "fwd_direct<4,2>", "fwd_lds<1,1,true>", "fwd_lds<2,2,true>", "fwd_lds<4,2,true>", "fwd_lds<4,2,true,1>",
             "dgrad_direct<1,1>", "dgrad_lds<1,1>", "dgrad_narrow", "wgrad_narrow<1>", "bwd_seq<false>", "bwd_seq<true>",
             "bwd_pair_direct<1,false>", "bwd_pair_direct<1,true>", "wgrad_tail<1>", "wgrad_tail<kNO>"]
# output tile (columns p x rows q) of the forward forms
FWD_TILE = {FWD_DIRECT_2x2: (32, 32), FWD_DIRECT_4x2: (64, 32), FWD_LDS_1x1: (16, 16), FWD_LDS_2x2: (32, 32), FWD_LDS_4x2: (64, 32),
            FWD_LDS_4x2_ONE_IMAGE: (64, 32)}
PADS = [0, 64]                      # dense; every leading dimension 64 floats (256 bytes: 16-byte alignment kept) larger than the width
REGIMES = ["uniform", "scaled"]


class Buf(C.Structure):
    _fields_ = [("host", C.c_void_p), ("count", C.c_int64), ("offset", C.c_int64)]


class Prob(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("mode", "Pdim", "Qdim", "Kred", "ldp", "ldq", "ldc", "ldm", "relu", "xcopy_col", "xcopy_n", "reserved")] + \
               [(n, Buf) for n in ("P", "Q", "bias", "mask", "seed_w", "dot_w", "C", "db", "partial", "C2", "dot_out", "xcopy_dst")]


def _entry():
    fn = testlib.load_test().dqnhip_test_gemm_form
    fn.restype = C.c_int
    fn.argtypes = [C.c_int32, C.c_int32, C.POINTER(Prob)]
    return fn


def _c_problem(pr):
    c = Prob(mode=pr.mode, Pdim=pr.Pdim, Qdim=pr.Qdim, Kred=pr.Kred, ldp=pr.ldp, ldq=pr.ldq, ldc=pr.ldc, ldm=pr.ldm, relu=pr.relu,
             xcopy_col=pr.xcopy_col, xcopy_n=pr.xcopy_n)
    for name, panel in list(pr.inp.items()) + list(pr.out.items()):
        setattr(c, name, Buf(panel.buf.ctypes.data, panel.buf.size, panel.offset))
    return c


def launch(form, problems):
    """one launch of `form` on freshly sentinel-filled outputs; returns the bit image of every output buffer, per problem"""
    for pr in problems:
        pr.reset_outputs()
    arr = (Prob * len(problems))(*[_c_problem(pr) for pr in problems])
    rc = _entry()(form, len(problems), arr)
    assert rc == 0, (FORM_NAME[form], rc)
    return [pr.snapshot() for pr in problems]


def same_bits(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def run_and_check(form, problems, tag):
    """launch twice (bit-identical), then the comparator on every problem; prints the yardstick and kernel max r"""
    first = launch(form, problems)
    again = launch(form, problems)
    for i, (a, b) in enumerate(zip(first, again)):
        assert same_bits(a, b), f"{FORM_NAME[form]} {tag} problem {i}: two runs differ (the kernels document a fixed reduction order)"
    stats = []
    for i, pr in enumerate(problems):
        st = G.check(pr, f"{FORM_NAME[form]} {tag} problem {i}")
        print(f"MAXR {FORM_NAME[form]} {tag} problem {i}: yardstick {st['yard_r']:.3f} kernel {st['kernel_r']:.3f} "
              + " ".join(f"{k} {v:.3g}" for k, v in st.items() if k not in ("yard_r", "kernel_r")))
        stats.append(st)
    return again, stats


# ---- forward ---------------------------------------------------------------------------------------------------------------------
# (rows, outputs, K).  lds forms (T = K / 128 steps of 32 k per wave, loop `t + 4 < T; t += 2`): K = 512 (prologue + drain only),
# 768 (one loop trip), 1024 (two).  direct forms (nkb = K / 64 blocks of 16 k per wave, ring of 4, loop `kb + 4 < (nkb & ~3)`):
# K = 64 (one tail step only), 128 (two tail steps), 320 (the primed ring, no loop trip, one tail step), 576 (one loop trip + one
# tail step), 832 (two trips + one tail step); 576 and 832 are no multiples of 256, i.e. what the learner sends to the direct forms.
# Rows 48 where the tile takes multiples of 16 only; 512 outputs: a multiple of eight tiles in p for every tile width, which is
# what switches tile_of_problem to the XCD-interleaved tile map (every 1024-wide layer of the product takes it).
FWD_LDS_SHAPES = [(32, 128, 512), (96, 192, 768), (48, 64, 768), (96, 64, 512), (32, 512, 512), (32, 64, 1024)]
FWD_DIRECT_SHAPES = [(32, 128, 64), (96, 192, 320), (96, 64, 128), (64, 512, 64), (32, 64, 576), (64, 128, 832)]


def fwd_cases():
    for form, (bp, bq) in FWD_TILE.items():
        lds = form >= FWD_LDS_1x1
        for (rows, outs, k) in (FWD_LDS_SHAPES if lds else FWD_DIRECT_SHAPES):
            if outs % bp or rows % bq:
                continue
            yield pytest.param(form, rows, outs, k, id=f"{FORM_NAME[form]}-{rows}x{outs}x{k}")


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("form,rows,outs,k", list(fwd_cases()))
def test_forward_forms(pkg, gpu, form, rows, outs, k, regime, pad):
    """n = 1 and n = 2 (layer_forward with two passes): different data per problem; each problem of the grouped launch must equal
    its own single-problem result bit for bit"""
    tag = f"{rows}x{outs}x{k} {regime} pad {pad}"
    a = G.Problem(G.FWD, outs, rows, k, seed=1000 + form, regime=regime, pad=pad)
    b = G.Problem(G.FWD, outs, rows, k, seed=2000 + form, regime=regime, pad=pad)
    (sa,), _ = run_and_check(form, [a], tag + " single")
    (sb,), _ = run_and_check(form, [b], tag + " single(second data)")
    (ga, gb), _ = run_and_check(form, [a, b], tag + " grouped")
    assert same_bits(ga, sa), f"{FORM_NAME[form]} {tag}: problem 0 of the grouped launch differs from its single launch"
    assert same_bits(gb, sb), f"{FORM_NAME[form]} {tag}: problem 1 of the grouped launch differs from its single launch"


# the top tower layer's epilogue extras (layer_forward: seed_w / C2 of the critic(s, mu(s)) pass, dot_w / dot_out of Step(1)'s critic
# passes), on every forward form that layer can take.  Seeds fixed: tests/test_gemm_ref_host.py confirms on the CPU that fewer
# than 0.1 % of the pre-activations lie within the bound of the ReLU kink for exactly these problems.
HEAD_CASES = G.HEAD_CASES          # (form, rows, outputs, K), one per forward form
head_problem = G.head_problem


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("form,rows,outs,k", [pytest.param(*c, id=f"{FORM_NAME[c[0]]}-{c[1]}x{c[2]}x{c[3]}") for c in HEAD_CASES])
def test_forward_head_epilogues(pkg, gpu, form, rows, outs, k, regime, pad):
    """C2 = (-seed_w) * lrelu'(C) (exact; either branch within the bound of the kink) and dot_out = 16-column pieces of C . dot_w"""
    run_and_check(form, [head_problem(form, rows, outs, k, regime, pad)], f"{rows}x{outs}x{k} {regime} pad {pad} seed+dot")


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("regime", REGIMES)
def test_first_layers_xcopy(pkg, gpu, regime, pad):
    """first_layers_launch: a grouped fwd_direct<4,2> of four problems of different shapes whose third has no bias, no ReLU, K = the
    state columns of a wider panel row and leaves columns [xcopy_col, +xcopy_n) of its weights transposed — bit-exact; three row
    tiles share the columns"""
    rows = 96
    a = G.Problem(G.FWD, 128, rows, 64, seed=4001, regime=regime, pad=pad)
    b = G.Problem(G.FWD, 64, rows, 128, seed=4002, regime=regime, pad=pad)
    x = G.Problem(G.FWD, 128, rows, 64, seed=4003, regime=regime, pad=pad, bias=False, relu=0, xcopy=(58, 10), p_width=128)
    d = G.Problem(G.FWD, 192, rows, 64, seed=4004, regime=regime, pad=pad)
    run_and_check(FWD_DIRECT_4x2, [a, b, x, d], f"{rows} rows {regime} pad {pad} first layers")


# ---- dgrad -------------------------------------------------------------------------------------------------------------------------
# (rows, columns = Pdim, reduction = the layer's outputs); the reductions as for the forward forms: direct 576 / 832 and lds 768 / 1024
# run one / two trips of the ring loop
DGRAD_CASES = [(DGRAD_DIRECT, 32, 128, 64), (DGRAD_DIRECT, 48, 192, 320), (DGRAD_DIRECT, 96, 64, 128), (DGRAD_DIRECT, 32, 512, 128),
               (DGRAD_DIRECT, 32, 64, 576), (DGRAD_DIRECT, 48, 128, 832),
               (DGRAD_LDS, 32, 128, 512), (DGRAD_LDS, 48, 192, 768), (DGRAD_LDS, 96, 64, 512), (DGRAD_LDS, 32, 512, 768), (DGRAD_LDS, 32, 64, 1024)]


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("form,rows,cols,red", [pytest.param(*c, id=f"{FORM_NAME[c[0]]}-{c[1]}x{c[2]}x{c[3]}") for c in DGRAD_CASES])
def test_dgrad_forms(pkg, gpu, form, rows, cols, red, regime, pad):
    tag = f"{rows}x{cols}x{red} {regime} pad {pad}"
    run_and_check(form, [G.Problem(G.DGRAD, cols, rows, red, seed=5000 + form, regime=regime, pad=pad)], tag)
    # the first layer's input gradient has no ReLU' mask (tower_backward: mask = i > 0 ? act[i] : nullptr)
    run_and_check(form, [G.Problem(G.DGRAD, cols, rows, red, seed=5100 + form, regime=regime, pad=pad, mask=False)], tag + " no mask")


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("pdim,panel_w,col0", [(16, 64, 16), (32, 128, 16), (32, 32, 0)])
@pytest.mark.parametrize("rows,red", [(32, 64), (96, 128), (48, 320), (96, 512), (32, 832)])   # ring of 4 blocks of 16 k: 512 one loop trip, 832 two + a tail step
def test_dgrad_narrow(pkg, gpu, rows, red, pdim, panel_w, col0, regime, pad):
    """the product's addressing (tower_backward): P, C and the mask offset by c0 = 16 columns inside the first layer's panel, Pdim = 16 / 32
    of its 64 / 128 columns; the other columns of C must stay untouched, those of P and the mask hold NaN.  Without a mask first: the
    learner launches this form for layer 0 only, whose input has no ReLU (tower_backward: mask = i > 0 ? act[i] : nullptr)"""
    tag = f"{rows}x{pdim}@{col0}/{panel_w}x{red} {regime} pad {pad}"
    pr = G.Problem(G.DGRAD, pdim, rows, red, seed=6100 + pdim, regime=regime, pad=pad, col0=col0, panel_w=panel_w, mask=False)
    run_and_check(DGRAD_NARROW, [pr], tag + " no mask")
    pr = G.Problem(G.DGRAD, pdim, rows, red, seed=6000 + pdim, regime=regime, pad=pad, col0=col0, panel_w=panel_w)
    run_and_check(DGRAD_NARROW, [pr], tag)


# ---- wgrad -------------------------------------------------------------------------------------------------------------------------
# (rows = the reduction, outputs = Qdim, columns = Pdim).  Both wgrad bodies step four rows per wave (nst = rows / 16 steps, ring of 4,
# loop `st + 4 < nst - nst % 4`): rows 32 and 48 take tail steps only, 96 the primed ring and two tail steps, 160 one loop trip and
# two tail steps, 208 two trips and one tail step.
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("rows,outs,cols", [(32, 64, 128), (48, 192, 64), (96, 128, 192), (96, 48, 512), (160, 64, 64), (208, 128, 128)])
def test_wgrad_narrow(pkg, gpu, rows, outs, cols, regime, pad):
    run_and_check(WGRAD_NARROW, [G.Problem(G.WGRAD, cols, outs, rows, seed=7000 + rows, regime=regime, pad=pad, bq=16)],
                  f"{rows}x{outs}x{cols} {regime} pad {pad}")


# ---- one layer's backward in one launch: prob[0] dgrad (64 x 16 tiles), prob[1] wgrad (64 x 64 tiles) ---------------------------------
# ((rows, columns, reduction) of the dgrad, (rows, outputs, columns) of the wgrad): different tile counts, so that
# grid = max(nd, nw) has idle blocks on either side — once nd > nw, once nw > nd
def bwd_cases(direct, lds):
    for form, is_lds in ((direct, False), (lds, True)):
        short, long_ = (512, 768) if is_lds else (64, 320)
        yield pytest.param(form, (96, 192, long_), (96, 128, 64), id=f"{FORM_NAME[form]}-nd18-nw2")
        yield pytest.param(form, (32, 64, short), (48, 192, 192), id=f"{FORM_NAME[form]}-nd2-nw9")
        # the layer as the learner couples it: dgrad (rows, kp, N) with wgrad (rows, N, kp)
        n = 512 if is_lds else 128
        yield pytest.param(form, (32, 128, n), (32, n, 128), id=f"{FORM_NAME[form]}-layer")
        # eight tiles in p on both sides: the XCD-interleaved tile map
        yield pytest.param(form, (32, 512, n), (32, n, 512), id=f"{FORM_NAME[form]}-layer-xcd")
        # both ring loops turning (see the forward and wgrad case lists): one trip each, then two trips each, coupled as a layer
        n1, n2 = (768, 1024) if is_lds else (576, 832)
        yield pytest.param(form, (160, 128, n1), (160, n1, 128), id=f"{FORM_NAME[form]}-layer-one-trip")
        yield pytest.param(form, (208, 64, n2), (208, n2, 64), id=f"{FORM_NAME[form]}-layer-two-trips")


def _bwd(form, d, w, regime, pad):
    pd = G.Problem(G.DGRAD, d[1], d[0], d[2], seed=8000 + form, regime=regime, pad=pad)
    pw = G.Problem(G.WGRAD, w[2], w[1], w[0], seed=8100 + form, regime=regime, pad=pad, bq=64)
    run_and_check(form, [pd, pw], f"dgrad {d} wgrad {w} {regime} pad {pad}")


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("form,d,w", list(bwd_cases(BWD_SEQ, BWD_SEQ_LDS)))
def test_bwd_seq(pkg, gpu, form, d, w, regime, pad):
    _bwd(form, d, w, regime, pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("form,d,w", list(bwd_cases(BWD_PAIR, BWD_PAIR_LDS)))
def test_bwd_pair(pkg, gpu, form, d, w, regime, pad):
    _bwd(form, d, w, regime, pad)


# ---- the shifted schedule's last launch: prob[0] wgrad on 64 x 64 tiles, prob[1] on 64 x 16 tiles, no riders ---------------------------
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("regime", REGIMES)
# (512 columns: the XCD-interleaved tile map; 160 / 208 rows: one / two trips of both bodies' ring loops)
@pytest.mark.parametrize("rows,cols1,cols0", [(32, 128, 64), (96, 192, 128), (32, 512, 512), (160, 128, 64), (208, 64, 128)])
@pytest.mark.parametrize("form", [WGRAD_TAIL_1, WGRAD_TAIL_NO], ids=lambda f: FORM_NAME[f])
def test_wgrad_tail(pkg, gpu, form, rows, cols1, cols0, regime, pad):
    w1 = G.Problem(G.WGRAD, cols1, 192, rows, seed=9000 + form, regime=regime, pad=pad, bq=64)
    w0 = G.Problem(G.WGRAD, cols0, 64, rows, seed=9100 + form, regime=regime, pad=pad, bq=16)
    run_and_check(form, [w1, w0], f"{rows} rows {cols1}/{cols0} columns {regime} pad {pad}")


# ---- shape validation: an invalid shape never reaches the GPU ----------------------------------------------------------------------------
def test_invalid_shapes_are_refused(pkg, gpu):
    """return code 1 before anything is uploaded or launched: the outputs are still all sentinel"""
    def refused(form, problems):
        for pr in problems:
            pr.reset_outputs()
        arr = (Prob * len(problems))(*[_c_problem(pr) for pr in problems])
        rc = _entry()(form, len(problems), arr)
        untouched = all((pr.out[k].buf.view(np.uint32) == G.SENTINEL_BITS).all() for pr in problems for k in pr.out)
        return rc == 1 and untouched

    fwd = lambda outs, rows, k, **kw: G.Problem(G.FWD, outs, rows, k, seed=1, **kw)
    assert refused(FWD_LDS_2x2, [fwd(64, 32, 256)])                     # the LDS-transpose bodies need K >= 512
    assert refused(FWD_LDS_2x2, [fwd(64, 32, 640)])                     # ... and K % 256 == 0
    assert refused(FWD_LDS_2x2, [fwd(64, 48, 512)])                     # 32-row tiles
    assert refused(FWD_DIRECT_4x2, [fwd(96, 32, 64)])                   # 64-column tiles
    assert refused(FWD_DIRECT_2x2, [fwd(64, 32, 96)])                   # K % 64 == 0
    assert refused(FWD_LDS_4x2, [fwd(64, 32, 512, xcopy=(0, 4))])       # no transposed copy in the lds body
    assert refused(DGRAD_DIRECT, [fwd(64, 32, 64)])                     # a forward problem for a dgrad form
    assert refused(WGRAD_NARROW, [G.Problem(G.WGRAD, 64, 64, 24, seed=1, bq=16)])   # the reduction advances four rows per wave and step
    assert refused(BWD_SEQ, [G.Problem(G.DGRAD, 64, 32, 64, seed=1)])   # two problems: dgrad, wgrad
    assert refused(BWD_SEQ_LDS, [G.Problem(G.DGRAD, 64, 32, 128, seed=1), G.Problem(G.WGRAD, 64, 64, 32, seed=1, bq=64)])
    assert refused(16, [fwd(64, 32, 64)])                               # no such form
    # a leading dimension smaller than the width, an operand that does not fit its buffer
    pr = fwd(64, 32, 64)
    pr.ldc = 32
    assert refused(FWD_DIRECT_2x2, [pr])
    pr = fwd(64, 32, 64)
    pr.Qdim = 64
    assert refused(FWD_DIRECT_2x2, [pr])
    pr = fwd(64, 32, 64)
    pr.inp["P"].offset += 2                                             # 16-byte alignment of the float4 loads
    assert refused(FWD_DIRECT_2x2, [pr])
