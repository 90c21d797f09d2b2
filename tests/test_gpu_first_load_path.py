"""The path from a GEMM workgroup's entry to its first operand load (dqn-hfo_amd/csrc/gemm_bodies.hip.h): the record of the
workgroup's problem is taken behind uniform branches on the block index (record 0, record 1, a select between 2 and 3), the tile
comes from a multiply by the reciprocal pack_args() stores instead of a division (tile_decode), and every operand is addressed as
a wave-uniform base plus one 32-bit lane offset.  None of it touches arithmetic on data, so what can go wrong is WHICH tile a
workgroup computes and WHERE its lanes read — these are the smallest shapes that reach every way of getting that wrong:

  * tile counts that are not powers of two: rows 96 and 192 (tiles_q 3, 6 and 12 over the 32- and 16-row tiles; 2 and 3 in the
    64-row wgrad tiles come from the widths), tiles_q = 1 (one row tile);
  * widths 192 and 320 (tiles_p 3 .. 20: off the XCD map) and 128, 256, 512 (tiles_p a multiple of 8 for the 16-, 32- and 64-wide
    tiles: the XCD map, block index >> 3);
  * leading dimensions larger than the width (pad 8 / 24 floats) and operands that start inside a larger allocation (gemm_ref's
    panels sit behind guard rows; the dgrad operands at a column offset of a wider panel);
  * groups of 1, 2, 3 and 4 per grouped form (every branch of the record choice), problems of unequal tile counts;
  * the two-tile kernels (gemm_bwd_seq, gemm_wgrad_tail) with unequal tile counts of their two problems.

Reductions: 512 for the LDS-transpose bodies, 64 and 128 for the direct and narrow ones.  Every output is bit-identical to the
same problem launched alone and within gemm_ref's own float64 bound on NaN-filled, guard-banded buffers; no tolerance of this
test's own.  k_dqda_head_bwd (its narrow tile shares the dgrad bodies' file) is reached through the learner's update on the
smallest tower that takes that plan and compared bit for bit with DQNHIP_TUNE_SEPARATE_ACTOR_HEAD_BWD."""
import pytest

import gemm_forms_lib as F
import gemm_ref as G

pytestmark = pytest.mark.gpu

# (rows, width, pad) of the four problems of a grouped launch, per family of tile shapes.  Row tiles / column tiles:
#   16 x 16 (fwd_lds<1,1>, dgrad_narrow):      6 x 12, 12 x 8, 1 x 20, 6 x 16
#   32 x 32 (fwd_direct<2,2>, fwd_lds<2,2>):   3 x 6, 6 x 8, 1 x 10, 3 x 16
#   32 x 64 (the <4,2> forwards):              3 x 3, 6 x 8 (width 512), 1 x 5, 3 x 4
#   16 x 64 (dgrad_direct, dgrad_lds):         6 x 3, 12 x 8 (width 512), 2 x 5, 6 x 4
SHAPES_16 = [(96, 192, 8), (192, 128, 0), (16, 320, 24), (96, 256, 8)]
SHAPES_32 = [(96, 192, 8), (192, 256, 0), (32, 320, 24), (96, 512, 8)]
SHAPES_64 = [(96, 192, 8), (192, 512, 0), (32, 320, 24), (96, 256, 8)]
# wgrad_narrow, 64 x 16 tiles of dW[outputs][columns]: (outputs, columns, pad) — 6 x 3, 12 x 8, 1 x 5, 6 x 4 tiles
SHAPES_WN = [(96, 192, 8), (192, 512, 0), (16, 320, 24), (96, 256, 8)]

# form -> (mode, shapes, reductions of problems 0 .. 3)
GROUPED = {
    F.FWD_DIRECT_2x2: (G.FWD, SHAPES_32, (64, 128, 64, 128)), F.FWD_DIRECT_4x2: (G.FWD, SHAPES_64, (128, 64, 128, 64)),
    F.FWD_LDS_1x1: (G.FWD, SHAPES_16, (512,) * 4), F.FWD_LDS_2x2: (G.FWD, SHAPES_32, (512,) * 4),
    F.FWD_LDS_4x2: (G.FWD, SHAPES_64, (512,) * 4), F.FWD_LDS_4x2_ONE_IMAGE: (G.FWD, SHAPES_64, (512,) * 4),
    F.DGRAD_DIRECT: (G.DGRAD, SHAPES_64, (64, 128, 64, 128)), F.DGRAD_LDS: (G.DGRAD, SHAPES_64, (512,) * 4),
    F.DGRAD_NARROW: (G.DGRAD, SHAPES_16, (128, 64, 128, 64)),
    F.WGRAD_NARROW: (G.WGRAD, SHAPES_WN, (64, 128, 64, 128)),
}
ORDERS = [(0,), (0, 1), (0, 1, 2), (0, 1, 2, 3), (3, 2, 1, 0)]


def _problem(form, i):
    mode, shapes, reds = GROUPED[form]
    rows, width, pad = shapes[i]
    seed = 21000 + 16 * form + i
    if mode == G.WGRAD:
        return G.Problem(G.WGRAD, width, rows, reds[i], seed=seed, pad=pad, bq=16)
    if mode == G.DGRAD:        # P, mask and C at a column offset inside a wider panel
        return G.Problem(mode, width, rows, reds[i], seed=seed, pad=pad, col0=16 * (i + 1), panel_w=width + 64)
    return G.Problem(mode, width, rows, reds[i], seed=seed, pad=pad)


_alone = {}


def alone(form, i):
    """problem i of `form` launched by itself, checked, its output bits — computed once per form"""
    if (form, i) not in _alone:
        (bits,) = F.run_and_check(form, [_problem(form, i)], f"problem {i} alone")
        _alone[(form, i)] = bits
    return _alone[(form, i)]


@pytest.mark.parametrize("order", ORDERS, ids=lambda o: "p" + "".join(map(str, o)))
@pytest.mark.parametrize("form", list(GROUPED), ids=lambda f: F.FORM_NAME[f])
def test_every_record_and_tile_count(pkg, gpu, form, order):
    problems = [_problem(form, i) for i in order]
    bits = F.run_and_check(form, problems, f"grouped {order}")
    for got, i in zip(bits, order):
        assert F.same_bits(got, alone(form, i)), f"{F.FORM_NAME[form]} grouped {order}: problem {i} differs from its single launch"


# ---- the two-tile kernels: unequal tile counts of their two problems --------------------------------------------------------------
@pytest.mark.parametrize("lds", [False, True], ids=["direct", "lds"])
@pytest.mark.parametrize("rows,cols,outs", [(96, 192, 128), (32, 512, 192), (192, 64, 64)], ids=["18d-6w", "16d-24w", "12d-1w"])
def test_bwd_seq_unequal_tile_counts(pkg, gpu, lds, rows, cols, outs):
    """gemm_bwd_seq: workgroup b computes wgrad tile b (64 x 64 tiles of dW[outs][cols]) and then dgrad tile b (64 x 16 tiles of
    dX[rows][cols]); the grid is the larger count, the workgroups beyond the smaller one skip that tile.  dgrad tiles (rows / 16) x
    (cols / 64), wgrad tiles (outs / 64) x (cols / 64): more dgrad tiles, more wgrad tiles, and one wgrad tile.  Against the dgrad
    form alone and the wgrad slot of the tail launch (record 0 there), bit for bit."""
    red = 512 if lds else 128
    seq, dgrad = (F.BWD_SEQ_LDS, F.DGRAD_LDS) if lds else (F.BWD_SEQ, F.DGRAD_DIRECT)
    mk_d = lambda: G.Problem(G.DGRAD, cols, rows, red, seed=23000 + cols, pad=8)
    mk_w = lambda: G.Problem(G.WGRAD, cols, outs, 32, seed=23100 + cols, pad=8, bq=64)
    (sd, sw) = F.run_and_check(seq, [mk_d(), mk_w()], f"bwd_seq {rows}x{cols}x{outs}")
    (ad,) = F.run_and_check(dgrad, [mk_d()], "dgrad alone")
    assert F.same_bits(sd, ad), "dgrad tiles differ between gemm_bwd_seq and the dgrad launch"
    (tw, _) = F.run_and_check(F.WGRAD_TAIL_1, [mk_w(), G.Problem(G.WGRAD, 64, 16, 32, seed=23200, bq=16)], "wgrad_tail")
    assert F.same_bits(tw, sw), "the tail launch's 64 x 64 wgrad tiles differ from gemm_bwd_seq's"


@pytest.mark.parametrize("form", [F.WGRAD_TAIL_1, F.WGRAD_TAIL_NO], ids=lambda f: F.FORM_NAME[f])
@pytest.mark.parametrize("outs1,cols1,outs0,cols0", [(192, 320, 96, 192), (64, 512, 16, 512), (128, 192, 192, 64)],
                         ids=["15w-18n", "8w-8n", "6w-12n"])
def test_wgrad_tail_unequal_tile_counts(pkg, gpu, form, outs1, cols1, outs0, cols0):
    """gemm_wgrad_tail: the narrow wgrad's 64 x 16 tiles (record 1) come first in the grid, then the 64 x 64 tiles (record 0).
    The narrow slot against gemm_wgrad_narrow alone, the wide slot against the same problem beside another narrow problem."""
    mk1 = lambda: G.Problem(G.WGRAD, cols1, outs1, 64, seed=24000 + cols1, pad=8, bq=64)
    mk0 = lambda: G.Problem(G.WGRAD, cols0, outs0, 128, seed=24100 + cols0, pad=24, bq=16)
    (tw, tn) = F.run_and_check(form, [mk1(), mk0()], "wgrad_tail")
    (an,) = F.run_and_check(F.WGRAD_NARROW, [mk0()], "wgrad_narrow alone")
    assert F.same_bits(tn, an), "the tail launch's narrow wgrad tiles differ from gemm_wgrad_narrow's"
    (ow, _) = F.run_and_check(form, [mk1(), G.Problem(G.WGRAD, 64, 16, 32, seed=24200, bq=16)], "wgrad_tail, other narrow problem")
    assert F.same_bits(tw, ow), "the tail launch's 64 x 64 wgrad tiles depend on the narrow problem beside them"


# ---- k_dqda_head_bwd through the learner ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,hidden,S", [(64, (256, 128, 64, 64), 59), (32, (1024, 512, 256, 128), 59)])
def test_dqda_head_bwd_equals_separate_launches(pkg, gpu, B, hidden, S):
    """k_dqda_head_bwd at tower tops of 64 and 128 units (four and two row tiles, one column chunk: the smallest towers of
    test_gpu_tuning_flags.py that take the plan) against the narrow dgrad launch + k_head_bwd<10>: every result bit-identical"""
    a = F.run32(pkg, 0, B, hidden, S, want={"dqda_head_bwd"})
    b = F.run32(pkg, pkg.capi.TUNE_SEPARATE_ACTOR_HEAD_BWD, B, hidden, S, unwanted={"dqda_head_bwd"})
    F.assert_same_run(a, b)
