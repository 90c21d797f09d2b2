"""The tile bookkeeping of the packed GEMM launch arguments (GemmArgs, dqn-hfo_amd/csrc/gemm_common.hip.h): a launcher packs its
GemmBatch into a 64-byte header (tile_base / tiles_p / tiles_q of up to four problems), one hot record per problem and the
cold epilogue fields; the workgroup finds its problem and tile from the header alone and picks the operand pointers with
scalar selects.  What can go wrong is which tile of which problem a workgroup takes, not the arithmetic, so these cases are the
smallest that reach every branch of that search: launches of 1, 2, 3 and 4 problems whose tile counts all differ, with
problems on either side of the `tiles_p % 8 == 0` switch of the tile map in one launch and a problem whose first tile is
workgroup 256 of the grid (one workgroup per CU before it).  Every output must be bit-identical to the same problem launched
alone and pass the float64 comparator of tests/gemm_ref.py on NaN-filled, guard-banded buffers (a tile written twice with other
data, not at all, or into a neighbour's problem shows).  The kernels that carry their problems as a compile-time fact
(gemm_bwd_seq, gemm_wgrad_tail) are compared with the forms that compute the same tiles through the grouped search; the
kernels only the learner reaches (the wgrad tail with its head rider against gemm_wgrad_narrow_rider, gemm_dgrad_narrow_qrider
against k_dqda_head_bwd, k_dgrad_qtrain, the two actors' heads in one launch) through the schedules its tuning flags and update
phases already select, on the smallest towers that take those schedules (asserted on the learner's update plan).

Rows are 32 and 64, widths 64 .. 512; reductions 512 for the LDS-transpose bodies, 64 and 128 for the direct and narrow ones.
The bounds are gemm_ref's ((red + 8) u s per element, kernel max r <= 4 x the float32 yardstick's)."""
import numpy as np
import pytest

import gemm_forms_lib as F
import gemm_ref as G

pytestmark = pytest.mark.gpu

# (rows, width) of the four problems of a grouped launch.  Tiles in p, by tile width 16 / 32 / 64: 16, 4, 32, 8 / 8, 2, 16, 4 /
# 4, 1, 8, 2 — for every tile width problems with tiles_p % 8 == 0 and != 0 share a launch, and every prefix has distinct counts.
SHAPES = [(32, 256), (64, 64), (32, 512), (64, 128)]
ORDERS = [(0,), (0, 1), (0, 1, 2), (0, 1, 2, 3), (3, 2, 1, 0), (2, 1, 3)]

# form -> (mode, reductions of problems 0 .. 3)
GROUPED = {
    F.FWD_DIRECT_2x2: (G.FWD, (64, 128, 64, 128)), F.FWD_DIRECT_4x2: (G.FWD, (128, 64, 128, 64)),
    F.FWD_LDS_1x1: (G.FWD, (512,) * 4), F.FWD_LDS_2x2: (G.FWD, (512,) * 4), F.FWD_LDS_4x2: (G.FWD, (512,) * 4),
    F.FWD_LDS_4x2_ONE_IMAGE: (G.FWD, (512,) * 4),
    F.DGRAD_DIRECT: (G.DGRAD, (64, 128, 64, 128)), F.DGRAD_LDS: (G.DGRAD, (512,) * 4), F.DGRAD_NARROW: (G.DGRAD, (128, 64, 128, 64)),
    F.WGRAD_NARROW: (G.WGRAD, (64, 128, 64, 128)),
}


def _problem(form, i, regime="uniform", pad=0):
    mode, reds = GROUPED[form]
    rows, width = SHAPES[i]
    seed = 11000 + 16 * form + i
    if mode == G.WGRAD:        # 64 x 16 tiles of dW[outputs][columns]: `rows` outputs, `width` columns, the reduction over reds[i] samples
        return G.Problem(G.WGRAD, width, rows, reds[i], seed=seed, regime=regime, pad=pad, bq=16)
    return G.Problem(mode, width, rows, reds[i], seed=seed, regime=regime, pad=pad)


_alone = {}


def alone(form, i):
    """problem i of `form` launched by itself, checked, its output bits — computed once per form"""
    if (form, i) not in _alone:
        pr = _problem(form, i)
        (bits,) = F.run_and_check(form, [pr], f"problem {i} alone")
        _alone[(form, i)] = bits
    return _alone[(form, i)]


@pytest.mark.parametrize("order", ORDERS, ids=lambda o: "p" + "".join(map(str, o)))
@pytest.mark.parametrize("form", list(GROUPED), ids=lambda f: F.FORM_NAME[f])
def test_grouped_launch_finds_every_tile(pkg, gpu, form, order):
    problems = [_problem(form, i) for i in order]
    bits = F.run_and_check(form, problems, f"grouped {order}")
    for got, i in zip(bits, order):
        assert F.same_bits(got, alone(form, i)), f"{F.FORM_NAME[form]} grouped {order}: problem {i} differs from its single launch"


@pytest.mark.parametrize("form,first", [(F.FWD_LDS_1x1, (64, 512)), (F.DGRAD_NARROW, (64, 512))], ids=lambda v: F.FORM_NAME[v] if isinstance(v, int) else "")
def test_problem_starting_at_workgroup_256(pkg, gpu, form, first):
    """16 x 16 tiles: two 64 x 512 problems are 128 workgroups each, so the third problem's tile_base is exactly 256 — the first
    workgroup after one per CU — and the fourth follows a problem of 8 tiles"""
    mode, reds = GROUPED[form]
    mk = lambda rows, width, seed: G.Problem(mode, width, rows, reds[0], seed=seed)
    problems = [mk(*first, 12000 + form), mk(*first, 12100 + form), mk(32, 64, 12200 + form), mk(32, 256, 12300 + form)]
    bits = F.run_and_check(form, problems, "tile_base 0 / 128 / 256 / 264")
    for i, pr in enumerate(problems):
        (single,) = F.run_and_check(form, [pr], f"problem {i} alone")
        assert F.same_bits(bits[i], single), f"{F.FORM_NAME[form]}: problem {i} (tile_base {[0, 128, 256, 264][i]}) differs from its single launch"


# ---- the kernels whose problems are a compile-time fact ---------------------------------------------------------------------------
@pytest.mark.parametrize("lds", [False, True], ids=["direct", "lds"])
@pytest.mark.parametrize("cols", [64, 512], ids=["1-tile-in-p", "8-tiles-in-p"])
def test_bwd_seq_tiles_equal_the_grouped_forms(pkg, gpu, lds, cols):
    """gemm_bwd_seq (workgroup b: wgrad tile b, then dgrad tile b; both problems count their tiles from 0) at its smallest legal
    shapes, 32 rows: the dgrad output against the dgrad form alone, the wgrad outputs against the same problem in the pair launch
    (two workgroup types, found through the grouped search) and in the tail launch's 64 x 64 slot — the same bodies on the same
    data, bit for bit"""
    red = 512 if lds else 64
    seq, pair, dgrad = (F.BWD_SEQ_LDS, F.BWD_PAIR_LDS, F.DGRAD_LDS) if lds else (F.BWD_SEQ, F.BWD_PAIR, F.DGRAD_DIRECT)
    mk_d = lambda: G.Problem(G.DGRAD, cols, 32, red, seed=13000 + cols)
    mk_w = lambda: G.Problem(G.WGRAD, cols, 64, 32, seed=13100 + cols, bq=64)
    (sd, sw) = F.run_and_check(seq, [mk_d(), mk_w()], f"bwd_seq {cols}")
    (pd, pw) = F.run_and_check(pair, [mk_d(), mk_w()], f"bwd_pair {cols}")
    (ad,) = F.run_and_check(dgrad, [mk_d()], f"dgrad alone {cols}")
    assert F.same_bits(sd, ad) and F.same_bits(pd, ad), "dgrad tiles differ between gemm_bwd_seq, the pair launch and the dgrad launch"
    assert F.same_bits(sw, pw), "wgrad tiles differ between gemm_bwd_seq and the pair launch"
    (tw, tn) = F.run_and_check(F.WGRAD_TAIL_1, [mk_w(), G.Problem(G.WGRAD, 64, 32, 32, seed=13200, bq=16)], f"wgrad_tail {cols}")
    assert F.same_bits(tw, sw), "the tail launch's 64 x 64 wgrad tiles differ from gemm_bwd_seq's"


@pytest.mark.parametrize("form", [F.WGRAD_TAIL_1, F.WGRAD_TAIL_NO], ids=lambda f: F.FORM_NAME[f])
@pytest.mark.parametrize("cols0", [64, 512], ids=["1-tile-in-p", "8-tiles-in-p"])
def test_wgrad_tail_narrow_tiles_equal_the_narrow_form(pkg, gpu, form, cols0):
    """gemm_wgrad_tail without riders: its 64 x 16 slot (first in the grid) against gemm_wgrad_narrow alone, bit for bit"""
    w1 = G.Problem(G.WGRAD, 128, 64, 32, seed=14000 + form, bq=64)
    mk0 = lambda: G.Problem(G.WGRAD, cols0, 32, 32, seed=14100 + cols0, bq=16)
    (_, tn) = F.run_and_check(form, [w1, mk0()], f"wgrad_tail narrow {cols0}")
    (an,) = F.run_and_check(F.WGRAD_NARROW, [mk0()], f"wgrad_narrow alone {cols0}")
    assert F.same_bits(tn, an), "the tail launch's narrow wgrad tiles differ from gemm_wgrad_narrow's"


# ---- the kernels only the learner launches ----------------------------------------------------------------------------------------
# The smallest towers whose plan takes the shifted backward (no layer above the first fits the side-by-side pair launch:
# kp / 64 * (rows / 16 + outputs / 64) > 256) and with it k_dgrad_qtrain, gemm_wgrad_tail with the head rider, and — on the other
# side of each flag — gemm_wgrad_narrow_rider and gemm_dgrad_narrow_qrider.  At 32 rows: 1024 x 1024 (16 (2 + 16) = 288), and,
# for k_dgrad_qtrain's smallest tower top, 2048 -> 512 (32 (2 + 8) = 320: H = 512 with 32 rows).
LEARNER_SHAPES = [(32, (1024, 1024), 58), (32, (2048, 512), 59)]
SHIFTED = {"bwd_shifted_critic", "bwd_shifted_actor", "head_wgrad_rides_critic", "head_wgrad_rides_actor"}


@pytest.mark.parametrize("B,hidden,S", LEARNER_SHAPES)
def test_learner_shifted_backward_and_head_rider(pkg, gpu, B, hidden, S):
    """gemm_bwd_seq + gemm_wgrad_tail<NH> with the head's dW / db rider against the per-layer schedule, whose last launch is
    gemm_wgrad_narrow_rider<NH>: the same workgroups doing the same arithmetic in other launches, every result bit-identical
    (both sides with k_head_q_train in a launch of its own)"""
    sep = pkg.capi.TUNE_SEPARATE_Q_TRAIN
    a = F.run32(pkg, sep, B, hidden, S, want=SHIFTED, unwanted={"q_train_in_dgrad"})
    b = F.run32(pkg, sep | pkg.capi.TUNE_BWD_UNSHIFTED, B, hidden, S, want={"head_wgrad_rides_critic", "head_wgrad_rides_actor"},
                unwanted={"bwd_shifted_critic", "bwd_shifted_actor"})
    F.assert_same_run(a, b)


@pytest.mark.parametrize("B,hidden,S", LEARNER_SHAPES)
def test_learner_dqda_head_bwd_and_narrow_qrider(pkg, gpu, B, hidden, S):
    """k_dqda_head_bwd (its embedded narrow-dgrad problem) against gemm_dgrad_narrow_qrider + the heads' backward: bit-identical,
    eager and graph-replayed"""
    a = F.run32(pkg, 0, B, hidden, S, want={"dqda_head_bwd"})
    b = F.run32(pkg, pkg.capi.TUNE_SEPARATE_ACTOR_HEAD_BWD, B, hidden, S, unwanted={"dqda_head_bwd"})
    F.assert_same_run(a, b)
    g = F.run32(pkg, 0, B, hidden, S, use_graph=True, want={"dqda_head_bwd"})
    assert a[0] == g[0]
    for x, y in zip(a[2], g[2]):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("B,hidden,S", LEARNER_SHAPES)
def test_learner_dgrad_qtrain(pkg, gpu, B, hidden, S):
    """k_dgrad_qtrain against the dgrad launch + k_head_q_train.  The head dot product is summed in another fixed order and dq_r is
    applied after the reduction instead of before: fp32 round-off.  Bounds as test_gpu_tuning_flags.py sets them for this pair of
    schedules: per-row outputs within 4e-6 of the largest magnitude, the loss within 1e-5, the critic's gradient within 2e-5 of
    its norm; parameters within the three Adam steps taken (each of magnitude lr whatever |g| is)."""
    out = {}
    for tuning in (0, pkg.capi.TUNE_SEPARATE_Q_TRAIN):
        d = F.learner(pkg, tuning, B, hidden, S)
        forms = set(d.update_plan()["forms"])
        assert SHIFTED <= forms and ("q_train_in_dgrad" in forms) == (tuning == 0), (tuning, sorted(forms))
        rng = np.random.default_rng(7)
        rec = []
        for u in range(3):
            idx = rng.integers(0, 2000, B).astype(np.int32)
            d.update_phase(0, idx)
            first = {k: d.debug_read(k) for k in ("q_target", "q_train", "y")}
            first["gc"] = d.get_params(1, pkg.KIND_G)
            d.update_phase(1); d.update_phase(2)
            first["stats"] = d.read_stats()
            rec.append(first)
        out[tuning] = (rec, [d.get_params(n).astype(np.float64) for n in range(4)])
        d.close()
    (ra, wa), (rb, wb) = out[0], out[pkg.capi.TUNE_SEPARATE_Q_TRAIN]
    for k in ("q_target", "q_train", "y"):                           # first update: same weights
        scale = max(1.0, float(np.abs(rb[0][k]).max()))
        np.testing.assert_allclose(ra[0][k], rb[0][k], rtol=0, atol=4e-6 * scale)
    assert abs(ra[0]["stats"][0] - rb[0]["stats"][0]) <= 1e-5 * max(1.0, abs(rb[0]["stats"][0]))
    rel = np.linalg.norm(ra[0]["gc"].astype(np.float64) - rb[0]["gc"]) / np.linalg.norm(rb[0]["gc"])
    assert rel <= 2e-5, rel
    for a, b in zip(ra, rb):
        assert np.allclose(a["stats"], b["stats"], rtol=1e-4, atol=1e-6), (a["stats"], b["stats"])
    lr = {0: 1e-5, 1: 1e-3, 2: 1e-5 * 1e-3, 3: 1e-3 * 1e-3}
    for net, (x, y) in enumerate(zip(wa, wb)):
        dd = np.abs(x - y)
        assert dd.max() <= 2 * 3 * lr[net] + 1e-7 and dd.mean() <= 0.01 * lr[net] + 1e-9, (net, dd.max(), dd.mean())


def test_wgrad_tail_with_the_tails_block(pkg, gpu):
    """A data-parallel rank (a one-rank group with the bf16 exchange runs the N-rank path): gemm_wgrad_tail carries the head rider AND,
    as its last block, the tails block that reduces the loss / q partials (dp_tails_ride), against the per-layer schedule where
    the tails have a launch of their own and the last GEMM launch is gemm_wgrad_narrow_rider.  Same arithmetic: the statistics
    the tails produce and every parameter bit-identical."""
    B, hidden, S = 32, (1024, 1024), 58
    out = []
    for tuning, rides in ((pkg.capi.TUNE_SEPARATE_Q_TRAIN, True), (pkg.capi.TUNE_SEPARATE_Q_TRAIN | pkg.capi.TUNE_BWD_UNSHIFTED, False)):
        d = F.learner(pkg, tuning, B, hidden, S)
        d.dp_init(pkg.DQN.dp_unique_id(), half_grads=True)
        forms = set(d.update_plan()["forms"])
        assert "data_parallel" in forms and ("dp_tails_ride" in forms) == rides and ("bwd_shifted_critic" in forms) == rides, sorted(forms)
        stats = []
        for _ in range(3):
            d.dp_update_n(1)
            stats.append(d.read_stats())
        out.append((stats, [d.get_params(n) for n in range(4)]))
        d.close()
    (sa, wa), (sb, wb) = out
    assert sa == sb, (sa, sb)
    assert all(np.isfinite(s).all() for s in sa)
    for x, y in zip(wa, wb):
        np.testing.assert_array_equal(x, y)


def test_both_actor_heads_in_one_launch_equal_each_alone(pkg, gpu):
    """Step(1) runs the target actor's and the online actor's heads as blockIdx.y = 0 / 1 of one k_head_fwd launch (different
    panels, different weights); the split update (phases 10 and 11) launches each alone.  Everything downstream bit-identical."""
    B, hidden, S = 32, (1024, 1024), 58
    out = []
    for split in (False, True):
        d = F.learner(pkg, 0, B, hidden, S)
        rng = np.random.default_rng(7)
        rec = []
        for _ in range(2):
            idx = rng.integers(0, 2000, B).astype(np.int32)
            if split:
                d.update_phase(10, idx); d.update_phase(11)
            else:
                d.update_phase(0, idx)
            rec.append([d.debug_read(k) for k in ("q_target", "q_train", "y", "actor_out")])
            d.update_phase(1); d.update_phase(2)
            rec.append([d.debug_read("dq_da")])
        out.append((rec, [d.get_params(n) for n in range(4)]))
        d.close()
    (ra, wa), (rb, wb) = out
    for xs, ys in zip(ra, rb):
        for x, y in zip(xs, ys):
            np.testing.assert_array_equal(x, y)
    for x, y in zip(wa, wb):
        np.testing.assert_array_equal(x, y)
