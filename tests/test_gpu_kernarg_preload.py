"""The kernarg preload path of the chain's fp32 GEMM kernels (GemmPreload, dqn-hfo_amd/csrc/gemm_common.hip.h): the kernels take
the operand bases, leading dimensions, reduction length and tile decode of their first tile as 14 leading scalar words — which
gfx950 delivers in SGPRs at wave launch — and everything else from the GemmArgs behind them.  Only address formation moves, so
what can go wrong is WHICH tile a workgroup computes and WHICH problem's operands it reads:

  * a PAIR of equal shape (one copy of the shape words, two pairs of operand bases, the split between them) — the form of
    gemm_fwd_lds<4,2,true,1>'s actor / actor_target and critic / critic_target launches.  The pairs of tests/test_gpu_first_load_path.py
    are of unequal shape and take the GemmArgs path; these take the preloaded one.  Same shape, different data, different
    buffers: each problem bit-identical to its single launch (itself the one-problem preloaded form) and inside gemm_ref's
    float64 bound;
  * gemm_wgrad_tail (the preloaded words are the 64 x 64 wgrad's record, whose tiles come behind the narrow ones in the grid) and
    gemm_bwd_seq (which keeps the GemmArgs path: its first tile gained nothing from the preloaded words) with unequal tile counts
    of their two problems: the workgroups beyond a problem's tiles must skip it, the blocks in front of the preloaded record must
    not take it;
  * all of these with the tuning bit clear AND set, bit for bit: tests/csrc/gemm_forms_nopreload.hip is the harness entry once
    more in a library of its own, built here with the preload option (so the words really arrive in SGPRs), whose launches can
    carry LaunchOn::no_preload — what DQNHIP_TUNE_NO_KERNARG_PRELOAD sets in the learner;
  * the learner, with DQNHIP_TUNE_NO_KERNARG_PRELOAD clear and set (every block marked "not valid": the GemmArgs path behind one
    uniform branch), eager and as a multi-update graph: every weight, moment, loss and avg-Q bit-identical.

Shapes: the small ones of tests/test_gpu_first_load_path.py (rows 96 / 192 / 32, widths 192 / 256 / 320 / 512, pad 8 / 24,
reductions 512 for the LDS bodies, 64 / 128 for the direct ones).  No tolerance of this test's own.  The block itself, field by
field and at its limits: tests/test_kernarg_preload_host.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gemm_forms_lib as F
import gemm_ref as G
from synth import synth_replay

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def bitlib():
    """tests/csrc/gemm_forms_nopreload.hip as a library of its own, with the product's preload option (a few seconds of hipcc)"""
    so = os.path.join(CSRC, "libdqnhip_test_nopreload.so")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unused-variable",
           "-Wno-unused-result", "-Wno-unused-value", "-I" + os.path.join(CSRC, "..", "..", "dqn-hfo_amd", "csrc"), "-I" + CSRC,
           "-mllvm", "-amdgpu-kernarg-preload-count=14", "-shared", "-o", so, os.path.join(CSRC, "gemm_forms_nopreload.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(so)
    lib.dqnhip_test_gemm_form.restype = C.c_int
    lib.dqnhip_test_gemm_form.argtypes = [C.c_int32, C.c_int32, C.POINTER(F.Prob)]
    lib.dqnhip_test_set_no_preload.restype = None
    lib.dqnhip_test_set_no_preload.argtypes = [C.c_int]
    return lib


def launch_bit(lib, bit_set, form, problems):
    """F.launch through `lib` with the tuning bit clear / set: the bit image of every output buffer, per problem"""
    for pr in problems:
        pr.reset_outputs()
    arr = (F.Prob * len(problems))(*[F._c_problem(pr) for pr in problems])
    lib.dqnhip_test_set_no_preload(1 if bit_set else 0)
    try:
        rc = lib.dqnhip_test_gemm_form(form, len(problems), arr)
    finally:
        lib.dqnhip_test_set_no_preload(0)
    assert rc == 0, (F.FORM_NAME[form], rc)
    return [pr.snapshot() for pr in problems]


def assert_bit_clear_equals_bit_set(lib, form, problems, reference, tag):
    """the launch with the words preloaded and with the block marked "not valid", each against the harness's checked bits"""
    for bit_set in (False, True):
        got = launch_bit(lib, bit_set, form, problems)
        for i, (g, r) in enumerate(zip(got, reference)):
            assert F.same_bits(g, r), f"{F.FORM_NAME[form]} {tag}: problem {i} with the bit {'set' if bit_set else 'clear'} differs from the harness launch"

# form -> (mode, [(rows, width, pad)], reduction).  Every grouped form that takes two problems: the forms with a preloaded path
# (fwd_lds, dgrad_lds) and, as a control on the same shapes, the ones that keep the GemmArgs path.
PAIRS = {
    F.FWD_LDS_1x1: (G.FWD, [(96, 192, 8), (16, 320, 24)], 512), F.FWD_LDS_2x2: (G.FWD, [(96, 192, 8), (192, 256, 0), (32, 320, 24)], 512),
    F.FWD_LDS_4x2: (G.FWD, [(96, 192, 8), (192, 512, 0), (32, 320, 24)], 512), F.FWD_LDS_4x2_ONE_IMAGE: (G.FWD, [(96, 192, 8), (192, 512, 0), (32, 320, 24)], 512),
    F.DGRAD_LDS: (G.DGRAD, [(96, 192, 8), (192, 512, 0), (32, 320, 24)], 512),
    F.FWD_DIRECT_2x2: (G.FWD, [(96, 192, 8)], 64), F.FWD_DIRECT_4x2: (G.FWD, [(96, 192, 8)], 128), F.DGRAD_DIRECT: (G.DGRAD, [(96, 192, 8)], 128),
}
CASES = [(f, s) for f in PAIRS for s in range(len(PAIRS[f][1]))]


def _problem(form, s, which):
    mode, shapes, red = PAIRS[form]
    rows, width, pad = shapes[s]
    seed = 31000 + 64 * form + 8 * s + which
    if mode == G.DGRAD:        # the two problems at different column offsets of (different) wider panels
        return G.Problem(mode, width, rows, red, seed=seed, pad=pad, col0=16 * (which + 1), panel_w=width + 64)
    return G.Problem(mode, width, rows, red, seed=seed, pad=pad)


@pytest.mark.parametrize("form,s", CASES, ids=["%s-shape%d" % (F.FORM_NAME[f], s) for f, s in CASES])
def test_pair_of_equal_shape(pkg, gpu, bitlib, form, s):
    if PAIRS[form][0] == G.DGRAD:
        # (a column offset changes no leading dimension: both problems' panels are width + 64 wide)
        assert _problem(form, s, 0).ldp == _problem(form, s, 1).ldp
    pair = [_problem(form, s, 0), _problem(form, s, 1)]
    assert (pair[0].ldp, pair[0].ldq, pair[0].Kred, pair[0].Pdim, pair[0].Qdim) == (pair[1].ldp, pair[1].ldq, pair[1].Kred, pair[1].Pdim, pair[1].Qdim)
    bits = F.run_and_check(form, pair, f"equal pair, shape {s}")
    assert_bit_clear_equals_bit_set(bitlib, form, pair, bits, f"equal pair, shape {s}")
    swapped = F.run_and_check(form, [_problem(form, s, 1), _problem(form, s, 0)], f"equal pair swapped, shape {s}")
    for which in (0, 1):
        (alone,) = F.run_and_check(form, [_problem(form, s, which)], f"problem {which} alone")
        assert F.same_bits(bits[which], alone), f"{F.FORM_NAME[form]} shape {s}: problem {which} of the pair differs from its single launch"
        assert F.same_bits(swapped[1 - which], alone), f"{F.FORM_NAME[form]} shape {s}: problem {which} as the pair's other half differs"


@pytest.mark.parametrize("lds", [False, True], ids=["direct", "lds"])
@pytest.mark.parametrize("rows,cols,outs", [(192, 192, 64), (32, 320, 256), (96, 256, 192), (96, 512, 64)], ids=["36d-3w", "10d-20w", "24d-12w", "48d-8w"])
def test_bwd_seq_skips_beyond_either_record(pkg, gpu, bitlib, lds, rows, cols, outs):
    """gemm_bwd_seq: wgrad tile b, then dgrad tile b; the grid is the larger count.  More dgrad tiles than wgrad tiles (the
    workgroups beyond a record's tiles skip it), more wgrad tiles, on and off the XCD map (tiles_p = cols / 64 = 3, 5, 4, 8).  dgrad against the dgrad form alone, wgrad against the tail launch's
    wide slot, bit for bit."""
    red = 512 if lds else 128
    seq, dgrad = (F.BWD_SEQ_LDS, F.DGRAD_LDS) if lds else (F.BWD_SEQ, F.DGRAD_DIRECT)
    mk_d = lambda: G.Problem(G.DGRAD, cols, rows, red, seed=33000 + cols, pad=24)
    mk_w = lambda: G.Problem(G.WGRAD, cols, outs, 32, seed=33100 + cols, pad=8, bq=64)
    (sd, sw) = F.run_and_check(seq, [mk_d(), mk_w()], f"bwd_seq {rows}x{cols}x{outs}")
    assert_bit_clear_equals_bit_set(bitlib, seq, [mk_d(), mk_w()], (sd, sw), f"bwd_seq {rows}x{cols}x{outs}")
    (ad,) = F.run_and_check(dgrad, [mk_d()], "dgrad alone")
    assert F.same_bits(sd, ad), "dgrad tiles differ between gemm_bwd_seq and the dgrad launch"
    (tw, _) = F.run_and_check(F.WGRAD_TAIL_1, [mk_w(), G.Problem(G.WGRAD, 64, 16, 32, seed=33200, bq=16)], "wgrad_tail")
    assert F.same_bits(tw, sw), "the tail launch's 64 x 64 wgrad tiles differ from gemm_bwd_seq's"


@pytest.mark.parametrize("form", [F.WGRAD_TAIL_1, F.WGRAD_TAIL_NO], ids=lambda f: F.FORM_NAME[f])
@pytest.mark.parametrize("outs1,cols1,outs0,cols0", [(64, 192, 192, 320), (192, 512, 32, 64), (128, 320, 96, 256)], ids=["3w-60n", "24w-2n", "10w-24n"])
def test_wgrad_tail_preloaded_record_starts_behind_the_narrow_tiles(pkg, gpu, bitlib, form, outs1, cols1, outs0, cols0):
    """gemm_wgrad_tail: the narrow wgrad's 64 x 16 tiles (record 1, the GemmArgs path) come first in the grid, the 64 x 64 tiles
    (record 0, the preloaded words) from block `first` on.  Many narrow tiles in front of few wide ones and the reverse; the narrow
    slot against gemm_wgrad_narrow alone, the wide slot against gemm_bwd_seq's wgrad tiles (the GemmArgs path)."""
    mk1 = lambda: G.Problem(G.WGRAD, cols1, outs1, 64, seed=34000 + cols1, pad=8, bq=64)
    mk0 = lambda: G.Problem(G.WGRAD, cols0, outs0, 128, seed=34100 + cols0, pad=24, bq=16)
    (tw, tn) = F.run_and_check(form, [mk1(), mk0()], "wgrad_tail")
    assert_bit_clear_equals_bit_set(bitlib, form, [mk1(), mk0()], (tw, tn), "wgrad_tail")
    (an,) = F.run_and_check(F.WGRAD_NARROW, [mk0()], "wgrad_narrow alone")
    assert F.same_bits(tn, an), "the tail launch's narrow wgrad tiles differ from gemm_wgrad_narrow's"
    (_, sw) = F.run_and_check(F.BWD_SEQ, [G.Problem(G.DGRAD, 64, 16, 64, seed=34200), mk1()], "bwd_seq beside a one-tile dgrad")
    assert F.same_bits(tw, sw), "the tail launch's 64 x 64 wgrad tiles differ from gemm_bwd_seq's"


# ---- the learner: every chain kernel, the bit clear and set ---------------------------------------------------------------------
LEARNERS = [(64, (1024, 1024, 1024), 58),       # the shifted_fp32 plan of tests/test_gpu_kernel_timing.py: launches every chain kernel
            (32, (256, 128, 64, 64), 59)]


@pytest.mark.parametrize("B,hidden,S", LEARNERS, ids=["b64-3x1024", "b32-small"])
def test_learner_eager_bit_clear_equals_bit_set(pkg, gpu, B, hidden, S):
    """three consecutive eager updates: statistics, q / dQ/da, parameters, Adam moments and gradients of every net"""
    # (the shifted plan: k_dgrad_qtrain, gemm_bwd_seq, gemm_wgrad_tail with the head riders — with the bit set as without it)
    want = {"bwd_shifted_critic", "bwd_shifted_actor", "q_train_in_dgrad", "head_wgrad_rides_critic", "head_wgrad_rides_actor"} if B == 64 else set()
    a = F.run32(pkg, 0, B, hidden, S, want=want)
    b = F.run32(pkg, pkg.capi.TUNE_NO_KERNARG_PRELOAD, B, hidden, S, want=want)
    F.assert_same_run(a, b)


@pytest.mark.parametrize("B,hidden,S", LEARNERS, ids=["b64-3x1024", "b32-small"])
def test_learner_multi_update_graph_bit_clear_equals_bit_set(pkg, gpu, B, hidden, S):
    """dqnhip_update_async_n, 19 updates: one graph of sixteen and three single updates; the same update plan either way"""
    out = []
    for tuning in (0, pkg.capi.TUNE_NO_KERNARG_PRELOAD):
        d = pkg.DQN(S, minibatch=B, hidden=hidden, memory=4096, seed=11, tuning=tuning, use_graph=True)
        d.add_transitions_arrays(*synth_replay(np.random.default_rng(2), 3000, S))
        plan = d.update_plan()
        d.update_async_n(19)
        st = d.read_stats()
        w = [d.get_params(k) for k in range(4)] + [d.get_params(k, kind) for k in (0, 1) for kind in (pkg.KIND_M, pkg.KIND_V)]
        out.append((st, w, (d.actor_iter(), d.critic_iter()), plan))
        d.close()
    assert out[0][0] == out[1][0] and out[0][2] == out[1][2] == (19, 19)
    assert out[0][3] == out[1][3], "the tuning bit must not change the update plan"
    for x, y in zip(out[0][1], out[1][1]):
        np.testing.assert_array_equal(x, y)
