"""What tests/test_gpu_packed_args.py shares: one launch of a GEMM form through dqnhip_test_gemm_form (tests/csrc/gemm_forms.hip) on
guard-banded buffers judged by tests/gemm_ref.py, and a short run of the fp32 learner under a tuning-flag word.  (The same
helpers as in test_gpu_gemm_forms.py / test_gpu_tuning_flags.py, here as a library so that no test file imports another.)"""
import ctypes as C

import numpy as np

import gemm_ref as G
import testlib
from synth import synth_replay

(FWD_DIRECT_2x2, FWD_DIRECT_4x2, FWD_LDS_1x1, FWD_LDS_2x2, FWD_LDS_4x2, FWD_LDS_4x2_ONE_IMAGE, DGRAD_DIRECT, DGRAD_LDS, DGRAD_NARROW,
 WGRAD_NARROW, BWD_SEQ, BWD_SEQ_LDS, BWD_PAIR, BWD_PAIR_LDS, WGRAD_TAIL_1, WGRAD_TAIL_NO) = range(16)      # dqnhip_internal.h DQNHIP_FORM_*
FORM_NAME = ["fwd_direct<2,2>", "fwd_direct<4,2>", "fwd_lds<1,1,true>", "fwd_lds<2,2,true>", "fwd_lds<4,2,true>", "fwd_lds<4,2,true,1>",
             "dgrad_direct<1,1>", "dgrad_lds<1,1>", "dgrad_narrow", "wgrad_narrow<1>", "bwd_seq<false>", "bwd_seq<true>",
             "bwd_pair_direct<1,false>", "bwd_pair_direct<1,true>", "wgrad_tail<1>", "wgrad_tail<kNO>"]


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
    """launch twice (bit-identical), then gemm_ref's comparator on every problem; returns the output bits per problem"""
    first = launch(form, problems)
    again = launch(form, problems)
    for i, (a, b) in enumerate(zip(first, again)):
        assert same_bits(a, b), f"{FORM_NAME[form]} {tag} problem {i}: two runs differ"
    for i, pr in enumerate(problems):
        st = G.check(pr, f"{FORM_NAME[form]} {tag} problem {i}")
        print(f"MAXR {FORM_NAME[form]} {tag} problem {i}: yardstick {st['yard_r']:.3f} kernel {st['kernel_r']:.3f}")
    return again


def learner(pkg, tuning, B, hidden, S, **kw):
    d = pkg.DQN(S, minibatch=B, hidden=hidden, memory=4096, seed=3, tuning=tuning, **kw)
    d.add_transitions_arrays(*synth_replay(np.random.default_rng(5), 2000, S))
    return d


def run32(pkg, tuning, B, hidden, S, n_up=3, use_graph=False, want=(), unwanted=()):
    """n_up updates of the fp32 learner; the plan must hold the forms `want` and none of `unwanted`.  Returns (stats per update,
    (q_policy, dq_da) per update, parameters + Adam moments + gradients of every net)."""
    d = learner(pkg, tuning, B, hidden, S, use_graph=use_graph)
    forms = set(d.update_plan()["forms"])
    assert set(want) <= forms and not (set(unwanted) & forms), (tuning, sorted(forms))
    rng = np.random.default_rng(7)
    stats, dbg = [], []
    for _ in range(n_up):
        stats.append(d.UpdateActorCritic(rng.integers(0, 2000, B).astype(np.int32)))
        dbg.append((d.debug_read("q_policy"), d.debug_read("dq_da")))
    w = [d.get_params(n) for n in range(4)] + [d.get_params(n, k) for n in (0, 1) for k in (pkg.KIND_M, pkg.KIND_V, pkg.KIND_G)]
    d.close()
    return stats, dbg, w


def assert_same_run(a, b):
    assert a[0] == b[0], (a[0], b[0])
    for (qa, da), (qb, db) in zip(a[1], b[1]):
        np.testing.assert_array_equal(qa, qb); np.testing.assert_array_equal(da, db)
    for x, y in zip(a[2], b[2]):
        np.testing.assert_array_equal(x, y)
