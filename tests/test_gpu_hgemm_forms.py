"""Every fp16 launch form of the learner, one launch each through the product's own launchers (dqnhip_test_hgemm_form,
tests/csrc/hgemm_forms.hip: hgemm.hip.h compiled as libdqnhip.so compiles it, without the test-build epilogues), judged per
element against a float64 reference (tests/hgemm_ref.py).

What each case checks, in this order: two launches are bit-identical (the kernels document a fixed order); every output element
is finite (outputs arrive as one NaN bit pattern, so an unwritten element shows; inputs carry the same pattern in their pads and
guards, so a read outside an operand shows too); guard rows, pad columns and every fp32 column at or beyond n_valid32 still hold
that pattern bit for bit, in every row; fp32 outputs |got - ref scale32| <= (K + 7) u s f scale32 and fp16 outputs inside
[rne16(ref - b), rne16(ref + b)] for EVERY element, and again with b = 4 x the float32 numpy yardstick's max r x u s f; CS16 bit
for bit from the C16 the kernel wrote; the sum-of-squares slots all written, not negative, their total within the propagated
slack; db of the column sums and dW / db of the head sums within (rows + 2) u s; k_cvt16 bit for bit with pad columns +0 and
rows beyond `rows` untouched; every problem of a grouped launch bit-identical to its single launch.  Parameters: both regimes
(uniform; rows scaled by 2**-4 .. 2**4) and pad 0 / 64 on every 2-D operand.

Shapes (tests/hgemm_ref.py, shared with tests/test_hgemm_ref_host.py) are the smallest at which a form can still go wrong: per
tile the K list runs the ring of hgemm_body through prologue only, no steady trip, one and two trips, the first and the second
reuse of a stage buffer; tile counts 3 x 5 (hg_tile_of_block's remainder branch) and 2 x 4; for the wgrads one grid hg_tile_2d
accepts and many it refuses; grouped launches of 2, 3 and 4 problems of different shapes.

max r = |y - ref| / (u s f) measured on the MI355X, worst case over the cases of a form (fp32 outputs: measured; fp16 outputs: the
smallest r consistent with the rounded values; every MAXR line under `pytest -s` carries both figures):

    form                  output   yardstick max r   kernel max r   worst kernel / yardstick of one problem
    hgemm_nt<2,2,0,0>      fp16         5.42             0.65            0.18
    hgemm_nt<2,2,0,0>      fp32         4.01             1.72            0.46
    hgemm_nt<2,2,2,2>      fp16         4.51             0.57            0.23
    hgemm_nt<2,2,2,2>      fp32         4.21             1.45            0.74
    hgemm_nt<2,2,3,3>      fp32         5.53             1.56            0.58
    hgemm_nt<1,1,0,0>      fp16         3.98             0.28            0.14
    hgemm_nt<1,1,0,0>      fp32         3.02             0.75            0.25
    hgemm_nt<1,1,2,2>      fp16         4.87             0.27            0.14
    hgemm_nt<1,1,2,2>      fp32         3.00             0.76            0.36
    hgemm_nt<1,1,2,3>      fp16         3.28             0.38            0.11
    hgemm_nt<1,1,2,3>      fp32         3.83             0.67            0.20
    hgemm_nt<1,1,3,3>      fp32         4.83             0.97            0.34
    hgemm_nt<4,2,0,0>      fp16         5.91             0.84            0.27
    hgemm_nt<4,2,0,0>      fp32         3.77             1.34            0.39
    hgemm_group_db<2,2>    fp32         4.85             1.59            0.66
    hgemm_group_db<1,1>    fp32         4.36             0.73            0.25

Column sums, r = |db - ref| / (u scale sum|dY|): k_db16_cols 0.32, as blocks of hgemm_group_db 0.26; head sums, r of dW: 1.04.
An MFMA adds 16 exact products before it rounds, so a kernel chain has K / 16 roundings where the BLAS product has K: every
kernel figure lies below its yardstick, the factor of 4 (gemm_ref.TIGHT_FACTOR) has a margin of five and more, and the derived
bound allows r up to K + 7 (71 .. 1159).  No element of any case left the fp16 interval: the kernels' float -> half conversion
rounds to nearest even and keeps subnormal results, as hgemm_ref.rne16 does.

Sensitivity, shown on scratch copies of hgemm.hip.h (never in the tree): hg_tile_of_block repeating a tile on one XCD fails the 3 x 5
tile cases of every hgemm_nt form and the dgrad + wgrad pairs ("not finite: .. C16[128][256]": the tile nobody wrote); the <1,1>
merge without p3 fails every case of the 64 x 64 tile ("outside the derived interval: .. C16[0][0]"); db16_cols_block's tail loop
stepping 64 rows fails test_db16_cols at rows 64 and 192 ("outside the derived bound: .. db0[0][0]"); the seed_w factor taken from
the fp32 value fails the three "seedkink" cases ("head seed: .. CS16[0][0]", a positive value that rounds to fp16 zero).
"""
import ctypes as C

import numpy as np
import pytest

import hgemm_ref as H
import testlib

pytestmark = pytest.mark.gpu


class Buf(C.Structure):
    _fields_ = [("host", C.c_void_p), ("count", C.c_int64), ("offset", C.c_int64)]


class Prob(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("M", "N", "K", "lda", "ldb", "ta", "tb", "ldc16", "ldc32", "n_valid32", "relu", "ldm", "ldcs16", "reserved")] + \
               [("scale32", C.c_float), ("seed_scale", C.c_float)] + \
               [(n, Buf) for n in ("A", "B", "mask", "bias", "seed_w", "C16", "CS16", "C32", "sumsq_partial")]


class Db(C.Structure):
    _fields_ = [("dy", Buf), ("ld", C.c_int32), ("n_out", C.c_int32), ("rows", C.c_int32), ("reserved", C.c_int32), ("db", Buf)]


class Cvt(C.Structure):
    _fields_ = [("src", Buf), ("ld_src", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("ld16", C.c_int32), ("scale", C.c_float),
                ("reserved", C.c_int32), ("dst", Buf)]


class Riders(C.Structure):
    _fields_ = [("n_db", C.c_int32), ("db_scale", C.c_float), ("db", Db * 8), ("db_sumsq", Buf)] + \
               [(n, C.c_int32) for n in ("nh", "lddy", "H", "rows", "blocks", "reserved")] + \
               [(n, Buf) for n in ("dy", "X16", "dW", "hdb", "partial")] + \
               [("n_cvt", C.c_int32), ("reserved2", C.c_int32), ("cvt", Cvt * 8)]


def _entry():
    fn = testlib.load_test_h().dqnhip_test_hgemm_form
    fn.restype = C.c_int
    fn.argtypes = [C.c_int32, C.c_int32, C.POINTER(Prob), C.POINTER(Riders)]
    return fn


def _buf(panel):
    return Buf(panel.raw.ctypes.data, panel.raw.size, panel.offset)


def _c_problem(pr):
    c = Prob(M=pr.M, N=pr.N, K=pr.K, lda=pr.ld("A"), ldb=pr.ld("B"), ta=pr.ta, tb=pr.tb, ldc16=pr.ld("C16"), ldc32=pr.ld("C32"),
             n_valid32=pr.n_valid32, relu=pr.relu, ldm=pr.ld("mask"), ldcs16=pr.ld("CS16"), scale32=pr.scale32, seed_scale=pr.seed_scale)
    for name, panel in list(pr.inp.items()) + list(pr.out.items()):
        setattr(c, name, _buf(panel))
    return c


def _c_riders(db=None, head=None, cvt=None):
    r = Riders()
    if db is not None:
        r.n_db, r.db_scale = len(db.widths), db.scale
        for i, w in enumerate(db.widths):
            r.db[i] = Db(dy=_buf(db.inp[f"dy{i}"]), ld=db.inp[f"dy{i}"].ld, n_out=w, rows=db.rows, db=_buf(db.out[f"db{i}"]))
        if "db_sumsq" in db.out:
            r.db_sumsq = _buf(db.out["db_sumsq"])
    if head is not None:
        r.nh, r.lddy, r.H, r.rows, r.blocks = head.nh, head.lddy, head.H, head.rows, head.H // 64
        r.dy, r.X16, r.dW, r.hdb = _buf(head.inp["dy"]), _buf(head.inp["X16"]), _buf(head.out["dW"]), _buf(head.out["hdb"])
        if "partial" in head.out:
            r.partial = _buf(head.out["partial"])
    if cvt is not None:
        r.n_cvt = len(cvt.entries)
        for i, (rows, cols, ld16, scale) in enumerate(cvt.entries):
            r.cvt[i] = Cvt(src=_buf(cvt.inp[f"src{i}"]), ld_src=cvt.inp[f"src{i}"].ld, rows=rows, cols=cols, ld16=ld16, scale=scale,
                           dst=_buf(cvt.out[f"dst{i}"]))
    return r


def call(form, problems, db=None, head=None, cvt=None, riders=None):
    """one call of the entry on freshly sentinel-filled outputs -> return code"""
    parts = list(problems) + [x for x in (db, head, cvt) if x is not None]
    for p in parts:
        p.reset_outputs()
    arr = (Prob * max(1, len(problems)))(*[_c_problem(pr) for pr in problems])
    if riders is None and (db is not None or head is not None or cvt is not None):
        riders = _c_riders(db, head, cvt)
    return _entry()(form, len(problems), arr, C.byref(riders) if riders is not None else None)


def launch(form, problems, **riders):
    """-> the bit image of every output buffer, per part (problems, then the riders given)"""
    rc = call(form, problems, **riders)
    assert rc == 0, (H.FORM_NAME[form], rc)
    return [p.snapshot() for p in list(problems) + [x for x in riders.values() if x is not None]]


def same_bits(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def run_and_check(form, problems, tag, **riders):
    """launch twice (bit-identical), then the comparator on every part; prints the yardstick and kernel max r"""
    first = launch(form, problems, **riders)
    again = launch(form, problems, **riders)
    for i, (a, b) in enumerate(zip(first, again)):
        assert same_bits(a, b), f"{H.FORM_NAME[form]} {tag} part {i}: two runs differ (the kernels document a fixed reduction order)"
    for i, pr in enumerate(problems):
        st = pr.check(f"{H.FORM_NAME[form]} {tag} problem {i}")
        print(f"MAXR {H.FORM_NAME[form]} {tag} problem {i}: yardstick {st['yard_r']:.3f} kernel {st['kernel_r']:.3f}"
              + (" (fp16: lower bound)" if "C32" not in pr.out else ""))
    for name, rd in riders.items():
        if rd is not None:
            st = rd.check(f"{H.FORM_NAME[form]} {tag} {name}")
            print(f"MAXR {H.FORM_NAME[form]} {tag} {name}: " + " ".join(f"{k} {v:.3f}" for k, v in st.items()))
    return again


SINGLE = H.single_cases()
GROUPED = H.grouped_cases()
# the single-problem form that runs the same body as problem i of a grouped form
SINGLE_FORM = {H.FWD: {64: H.NT_SMALL_FWD, 128: H.NT_BIG_FWD, 256: H.NT_HUGE_FWD}, H.DGRAD: {64: H.NT_SMALL_DGRAD, 128: H.NT_BIG_DGRAD},
               H.WGRAD: {64: H.NT_SMALL_WGRAD, 128: H.NT_BIG_WGRAD}}


@pytest.mark.parametrize("pad", H.PADS)
@pytest.mark.parametrize("regime", H.REGIMES)
@pytest.mark.parametrize("form,fn", [pytest.param(f, fn, id=name) for name, f, fn in SINGLE])
def test_single_launches(pkg, gpu, form, fn, regime, pad):
    """hgemm_launch_batch with one problem: forward (bias + leaky ReLU -> C16, with seed_w / CS16, with C16 and C32), dgrad (mask ->
    C16 with ldm != ldc16; layer 0: no mask, C32 * 1/4096), wgrad (C32 * 1/4096 + sumsq_partial, n_valid32 = N and N - 64, a grid
    hg_tile_2d accepts and grids it refuses), on each tile"""
    run_and_check(form, fn(regime, pad), f"{regime} pad {pad}")


@pytest.mark.parametrize("pad", H.PADS)
@pytest.mark.parametrize("regime", H.REGIMES)
@pytest.mark.parametrize("form,fn", [pytest.param(f, fn, id=name) for name, f, fn in GROUPED])
def test_grouped_launches(pkg, gpu, form, fn, regime, pad):
    """2, 3 and 4 problems of different shapes in one hgemm_nt launch (tile_end), the per-layer dgrad + wgrad pair (once the dgrad has
    more tiles, once the wgrad) and the forward pair on the 256 x 128 tile: each problem as judged alone, and bit-identical to its
    single launch"""
    problems = fn(regime, pad)
    tag = f"{regime} pad {pad}"
    grouped = run_and_check(form, problems, tag + " grouped")
    for i, pr in enumerate(problems):
        single = launch(SINGLE_FORM[pr.kind][pr.tile[0]], [pr])[0]
        assert same_bits(grouped[i], single), f"{H.FORM_NAME[form]} {tag}: problem {i} of the grouped launch differs from its single launch"


@pytest.mark.parametrize("pad", H.PADS)
@pytest.mark.parametrize("regime", H.REGIMES)
@pytest.mark.parametrize("form,rows,nh", [pytest.param(f, r, n, id=f"{H.FORM_NAME[f]}-rows{r}-nh{n}") for f, r, n in H.GROUP_CASES])
def test_group_db(pkg, gpu, form, rows, nh, regime, pad):
    """hgemm_group_db_launch: 1, 3 and 4 wgrads of different shapes, the column sums of 1 and 4 layers of different widths, the head
    sums (none, nh = 1 with lddy 1, nh = 10 with lddy 16) in one launch.  The grid order — tiles, head blocks, column-sum blocks — is
    pinned by the outputs: every output of every part is written and nothing else; each wgrad is bit-identical to its single launch,
    the column sums to k_db16_cols alone"""
    wg, db, head = H.group_case(form, rows, nh, regime, pad)
    tag = f"rows {rows} nh {nh} {regime} pad {pad}"
    grouped = run_and_check(form, wg, tag, db=db, head=head)
    for i, pr in enumerate(wg):
        single = launch(SINGLE_FORM[H.WGRAD][pr.tile[0]], [pr])[0]
        assert same_bits(grouped[i], single), f"{H.FORM_NAME[form]} {tag}: wgrad {i} differs from its single launch"
    alone = launch(H.DB16_COLS, [], db=db)[0]
    assert same_bits(grouped[len(wg)], alone), f"{H.FORM_NAME[form]} {tag}: the column sums differ from k_db16_cols alone"


@pytest.mark.parametrize("pad", H.PADS)
@pytest.mark.parametrize("regime", H.REGIMES)
@pytest.mark.parametrize("widths", H.DB16_WIDTHS, ids=lambda w: f"{len(w)}layers")
@pytest.mark.parametrize("rows", H.DB16_ROWS)
def test_db16_cols(pkg, gpu, rows, widths, regime, pad):
    """k_db16_cols<0> alone: 128 rows per trip, then 32-row tail steps — rows 64 and 192 end in the tail loop"""
    run_and_check(H.DB16_COLS, [], f"rows {rows} {regime} pad {pad}", db=H.db16_case(rows, widths, regime, pad))


@pytest.mark.parametrize("pad", H.PADS)
@pytest.mark.parametrize("regime", H.REGIMES)
def test_cvt16(pkg, gpu, regime, pad):
    """cvt16_add + cvt16_launch as sync_w16 calls them (no transposed output): three entries of different shapes in one launch"""
    run_and_check(H.CVT16, [], f"{regime} pad {pad}", cvt=H.cvt_case(regime, pad))


def test_invalid_calls_are_refused(pkg, gpu):
    """return code 1 before anything is uploaded or launched: every output is still all sentinel"""
    def refused(form, problems, **riders):
        rc = call(form, problems, **riders)
        parts = list(problems) + [x for x in riders.values() if x is not None and not isinstance(x, Riders)]
        return rc == 1 and all(p.outputs_untouched() for p in parts)

    mk = lambda form, kind, M, N, K, **kw: H.make(form, kind, M, N, K, "uniform", 0, "refuse", **kw)
    assert not refused(H.NT_BIG_FWD, [mk(H.NT_BIG_FWD, H.FWD, 128, 128, 64)])                 # (the probe itself: a valid call is not refused)
    assert refused(H.NT_BIG_FWD, [mk(H.NT_BIG_FWD, H.FWD, 192, 128, 64)])                     # M = 192 on the 128-tile
    assert refused(H.NT_SMALL_FWD, [mk(H.NT_SMALL_FWD, H.FWD, 64, 64, 64)])                   # K = 64 on the small tile (K step 128)
    assert refused(H.NT_HUGE_FWD, [mk(H.NT_HUGE_FWD, H.WGRAD, 256, 128, 64)])                 # a reduction-major problem on the 256 x 128 tile
    w = lambda: mk(H.NT_SMALL_WGRAD, H.WGRAD, 64, 64, 128)
    d = lambda: mk(H.NT_SMALL_DGRAD, H.DGRAD, 64, 64, 128)
    assert refused(H.NT_SMALL_BWD, [d(), w(), d()])                                           # the pair is two problems
    assert refused(H.NT_SMALL_DGRAD, [d(), d(), w()])                                         # mixed orientations beyond problem 1
    assert refused(H.NT_SMALL_WGRAD, [w(), w(), d(), w()])
    assert refused(H.GROUP_DB_SMALL, [d()])                                                   # a k-major problem for hgemm_group_db
    assert refused(H.GROUP_DB_BIG, [mk(H.GROUP_DB_BIG, H.FWD, 128, 128, 64)])
    assert refused(H.NT_SMALL_WGRAD, [w(), w(), w(), w(), w()])                               # 5 problems
    assert refused(12, [w()])                                                                  # no such form
    # head riders
    db, head = H.DbRider(128, [64], 1), H.HeadRider(128, 128, 1, 2)
    r = _c_riders(db, head); r.blocks = 1
    assert refused(H.GROUP_DB_SMALL, [w()], riders=r) and db.outputs_untouched() and head.outputs_untouched()    # head.blocks * 64 != H
    r = _c_riders(db, head); r.nh = 4
    assert refused(H.GROUP_DB_SMALL, [w()], riders=r) and head.outputs_untouched()            # nh = 4
    assert refused(H.NT_SMALL_WGRAD, [w()], db=db)                                            # riders on a form that takes none
    assert refused(H.DB16_COLS, [w()], db=db)                                                 # a problem on a riders-only form
    # a misaligned offset, ld < width, an operand that does not fit its buffer
    pr = w(); pr.inp["A"].offset += 4
    assert refused(H.NT_SMALL_WGRAD, [pr])
    pr = w(); pr.out["C32"].offset += 2
    assert refused(H.NT_SMALL_WGRAD, [pr])
    pr = d(); pr.inp["mask"].ld = 32
    assert refused(H.NT_SMALL_DGRAD, [pr])
    pr = d(); pr.M = 128
    assert refused(H.NT_SMALL_DGRAD, [pr])
    pr = w(); pr.n_valid32 = 60
    assert refused(H.NT_SMALL_WGRAD, [pr])
    cv = H.CvtRider([(64, 68, 128, 1.0)], 3)
    r = _c_riders(cvt=cv); r.cvt[0].rows = 64 + 2 * H.GUARD_ROWS      # past the guard rows behind the panel
    assert refused(H.CVT16, [], riders=r) and cv.outputs_untouched()
