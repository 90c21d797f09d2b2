"""Float64 reference and per-element comparator for the fp32 tower GEMMs (numpy only).

A `Problem` is one GemmProblem of dqn-hfo_amd/csrc/gemm_common.hip.h, C[q][p] = sum_k Pop(p,k) Qop(q,k):

    FWD    C = lrelu(Q @ P.T + bias)          P [Pdim][Kred], Q [Qdim][Kred]
    DGRAD  C = (Q @ P) * lrelu'(mask)         P [Kred][Pdim], Q [Qdim][Kred], mask [Qdim][Pdim]
    WGRAD  C = Q.T @ P, db = Q.sum(0)         P [Kred][Pdim], Q [Kred][Qdim]
           partial: one sum-of-squares slot per tile, compared as its total against sum(C**2) + sum(db**2)
    FWD extras: C2 = (-seed_w[p]) * lrelu'(C);  dot_out[q][p/16] = sum over 16 columns of C * dot_w;
                xcopy_dst[j][p] = P[p][xcopy_col + j], bit-exact

Every operand lives in a `Panel`: a flat float32 buffer with guard rows before and after, a pitch that may exceed the
width, possibly at a column offset inside a wider panel, everything prefilled with ONE fixed NaN bit pattern.  A kernel that
indexes with a dimension where it should use a leading dimension reads NaN or leaves NaN behind; one that leaves its tile
overwrites a sentinel.  tests/test_gemm_ref_host.py shows (without a GPU) that the comparator accepts a float32 product
and rejects each of those faults; tests/test_gpu_gemm_forms.py feeds it what the kernels wrote.

Error bounds.  u = 2**-24, s_ij = sum_k |a_ik| |b_jk| (+ |bias_j|) in float64.  Any ordering of fp32 fma / add over
`red` terms stays within gamma_red * s_ij, so |got - ref| <= (red + EXTRA_ROUNDINGS) * u * s_ij must hold for EVERY
element: a wrong value in a row of small magnitude cannot hide behind a large row.  The tight bound is measured at test time
against the reference, not against the kernel: r_ij = |y - ref| / (u * s_ij) for y = the plain float32 numpy product of
the same inputs; the kernel's max r may be at most TIGHT_FACTOR times that yardstick's max r.
"""
import numpy as np

FWD, DGRAD, WGRAD = 0, 1, 2
U = 2.0 ** -24
SLOPE32 = np.float32(0.01)                  # kLeakySlope, as the kernels hold it
SLOPE = float(SLOPE32)
SENTINEL_BITS = np.uint32(0x7FC0DEAD)       # a quiet NaN with a payload nothing computes by accident
GUARD_ROWS = 2
# bias add, ReLU (one product with the slope), ReLU' mask, the four-wave merge (two additions) and the final rounding
EXTRA_ROUNDINGS = 8
# The kernel's split-K order (four waves x a chain of 4-deep MFMA steps) differs from the BLAS's, and the maximum over
# 10^4 - 10^5 elements fluctuates; a product with an 11-bit mantissa is off by ~three orders of magnitude, far outside.
# Measured on the MI355X: kernel max r 1.04 .. 1.69, yardstick max r 1.36 .. 4.61, kernel / yardstick of one problem at most 0.87
# (dgrad_lds<1,1>), i.e. no correct kernel comes near the factor; per form: the table in test_gpu_gemm_forms.py.
TIGHT_FACTOR = 4.0
# the head dot adds a 16-term fp32 dot product (four fma per lane, two shuffle additions) on top of the activations' own error
DOT_ROUNDINGS = 18
# sum-of-squares partials: positive terms; per thread a chain of at most 20 fma (16 of a 64 x 64 tile's 4096 elements over 256
# threads, 4 more for db), six wave-reduction levels, two more over the four waves, each square rounded once: <= 32 roundings
PARTIAL_ROUNDINGS = 32
MAX_BRANCH_SHARE = 1e-3                     # ReLU branch flips: at most 0.1 % of the elements may sit within the bound of 0


def sentinel(n):
    return np.full(int(n), SENTINEL_BITS, np.uint32).view(np.float32)


class Panel:
    """A [rows][cols] operand at column `col0` of a [GUARD_ROWS + rows + GUARD_ROWS][ld] buffer of sentinels."""

    def __init__(self, rows, cols, ld=None, col0=0):
        self.rows, self.cols, self.col0 = int(rows), int(cols), int(col0)
        self.ld = int(ld) if ld is not None else self.cols + self.col0
        assert self.col0 + self.cols <= self.ld
        self.buf = sentinel((self.rows + 2 * GUARD_ROWS) * self.ld)
        self.offset = GUARD_ROWS * self.ld + self.col0

    def view(self):
        return self.buf.reshape(-1, self.ld)[GUARD_ROWS:GUARD_ROWS + self.rows, self.col0:self.col0 + self.cols]

    def put(self, a):
        self.view()[...] = np.asarray(a, np.float32).reshape(self.rows, self.cols)
        return self

    def reset(self):
        self.buf.view(np.uint32)[...] = SENTINEL_BITS

    def outside(self):
        """bool [all rows][ld]: True on guard rows, pad columns and the rest of a wider panel"""
        m = np.ones((self.rows + 2 * GUARD_ROWS, self.ld), bool)
        m[GUARD_ROWS:GUARD_ROWS + self.rows, self.col0:self.col0 + self.cols] = False
        return m


def row_scales(n):
    """powers of two cycling over 2**-6 .. 2**6"""
    return np.ldexp(1.0, (np.arange(n) % 13) - 6).astype(np.float32)


class Problem:
    """One GemmProblem: logical inputs (contiguous float32), their panels, and sentinel-filled output panels.

    regime "uniform": every input uniform in [-1, 1).  "scaled": the same data with the rows of Pop and Qop — the index p
    of the P operand and the index q of the Q operand, whichever axis of the stored matrix that is in the mode — and the
    bias (by p) multiplied by powers of two cycling over 2**-6 .. 2**6: output (q, p) is scaled by a power of two (exact),
    and the per-element bound has to hold on rows 2**12 smaller than their neighbours.
    pad: leading-dimension padding of every 2-D operand (0: dense).  col0 / panel_w (dgrad_narrow's addressing): P, C and
    mask sit at column col0 of a panel panel_w wide.  p_width: stored width of P's rows when it exceeds Kred (xcopy)."""

    def __init__(self, mode, Pdim, Qdim, Kred, seed, regime="uniform", pad=0, bq=None, bias=True, relu=1, mask=True,
                 db=True, partial=True, seed_w=False, dot_w=False, xcopy=None, col0=0, panel_w=None, p_width=None):
        self.mode, self.Pdim, self.Qdim, self.Kred = mode, Pdim, Qdim, Kred
        self.regime, self.relu, self.bq = regime, relu, bq
        rng = np.random.default_rng(seed)
        uni = lambda *shape: rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)
        sp, sq = row_scales(Pdim), row_scales(Qdim)
        if regime == "uniform":
            sp, sq = np.ones_like(sp), np.ones_like(sq)
        self.inp, self.out = {}, {}
        self.bias = self.mask = self.seed_w = self.dot_w = None
        self.xcopy_col, self.xcopy_n = 0, 0
        wide = (panel_w if panel_w is not None else Pdim + col0)
        if mode == FWD:
            pw = p_width if p_width is not None else Kred
            self.P = uni(Pdim, pw) * sp[:, None]
            self.Q = uni(Qdim, Kred) * sq[:, None]
            self.inp["P"] = Panel(Pdim, pw, pw + pad).put(self.P)
            self.inp["Q"] = Panel(Qdim, Kred, Kred + pad).put(self.Q)
            if bias:
                self.bias = uni(Pdim) * sp
                self.inp["bias"] = Panel(1, Pdim).put(self.bias)
            self.out["C"] = Panel(Qdim, Pdim, Pdim + pad)
            if seed_w:
                self.seed_w = uni(Pdim)
                self.inp["seed_w"] = Panel(1, Pdim).put(self.seed_w)
                self.out["C2"] = Panel(Qdim, Pdim, Pdim + pad)
            if dot_w:
                self.dot_w = uni(Pdim)
                self.inp["dot_w"] = Panel(1, Pdim).put(self.dot_w)
                self.out["dot_out"] = Panel(Qdim, Pdim // 16)
            if xcopy is not None:
                self.xcopy_col, self.xcopy_n = xcopy
                assert self.xcopy_col + self.xcopy_n <= pw
                self.out["xcopy_dst"] = Panel(self.xcopy_n, Pdim)
        elif mode == DGRAD:
            self.P = uni(Kred, Pdim) * sp[None, :]
            self.Q = uni(Qdim, Kred) * sq[:, None]
            self.inp["P"] = Panel(Kred, Pdim, wide + pad, col0).put(self.P)
            self.inp["Q"] = Panel(Qdim, Kred, Kred + pad).put(self.Q)
            if mask:
                self.mask = uni(Qdim, Pdim)
                self.inp["mask"] = Panel(Qdim, Pdim, wide + pad, col0).put(self.mask)
            self.out["C"] = Panel(Qdim, Pdim, wide + pad, col0)
        else:
            self.P = uni(Kred, Pdim) * sp[None, :]
            self.Q = uni(Kred, Qdim) * sq[None, :]
            self.inp["P"] = Panel(Kred, Pdim, Pdim + pad).put(self.P)
            self.inp["Q"] = Panel(Kred, Qdim, Qdim + pad).put(self.Q)
            self.out["C"] = Panel(Qdim, Pdim, Pdim + pad)
            if db:
                self.out["db"] = Panel(1, Qdim)
            if partial:
                self.out["partial"] = Panel(1, (Qdim // bq) * (Pdim // 64))
        self.ldp = self.inp["P"].ld
        self.ldq = self.inp["Q"].ld
        self.ldc = self.out["C"].ld
        self.ldm = self.inp["mask"].ld if "mask" in self.inp else 0

    @property
    def red(self):
        return self.Kred

    def reset_outputs(self):
        for p in self.out.values():
            p.reset()

    def snapshot(self):
        """bit image of every output buffer"""
        return {k: p.buf.view(np.uint32).copy() for k, p in self.out.items()}


def lrelu32(x):
    return np.maximum(x, np.float32(0)) + SLOPE32 * np.minimum(x, np.float32(0))


def float32_product(pr, P=None, Q=None):
    """The plain float32 CPU product of the same inputs (np.matmul on float32 arrays) with the epilogues in float32: the yardstick
    of the tight bound, and the stand-in for a correct kernel in the host test.  P / Q: substitutes for the problem's operands."""
    P = pr.P if P is None else np.asarray(P, np.float32)
    Q = pr.Q if Q is None else np.asarray(Q, np.float32)
    o = {}
    if pr.mode == FWD:
        y = np.matmul(Q, np.ascontiguousarray(P[:, :pr.Kred].T))
        if pr.bias is not None:
            y = y + pr.bias[None, :]
        if pr.relu:
            y = lrelu32(y)
        o["C"] = y.astype(np.float32)
        if pr.seed_w is not None:
            o["C2"] = (-pr.seed_w)[None, :] * np.where(o["C"] > 0, np.float32(1), SLOPE32)
        if pr.dot_w is not None:
            o["dot_out"] = (o["C"] * pr.dot_w[None, :]).reshape(pr.Qdim, pr.Pdim // 16, 16).sum(-1, dtype=np.float32)
        if pr.xcopy_n:
            o["xcopy_dst"] = np.ascontiguousarray(P[:, pr.xcopy_col:pr.xcopy_col + pr.xcopy_n].T)
    elif pr.mode == DGRAD:
        y = np.matmul(Q, P)
        if pr.mask is not None:
            y = y * np.where(pr.mask > 0, np.float32(1), SLOPE32)
        o["C"] = y.astype(np.float32)
    else:
        o["C"] = np.matmul(np.ascontiguousarray(Q.T), P).astype(np.float32)
        if "db" in pr.out:
            o["db"] = Q.sum(0, dtype=np.float32)
        if "partial" in pr.out:
            # per tile, as the kernels leave them: slot = tile_q * tiles_p + tile_p (db's squares in the tile_p == 0 slots)
            tq, tp = pr.Qdim // pr.bq, pr.Pdim // 64
            sq = (o["C"].astype(np.float64) ** 2).reshape(tq, pr.bq, tp, 64).sum((1, 3))
            if "db" in o:
                sq[:, 0] += (o["db"].astype(np.float64) ** 2).reshape(tq, pr.bq).sum(1)
            o["partial"] = sq.reshape(-1).astype(np.float32)
    return {k: np.asarray(v, np.float32) for k, v in o.items()}


def write_outputs(pr, outs):
    for k, v in outs.items():
        pr.out[k].put(v)


def reference(pr):
    """float64 results, the per-element magnitudes s, and (FWD) the float64 pre-activation"""
    P, Q = pr.P.astype(np.float64), pr.Q.astype(np.float64)
    r = {}
    if pr.mode == FWD:
        Pk = P[:, :pr.Kred]
        pre = Q @ Pk.T
        s = np.abs(Q) @ np.abs(Pk).T
        if pr.bias is not None:
            pre = pre + pr.bias.astype(np.float64)[None, :]
            s = s + np.abs(pr.bias.astype(np.float64))[None, :]
        r["pre"] = pre
        r["C"] = np.where(pre > 0, pre, SLOPE * pre) if pr.relu else pre
        r["s"] = s
    elif pr.mode == DGRAD:
        f = np.where(pr.mask > 0, 1.0, SLOPE) if pr.mask is not None else 1.0
        r["C"] = (Q @ P) * f
        r["s"] = (np.abs(Q) @ np.abs(P)) * f          # the mask factor is exact in the input: the error scales with it
    else:
        r["C"] = Q.T @ P
        r["s"] = np.abs(Q).T @ np.abs(P)
        r["db"] = Q.sum(0)
        r["s_db"] = np.abs(Q).sum(0)
    return r


def _first(bad):
    i = np.argwhere(bad)[0]
    return tuple(int(x) for x in i)


def check_finite(pr, tag=""):
    """1. every in-range element of every output is finite"""
    for name, panel in pr.out.items():
        bad = ~np.isfinite(panel.view())
        if bad.any():
            r, c = _first(bad)
            raise AssertionError(f"not finite: {tag} {name}[{r}][{c}] = {panel.view()[r, c]!r} "
                                 f"(bits {panel.view().view(np.uint32)[r, c]:#010x}); {int(bad.sum())} such elements")


def check_untouched(pr, tag=""):
    """2. every pad column and guard element is still the sentinel, bit for bit"""
    for name, panel in pr.out.items():
        bits = panel.buf.view(np.uint32).reshape(-1, panel.ld)
        bad = (bits != SENTINEL_BITS) & panel.outside()
        if bad.any():
            r, c = _first(bad)
            where = "guard row" if (r < GUARD_ROWS or r >= GUARD_ROWS + panel.rows) else "pad column"
            raise AssertionError(f"overwritten outside the output: {tag} {name} {where}, buffer row {r - GUARD_ROWS} col {c - panel.col0} "
                                 f"(bits {bits[r, c]:#010x}); {int(bad.sum())} such words")


def _check_bound(tag, name, got, ref, s, roundings):
    err = np.abs(got.astype(np.float64) - ref)
    bound = roundings * U * s
    bad = ~(err <= bound)
    if bad.any():
        r, c = _first(np.atleast_2d(bad))
        e, b = np.atleast_2d(err)[r, c], np.atleast_2d(bound)[r, c]
        raise AssertionError(f"outside the derived bound: {tag} {name}[{r}][{c}] = {np.atleast_2d(got)[r, c]!r}, reference "
                             f"{np.atleast_2d(ref)[r, c]!r}: |diff| {e:.3e} > ({roundings}) u s = {b:.3e}; {int(bad.sum())} such elements")
    with np.errstate(divide="ignore", invalid="ignore"):
        r_ = np.where(s > 0, err / (U * s), 0.0)
    return float(r_.max())


def check_values(pr, tag=""):
    """3. the elementwise bounds.  Returns {"kernel_r": max r of C, "yard_r": the float32 numpy product's, "branch_share": ...}."""
    ref = reference(pr)
    got = {k: p.view() for k, p in pr.out.items()}
    yard = float32_product(pr)
    red = pr.red
    stats = {}
    stats["kernel_r"] = _check_bound(tag, "C", got["C"], ref["C"], ref["s"], red + EXTRA_ROUNDINGS)
    stats["yard_r"] = _check_bound(tag + " (float32 numpy yardstick)", "C", yard["C"], ref["C"], ref["s"], red + EXTRA_ROUNDINGS)
    assert stats["kernel_r"] <= TIGHT_FACTOR * stats["yard_r"], (
        f"tight bound: {tag} kernel max r = {stats['kernel_r']:.3f} > {TIGHT_FACTOR} x yardstick max r = {stats['yard_r']:.3f} "
        f"(r = |y - ref| / (u s), reduction {red})")
    if "db" in got:
        stats["db_r"] = _check_bound(tag, "db", got["db"], ref["db"][None, :], ref["s_db"][None, :], red + EXTRA_ROUNDINGS)
    if "partial" in got:
        # The panel holds exactly tiles_q * tiles_p slots: that every one of them was written is check_finite's finding, that none
        # beyond them was is check_untouched's (the guard words around the panel).
        slots = got["partial"].astype(np.float64)
        e = (red + EXTRA_ROUNDINGS) * U * ref["s"]
        want = (ref["C"] ** 2).sum()
        slack = (2 * np.abs(ref["C"]) * e + e * e).sum()
        if "db" in got:
            e_db = (red + EXTRA_ROUNDINGS) * U * ref["s_db"]
            want += (ref["db"] ** 2).sum()
            slack += (2 * np.abs(ref["db"]) * e_db + e_db * e_db).sum()
        total = slots.sum()
        assert (slots >= 0).all(), f"negative sum-of-squares slot: {tag} partial[0][{_first(np.atleast_2d(slots < 0))[1]}]"
        assert abs(total - want) <= slack + PARTIAL_ROUNDINGS * U * want, (
            f"sum-of-squares partials: {tag} total of {slots.size} slots {total!r}, reference {want!r}, allowed {slack + PARTIAL_ROUNDINGS * U * want:.3e}")
    if "C2" in got:
        # lrelu' jumps at 0: elements whose float64 pre-activation lies within the derived bound of 0 may take either branch
        near = np.abs(ref["pre"]) <= (red + EXTRA_ROUNDINGS) * U * ref["s"]
        stats["branch_share"] = float(near.mean())
        assert stats["branch_share"] <= MAX_BRANCH_SHARE, (tag, "elements within the bound of the ReLU kink", stats["branch_share"])
        hi = np.broadcast_to((-pr.seed_w)[None, :], near.shape)
        lo = hi * SLOPE32                                             # the kernel's own single rounding
        want = np.where(ref["pre"] > 0, hi, lo)
        ok = (got["C2"] == want) | (near & ((got["C2"] == hi) | (got["C2"] == lo)))
        if not ok.all():
            r, c = _first(~ok)
            raise AssertionError(f"head seed: {tag} C2[{r}][{c}] = {got['C2'][r, c]!r}, expected {want[r, c]!r} "
                                 f"(pre-activation {ref['pre'][r, c]!r}); {int((~ok).sum())} such elements")
    if "dot_out" in got:
        dw = np.abs(pr.dot_w.astype(np.float64))[None, :]
        want = (ref["C"] * pr.dot_w.astype(np.float64)[None, :]).reshape(pr.Qdim, pr.Pdim // 16, 16).sum(-1)
        s_dot = (ref["s"] * dw).reshape(pr.Qdim, pr.Pdim // 16, 16).sum(-1)
        stats["dot_r"] = _check_bound(tag, "dot_out", got["dot_out"], want, s_dot, red + EXTRA_ROUNDINGS + DOT_ROUNDINGS)
    if "xcopy_dst" in got:
        want = float32_product(pr)["xcopy_dst"]
        bad = got["xcopy_dst"].view(np.uint32) != want.view(np.uint32)
        if bad.any():
            r, c = _first(bad)
            raise AssertionError(f"transposed copy: {tag} xcopy_dst[{r}][{c}] = {got['xcopy_dst'][r, c]!r}, expected P[{c}][{pr.xcopy_col + r}] = {want[r, c]!r}")
    return stats


# The problems test_gpu_gemm_forms.py runs with the head epilogues (seed_w / C2, dot_w / dot_out): (form id of dqnhip_internal.h, rows,
# outputs, K), one per forward form.  Kept here so that test_gemm_ref_host.py can confirm without a GPU, on exactly these seeds, that the
# reference alone puts fewer than MAX_BRANCH_SHARE of the pre-activations within the bound of the ReLU kink.
HEAD_CASES = [(0, 96, 128, 320), (1, 96, 128, 128), (2, 48, 128, 512), (3, 96, 64, 512), (4, 96, 128, 512), (5, 64, 192, 512)]


def head_problem(form, rows, outs, k, regime, pad):
    return Problem(FWD, outs, rows, k, seed=3000 + form, regime=regime, pad=pad, seed_w=True, dot_w=True)


def check(pr, tag=""):
    """The three assertions, in the order that names the most basic fault first."""
    check_finite(pr, tag)
    check_untouched(pr, tag)
    return check_values(pr, tag)
