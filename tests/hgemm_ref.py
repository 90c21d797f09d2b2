"""Float64 reference and per-element comparator for the fp16 launches of the learner (numpy only): the fp16-input /
fp32-accumulate GEMMs of dqn-hfo_amd/csrc/hgemm.hip.h with their epilogues, the bias-gradient column sums (Db16), the head's
weighted column sums (HeadWsum) and the fp32 -> fp16 glue (Cvt16).  The fp16 analogue of tests/gemm_ref.py, whose Panel idea,
sentinel word, u and TIGHT_FACTOR it reuses.

A `HProblem` is one HGemm, C[m][n] = sum_k Aop[m][k] Bop[n][k]:

    FWD    ta 0, tb 0   A stored [M][K], B stored [N][K]       bias + leaky ReLU -> C16 (+ seed_w / CS16, + C32)
    DGRAD  ta 0, tb 1   A stored [M][K], B stored [K][N]       ReLU' mask -> C16, or (layer 0) no mask, C32 * scale32
    WGRAD  ta 1, tb 1   A stored [K][M], B stored [K][N]       C32 * scale32 in columns < n_valid32, sumsq_partial per tile

Every operand lives in a `Panel`: a flat buffer with guard rows before and after and a pitch that may exceed the width,
everything prefilled with ONE NaN bit pattern (0x7FC0DEAD for fp32 words, 0x7DAD for fp16 halves) — inputs too, so that a read
outside an operand poisons the result and a write outside an output overwrites a sentinel.

Operands are drawn as float32, scaled, rounded to fp16; magnitudes below 2**-14 become 0, so that nothing rests on how the
MFMA treats subnormal fp16 inputs.  Regime "scaled": the rows of Aop (index m) and Bop (index n) and the bias (by n) are
multiplied by powers of two cycling over 2**-4 .. 2**4 (gemm_ref's 2**+-6 would overflow fp16).  A case whose reference plus
bound reaches 65504 is a wrong case, not a tolerance: assert_no_overflow().

Error model.  Every operand is exactly an fp16 value, every product is exact in fp32; the only errors are the fp32 accumulation
and the epilogue's roundings.  With u = 2**-24, s_ij = sum_k |a_ik| |b_jk| (+ |bias_j|) in float64 and f_ij the exact factor of
the activation (ReLU' of the mask: 1 or 0.01f; leaky output: 0.01f where the pre-activation lies below -b, 1 elsewhere),

    b_ij = (K + EXTRA_ROUNDINGS) u s_ij f_ij

    C32:   |got - ref scale32| <= b scale32                 columns >= n_valid32, pads and guards: the sentinel, in every row
    C16:   rne16(ref - b) <= got <= rne16(ref + b)          (rne16: float64 -> float32 -> float16 as numpy converts)
    CS16:  == fp16(((-seed_w[n]) * (C16_got[m][n] > 0 ? 1 : 0.01f)) * seed_scale) bit for bit, from the C16 the kernel wrote

and every element a second time with b replaced by TIGHT_FACTOR * yard_r * u s f, yard_r = the worst |y - ref| / (u s f) of the
plain float32 numpy product of the same fp16 operands with the epilogue in float32.  The C16 interval catches a second
rounding and truncation in place of round-to-nearest, and needs no separate rule for subnormal results.
"""
import zlib

import numpy as np

import gemm_ref as G

FWD, DGRAD, WGRAD = 0, 2, 3                  # hgemm_mode(): ta | tb << 1
U = G.U
SLOPE32 = G.SLOPE32
SLOPE = G.SLOPE
TIGHT_FACTOR = G.TIGHT_FACTOR
SENT32 = G.SENTINEL_BITS
SENT16 = np.uint16(0x7DAD)                   # an fp16 NaN (exponent all ones, mantissa 0x1AD) nothing computes by accident
GUARD_ROWS = G.GUARD_ROWS
FP16_MAX = 65504.0
# the epilogue's roundings on top of the K of the accumulation: bias add 1, leaky slope 1, ReLU' mask 1, the three additions of the
# <1,1> split-K merge (x0 + p1) + (p2 + p3) 3, scale32 1
EXTRA_ROUNDINGS = 7
# sum-of-squares slot of a tile: positive terms; per thread a chain of EIT * 8 <= 64 fma whose square is rounded with the sum (one
# rounding each), six wave-reduction levels, NW <= 8 additions over the waves: <= 78; the scaled value v * s itself is in b
PARTIAL_ROUNDINGS = 80
# Db16: the chain over the rows is counted by `rows`; the 32-row-group LDS reduction is part of it; + the multiplication by scale
DB_EXTRA = 2
# HeadWsum: one fma per row (counted by `rows`), the two-level LDS reduction is part of the same count; + nothing else; db: the
# six wave-reduction levels and three additions over the waves are additions of the same sum
HEAD_EXTRA = 2


# ---- panels -------------------------------------------------------------------------------------------------------------------------
class Panel:
    """A [rows][cols] operand of a [GUARD_ROWS + rows + GUARD_ROWS][ld] buffer of sentinels; dtype float32 or float16."""

    def __init__(self, rows, cols, ld=None, dtype=np.float32):
        self.rows, self.cols = int(rows), int(cols)
        self.ld = int(ld) if ld is not None else self.cols
        assert self.cols <= self.ld
        self.dtype = np.dtype(dtype)
        self.bits, self.sent = (np.uint16, SENT16) if self.dtype == np.float16 else (np.uint32, SENT32)
        self.raw = np.full((self.rows + 2 * GUARD_ROWS) * self.ld, self.sent, self.bits)
        self.offset = GUARD_ROWS * self.ld

    @property
    def buf(self):
        return self.raw.view(self.dtype)

    def view(self):
        return self.buf.reshape(-1, self.ld)[GUARD_ROWS:GUARD_ROWS + self.rows, :self.cols]

    def bitview(self):
        return self.raw.reshape(-1, self.ld)[GUARD_ROWS:GUARD_ROWS + self.rows, :self.cols]

    def put(self, a):
        self.view()[...] = np.asarray(a, self.dtype).reshape(self.rows, self.cols)
        return self

    def reset(self):
        self.raw[...] = self.sent

    def untouched(self):
        return bool((self.raw == self.sent).all())

    def outside(self):
        m = np.ones((self.rows + 2 * GUARD_ROWS, self.ld), bool)
        m[GUARD_ROWS:GUARD_ROWS + self.rows, :self.cols] = False
        return m


def row_scales(n, lo=-4):
    """powers of two cycling over 2**lo .. 2**(lo + 8)"""
    return np.ldexp(1.0, (np.arange(n) % 9) + lo).astype(np.float32)


def to16(x):
    """float32 -> fp16 (round to nearest), magnitudes below 2**-14 (the subnormal fp16 range) replaced by 0"""
    h = np.asarray(x, np.float32).astype(np.float16)
    h[np.abs(h.astype(np.float32)) < 2.0 ** -14] = 0
    return h


def rne16(x):
    """float64 -> float32 -> float16, as numpy converts (round to nearest even, subnormals kept), back as float64"""
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float16).astype(np.float64)


def _first(bad):
    return tuple(int(x) for x in np.argwhere(np.atleast_2d(bad))[0])


class _Case:
    """what HProblem and the riders share: sentinel-filled output panels, their bit image, the two structural checks"""
    inp = out = None

    def reset_outputs(self):
        for p in self.out.values():
            p.reset()

    def snapshot(self):
        return {k: p.raw.copy() for k, p in self.out.items()}

    def outputs_untouched(self):
        return all(p.untouched() for p in self.out.values())

    def check_finite(self, tag=""):
        """1. every in-range element of every output is finite (an unwritten element still holds the NaN it arrived with)"""
        for name, panel in self.out.items():
            bad = ~np.isfinite(panel.view().astype(np.float32))
            if bad.any():
                r, c = _first(bad)
                raise AssertionError(f"not finite: {tag} {name}[{r}][{c}] (bits {int(panel.bitview()[r, c]):#x}); {int(bad.sum())} such elements")

    def check_untouched(self, tag=""):
        """2. every pad column and guard element — for C32: every column at or beyond n_valid32 — is still the sentinel, in every row"""
        for name, panel in self.out.items():
            bits = panel.raw.reshape(-1, panel.ld)
            bad = (bits != panel.sent) & panel.outside()
            if bad.any():
                r, c = _first(bad)
                where = "guard row" if (r < GUARD_ROWS or r >= GUARD_ROWS + panel.rows) else "pad column"
                raise AssertionError(f"overwritten outside the output: {tag} {name} {where}, buffer row {r - GUARD_ROWS} col {c} "
                                     f"(bits {int(bits[r, c]):#x}); {int(bad.sum())} such words")

    def check(self, tag=""):
        self.check_finite(tag)
        self.check_untouched(tag)
        return self.check_values(tag)


def _bound32(tag, name, got, ref, bound, what):
    err = np.abs(np.asarray(got, np.float64) - ref)
    bad = ~(err <= bound)
    if bad.any():
        r, c = _first(bad)
        raise AssertionError(f"outside the {what} bound: {tag} {name}[{r}][{c}] = {np.atleast_2d(got)[r, c]!r}, reference {np.atleast_2d(ref)[r, c]!r}: "
                             f"|diff| {np.atleast_2d(err)[r, c]:.3e} > {np.atleast_2d(bound)[r, c]:.3e}; {int(bad.sum())} such elements")
    return err


def _interval16(tag, name, got16, ref, bound, what):
    got = got16.astype(np.float64)
    lo, hi = rne16(ref - bound), rne16(ref + bound)
    bad = ~((got >= lo) & (got <= hi))
    if bad.any():
        r, c = _first(bad)
        raise AssertionError(f"outside the {what} interval: {tag} {name}[{r}][{c}] = {got[r, c]!r} (bits {int(got16.view(np.uint16)[r, c]):#06x}), "
                             f"reference {ref[r, c]!r} +- {bound[r, c]:.3e} rounds to [{lo[r, c]!r}, {hi[r, c]!r}]; {int(bad.sum())} such elements")


def _dist16(got16, ref):
    """distance from ref to the set of reals that round to got16: the smallest error of the fp32 value the kernel can have had"""
    g = got16.astype(np.float64)
    up = np.nextafter(got16, np.float16(np.inf)).astype(np.float64)
    dn = np.nextafter(got16, np.float16(-np.inf)).astype(np.float64)
    return np.maximum(0.0, np.maximum((g + dn) / 2 - ref, ref - (g + up) / 2))


def _check_sumsq(tag, name, slots, want, slack):
    slots = np.asarray(slots, np.float64).reshape(-1)
    assert (slots >= 0).all(), f"negative sum-of-squares slot: {tag} {name}[{int(np.argmax(slots < 0))}]"
    total, allowed = slots.sum(), slack + PARTIAL_ROUNDINGS * U * want
    assert abs(total - want) <= allowed, f"sum-of-squares partials: {tag} {name}: total of {slots.size} slots {total!r}, reference {want!r}, allowed {allowed:.3e}"


# ---- one HGemm ------------------------------------------------------------------------------------------------------------------------
class HProblem(_Case):
    """One HGemm: logical fp16 operands Aop [M][K], Bop [N][K], their stored panels, sentinel-filled output panels.
    tile = (BM, BN) of the launch (the slot count of sumsq_partial).  pad: added to the pitch of every 2-D operand; the mask's pitch
    is 64 larger still, so that ldm != ldc16 always."""

    def __init__(self, kind, M, N, K, seed, regime="uniform", pad=0, tile=(64, 64), c16=True, c32=False, n_valid32=None, scale32=1.0,
                 bias=False, relu=0, mask=False, seed_w=False, seed_scale=256.0, sumsq=False):
        self.kind, self.M, self.N, self.K, self.tile = kind, M, N, K, tile
        self.ta, self.tb = kind & 1, (kind >> 1) & 1
        self.regime, self.pad, self.relu = regime, pad, int(relu)
        self.scale32, self.seed_scale = float(scale32), float(seed_scale)
        self.n_valid32 = int(n_valid32) if n_valid32 is not None else N
        rng = np.random.default_rng(seed)
        uni = lambda *shape: rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)
        sm, sn = (row_scales(M), row_scales(N)) if regime == "scaled" else (np.ones(M, np.float32), np.ones(N, np.float32))
        self.Aop = to16(uni(M, K) * sm[:, None])
        self.Bop = to16(uni(N, K) * sn[:, None])
        self.bias = uni(N) * sn if bias else None
        self.mask = to16(uni(M, N)) if mask else None
        self.seed_w = uni(N) if seed_w else None
        self.has = dict(C16=c16, C32=c32, CS16=seed_w, sumsq=sumsq)
        self.refresh()

    def refresh(self):
        """(re)build every panel from the logical operands; forget the cached reference"""
        M, N, K, pad = self.M, self.N, self.K, self.pad
        self._ref = self._yard = None
        self.inp, self.out = {}, {}
        A = self.Aop.T if self.ta else self.Aop
        B = self.Bop.T if self.tb else self.Bop
        self.inp["A"] = Panel(A.shape[0], A.shape[1], A.shape[1] + pad, np.float16).put(A)
        self.inp["B"] = Panel(B.shape[0], B.shape[1], B.shape[1] + pad, np.float16).put(B)
        if self.bias is not None:
            self.inp["bias"] = Panel(1, N).put(self.bias)
        if self.mask is not None:
            self.inp["mask"] = Panel(M, N, N + pad + 64, np.float16).put(self.mask)
        if self.seed_w is not None:
            self.inp["seed_w"] = Panel(1, N).put(self.seed_w)
        if self.has["C16"]:
            self.out["C16"] = Panel(M, N, N + pad, np.float16)
        if self.has["CS16"]:
            self.out["CS16"] = Panel(M, N, N + pad, np.float16)
        if self.has["C32"]:
            self.out["C32"] = Panel(M, self.n_valid32, N + pad)          # columns n_valid32 .. ld - 1 count as pad: sentinel in every row
        if self.has["sumsq"]:
            self.out["sumsq_partial"] = Panel(1, (M // self.tile[0]) * (N // self.tile[1]))

    def ld(self, name):
        p = self.inp.get(name) or self.out.get(name)
        return p.ld if p is not None else 0

    # -- float64 reference
    def reference(self):
        if self._ref is None:
            A, B = self.Aop.astype(np.float64), self.Bop.astype(np.float64)
            pre = A @ B.T
            s = np.abs(A) @ np.abs(B).T
            if self.bias is not None:
                pre = pre + self.bias.astype(np.float64)[None, :]
                s = s + np.abs(self.bias.astype(np.float64))[None, :]
            b0 = (self.K + EXTRA_ROUNDINGS) * U * s
            f, ref = np.ones_like(pre), pre
            if self.relu:
                f = np.where(pre < -b0, SLOPE, 1.0)
                ref = np.where(pre > 0, pre, SLOPE * pre)
            if self.mask is not None:
                fm = np.where(self.mask.astype(np.float32) > 0, 1.0, SLOPE)
                ref, f = ref * fm, f * fm
            self._ref = dict(pre=pre, ref=ref, s=s, f=f, b=b0 * f, usf=U * s * f)
        return self._ref

    # -- the float32 yardstick
    def cs16_from(self, c16):
        fac = np.where(np.asarray(c16, np.float16).astype(np.float32) > 0, np.float32(1), SLOPE32)
        return (((-self.seed_w)[None, :] * fac) * np.float32(self.seed_scale)).astype(np.float16)

    def float32_product(self, Aop=None, Bop=None):
        """the plain float32 numpy product of the same fp16 operands with the epilogue in float32: "y" (before any output rounding) and
        every output as a correct kernel would leave it.  Aop / Bop: substitutes for the operands."""
        A = (self.Aop if Aop is None else Aop).astype(np.float32)
        B = (self.Bop if Bop is None else Bop).astype(np.float32)
        y = np.matmul(A, np.ascontiguousarray(B.T))
        if self.bias is not None:
            y = y + self.bias[None, :]
        if self.relu:
            y = G.lrelu32(y)
        if self.mask is not None:
            y = y * np.where(self.mask.astype(np.float32) > 0, np.float32(1), SLOPE32)
        y = y.astype(np.float32)
        o = {"y": y}
        if self.has["C16"]:
            o["C16"] = y.astype(np.float16)
        if self.has["CS16"]:
            o["CS16"] = self.cs16_from(o["C16"])
        if self.has["C32"]:
            o["C32"] = (y * np.float32(self.scale32))[:, :self.n_valid32]
        if self.has["sumsq"]:
            bm, bn = self.tile
            sq = np.zeros((self.M, self.N))
            sq[:, :self.n_valid32] = o["C32"].astype(np.float64) ** 2
            o["sumsq_partial"] = sq.reshape(self.M // bm, bm, self.N // bn, bn).sum((1, 3)).reshape(-1).astype(np.float32)
        return o

    def write_outputs(self, outs):
        for k, p in self.out.items():
            p.put(outs[k])

    def yardstick_r(self):
        if self._yard is None:
            r = self.reference()
            self._yard = float((np.abs(self.float32_product()["y"].astype(np.float64) - r["ref"]) / r["usf"]).max())
        return self._yard

    def assert_no_overflow(self, tag=""):
        r = self.reference()
        top = float((np.abs(r["ref"]) + r["b"]).max())
        assert top < FP16_MAX, f"{tag}: reference + bound reaches {top!r}: fp16 would overflow — a wrong case, not a tolerance"
        assert (r["usf"] > 0).all(), f"{tag}: an element without magnitude"

    def check_values(self, tag=""):
        """3. the per-element rules.  Returns {"yard_r", "kernel_r" (C32: measured; C16 only: the smallest r consistent with the fp16 values)}."""
        self.assert_no_overflow(tag)
        r = self.reference()
        ref, b, usf = r["ref"], r["b"], r["usf"]
        yard_r = self.yardstick_r()
        bt = TIGHT_FACTOR * yard_r * usf
        st = {"yard_r": yard_r}
        tight = f"tight ({TIGHT_FACTOR} x yardstick max r {yard_r:.3f}, r = |y - ref| / (u s f), K {self.K})"
        if "C32" in self.out:
            nv, sc = self.n_valid32, self.scale32
            got = self.out["C32"].view()
            err = _bound32(tag, "C32", got, ref[:, :nv] * sc, b[:, :nv] * sc, "derived")
            st["kernel_r"] = float((err / (usf[:, :nv] * sc)).max())
            _bound32(tag, "C32", got, ref[:, :nv] * sc, bt[:, :nv] * sc, tight)
        if "C16" in self.out:
            got16 = self.out["C16"].view()
            _interval16(tag, "C16", got16, ref, b, "derived")
            st["kernel_r16"] = float((_dist16(got16, ref) / usf).max())
            st.setdefault("kernel_r", st["kernel_r16"])
            _interval16(tag, "C16", got16, ref, bt, tight)
        if "CS16" in self.out:
            want = self.cs16_from(self.out["C16"].view()).view(np.uint16)
            got = self.out["CS16"].bitview()
            bad = got != want
            if bad.any():
                i, j = _first(bad)
                raise AssertionError(f"head seed: {tag} CS16[{i}][{j}] bits {int(got[i, j]):#06x}, expected {int(want[i, j]):#06x} from the written "
                                     f"C16[{i}][{j}] = {self.out['C16'].view()[i, j]!r} (float64 pre-activation {r['pre'][i, j]!r}); {int(bad.sum())} such elements")
        if "sumsq_partial" in self.out:
            nv, sc = self.n_valid32, self.scale32
            e, a = b[:, :nv] * sc, np.abs(ref[:, :nv]) * sc
            _check_sumsq(tag, "sumsq_partial", self.out["sumsq_partial"].view(), (a * a).sum(), (2 * a * e + e * e).sum())
        return st


# ---- riders -------------------------------------------------------------------------------------------------------------------------
class DbRider(_Case):
    """Db16Batch: db_l[n] = scale * sum_b dY_l[b][n] for layers of widths `widths`, one sum-of-squares slot per 64-column block."""

    def __init__(self, rows, widths, seed, regime="uniform", pad=0, scale=1.0 / 4096, sumsq=True):
        self.rows, self.widths, self.scale = rows, list(widths), float(scale)
        rng = np.random.default_rng(seed)
        self.dy = [to16(rng.uniform(-1.0, 1.0, size=(rows, w)).astype(np.float32) * (row_scales(w)[None, :] if regime == "scaled" else np.float32(1)))
                   for w in self.widths]
        self.inp = {f"dy{i}": Panel(rows, w, w + pad, np.float16).put(d) for i, (w, d) in enumerate(zip(self.widths, self.dy))}
        self.out = {f"db{i}": Panel(1, w) for i, w in enumerate(self.widths)}
        self.blocks = sum(w // 64 for w in self.widths)
        if sumsq:
            self.out["db_sumsq"] = Panel(1, self.blocks)

    def float32_outputs(self):
        o = {f"db{i}": d.astype(np.float32).sum(0, dtype=np.float32) * np.float32(self.scale) for i, d in enumerate(self.dy)}
        if "db_sumsq" in self.out:
            o["db_sumsq"] = np.concatenate([(o[f"db{i}"].astype(np.float64) ** 2).reshape(-1, 64).sum(1) for i in range(len(self.dy))]).astype(np.float32)
        return o

    def write_outputs(self, outs):
        for k, p in self.out.items():
            p.put(outs[k])

    def check_values(self, tag=""):
        worst, blk = 0.0, 0
        for i, d in enumerate(self.dy):
            d64 = d.astype(np.float64)
            ref, s = self.scale * d64.sum(0)[None, :], self.scale * np.abs(d64).sum(0)[None, :]
            bound = (self.rows + DB_EXTRA) * U * s
            err = _bound32(tag, f"db{i}", self.out[f"db{i}"].view(), ref, bound, "derived")
            worst = max(worst, float((err / (U * s)).max()))
            if "db_sumsq" in self.out:      # slot order: the layers' 64-column blocks one after the other (Db16::row_base)
                slots = self.out["db_sumsq"].view()[0]
                for c in range(self.widths[i] // 64):
                    a, e = np.abs(ref[0, c * 64:(c + 1) * 64]), bound[0, c * 64:(c + 1) * 64]
                    _check_sumsq(tag, f"db_sumsq[{blk}] (layer {i} columns {c * 64}..)", slots[blk:blk + 1], (a * a).sum(), (2 * a * e + e * e).sum())
                    blk += 1
        return {"db_r": worst}


class HeadRider(_Case):
    """HeadWsum: dW[j][k] = sum_m dy[m][j] X16[m][k], db[j] = sum_m dy[m][j]; nh = 1 (lddy 1) or 10 (lddy 16: columns nh .. 15 of a dy
    row hold the sentinel — the kernel may load them, it must not use them); one sum-of-squares slot per 64-column block."""

    def __init__(self, rows, H, nh, seed, regime="uniform", partial=True):
        assert nh in (1, 10)
        self.rows, self.H, self.nh, self.lddy = rows, H, nh, (1 if nh == 1 else 16)
        rng = np.random.default_rng(seed)
        sc = row_scales(rows)[:, None] if regime == "scaled" else np.float32(1)
        self.dy = (rng.uniform(-1.0, 1.0, size=(rows, nh)).astype(np.float32) * sc).astype(np.float32)
        self.X = to16(rng.uniform(-1.0, 1.0, size=(rows, H)).astype(np.float32) * (row_scales(H)[None, :] if regime == "scaled" else np.float32(1)))
        self.inp = {"dy": Panel(rows, nh, self.lddy).put(self.dy), "X16": Panel(rows, H, H, np.float16).put(self.X)}
        self.out = {"dW": Panel(nh, H), "hdb": Panel(1, nh)}
        if partial:
            self.out["partial"] = Panel(1, H // 64)

    def float32_outputs(self, dy=None):
        dy = self.dy if dy is None else dy
        o = {"dW": np.matmul(np.ascontiguousarray(dy.T), self.X.astype(np.float32)).astype(np.float32), "hdb": dy.sum(0, dtype=np.float32)}
        if "partial" in self.out:
            sq = (o["dW"].astype(np.float64) ** 2).reshape(self.nh, -1, 64).sum((0, 2))
            sq[0] += (o["hdb"].astype(np.float64) ** 2).sum()
            o["partial"] = sq.astype(np.float32)
        return o

    def write_outputs(self, outs):
        for k, p in self.out.items():
            p.put(outs[k])

    def check_values(self, tag=""):
        dy, X = self.dy.astype(np.float64), self.X.astype(np.float64)
        ref, s = dy.T @ X, np.abs(dy).T @ np.abs(X)
        bound = (self.rows + HEAD_EXTRA) * U * s
        err = _bound32(tag, "dW", self.out["dW"].view(), ref, bound, "derived")
        rdb, sdb = dy.sum(0)[None, :], np.abs(dy).sum(0)[None, :]
        bdb = (self.rows + HEAD_EXTRA) * U * sdb
        _bound32(tag, "hdb", self.out["hdb"].view(), rdb, bdb, "derived")
        if "partial" in self.out:
            want = (ref ** 2).sum() + (rdb ** 2).sum()
            slack = (2 * np.abs(ref) * bound + bound ** 2).sum() + (2 * np.abs(rdb) * bdb + bdb ** 2).sum()
            _check_sumsq(tag, "partial", self.out["partial"].view(), want, slack)
        return {"head_r": float((err / (U * s)).max())}


class CvtRider(_Case):
    """Cvt16Batch as the learner fills it (no transposed output): dst [rows][ld16] = fp16(src [rows][cols] * scale), columns cols .. ld16 - 1
    exactly +0.  entries: (rows, cols, ld16, scale).  Regime "scaled": rows times 2**-8 .. 2**0 (with scale 4096 the largest product stays
    below 65504; the smallest land in the subnormal fp16 range, which the conversion keeps)."""

    def __init__(self, entries, seed, regime="uniform", pad=0):
        rng = np.random.default_rng(seed)
        self.entries = list(entries)
        self.src, self.inp, self.out = [], {}, {}
        for i, (rows, cols, ld16, scale) in enumerate(self.entries):
            sc = row_scales(rows, -8)[:, None] if regime == "scaled" else np.float32(1)
            x = (rng.uniform(-1.0, 1.0, size=(rows, cols)).astype(np.float32) * sc).astype(np.float32)
            self.src.append(x)
            self.inp[f"src{i}"] = Panel(rows, cols, cols + pad).put(x)
            self.out[f"dst{i}"] = Panel(rows, ld16, ld16, np.float16)

    def float32_outputs(self):
        o = {}
        for i, (rows, cols, ld16, scale) in enumerate(self.entries):
            d = np.zeros((rows, ld16), np.float16)
            d[:, :cols] = (self.src[i] * np.float32(scale)).astype(np.float16)
            o[f"dst{i}"] = d
        return o

    def write_outputs(self, outs):
        for k, p in self.out.items():
            p.put(outs[k])

    def check_finite(self, tag=""):
        pass                                 # bit-exact below: an unwritten element differs from its expected bits

    def check_values(self, tag=""):
        want = self.float32_outputs()
        for i, (rows, cols, ld16, scale) in enumerate(self.entries):
            got, w = self.out[f"dst{i}"].bitview(), want[f"dst{i}"].view(np.uint16)
            bad = got != w
            if bad.any():
                r, c = _first(bad)
                what = "pad column (must be +0)" if c >= cols else f"fp16(src * {scale})"
                raise AssertionError(f"cvt16: {tag} dst{i}[{r}][{c}] bits {int(got[r, c]):#06x}, expected {int(w[r, c]):#06x}: {what}; {int(bad.sum())} such elements")
        return {}


# ---- forms and case lists (shared by tests/test_hgemm_ref_host.py and tests/test_gpu_hgemm_forms.py: same shapes, same seeds) --------------
(NT_BIG_FWD, NT_BIG_DGRAD, NT_BIG_WGRAD, NT_SMALL_FWD, NT_SMALL_DGRAD, NT_SMALL_WGRAD, NT_SMALL_BWD, NT_HUGE_FWD,
 GROUP_DB_BIG, GROUP_DB_SMALL, DB16_COLS, CVT16) = range(12)                 # dqnhip_internal.h DQNHIP_HFORM_*
FORM_NAME = ["hgemm_nt<2,2,0,0>", "hgemm_nt<2,2,2,2>", "hgemm_nt<2,2,3,3>", "hgemm_nt<1,1,0,0>", "hgemm_nt<1,1,2,2>", "hgemm_nt<1,1,3,3>",
             "hgemm_nt<1,1,2,3>", "hgemm_nt<4,2,0,0>", "hgemm_group_db<2,2>", "hgemm_group_db<1,1>", "k_db16_cols", "k_cvt16"]
TILE = {NT_BIG_FWD: (128, 128), NT_BIG_DGRAD: (128, 128), NT_BIG_WGRAD: (128, 128), NT_SMALL_FWD: (64, 64), NT_SMALL_DGRAD: (64, 64),
        NT_SMALL_WGRAD: (64, 64), NT_SMALL_BWD: (64, 64), NT_HUGE_FWD: (256, 128), GROUP_DB_BIG: (128, 128), GROUP_DB_SMALL: (64, 64)}
PADS = [0, 64]
REGIMES = ["uniform", "scaled"]
LOSS_SCALE = 4096.0


def seed_of(name):
    return zlib.crc32(name.encode())


# pre-activations of the "kink" variant's row 0 (a zero row of A: the bias alone): positive, and all but the last round to fp16 zero
# (2**-25 = 2.98e-8 is half the smallest fp16 subnormal), so that C16 > 0 and the fp32 value > 0 disagree on them
KINK_BIAS = np.array([1e-8, 2e-8, 2.5e-8, 4e-8], np.float32)


def make(form, kind, M, N, K, regime, pad, variant="", l0=False, kink=False, **kw):
    """the problem of a case: the epilogue of its orientation as the learner builds it (fwd16_problem, tower_backward16).  kink: row 0
    of A is zero and the first bias values are KINK_BIAS — CS16 must follow the sign of the fp16 value the kernel stored"""
    tile = TILE[form]
    name = f"{form}-{kind}-{M}x{N}x{K}-{variant}"
    base = dict(seed=seed_of(name), regime=regime, pad=pad, tile=tile)
    if kind == FWD:            # bias + leaky ReLU -> C16
        base.update(bias=True, relu=1, c16=True)
    elif l0:                   # layer 0's input gradient: no mask, C32 only, loss scale removed
        base.update(c16=False, c32=True, scale32=1.0 / LOSS_SCALE)
    elif kind == DGRAD:        # ReLU' mask -> C16
        base.update(mask=True, c16=True)
    else:                      # wgrad: C32 with the loss scale removed, the clip norm's partial sums
        base.update(c16=False, c32=True, scale32=1.0 / LOSS_SCALE, sumsq=True)
    base.update(kw)
    pr = HProblem(kind, M, N, K, **base)
    if kink:
        pr.Aop[0, :] = 0
        pr.bias[:KINK_BIAS.size] = KINK_BIAS
        pr.refresh()
    return pr


# K lists from the ring of hgemm_body (prologue STAGES - 1 stages, steady loop while kt + STAGES - 1 < nk, then the drain; a stage
# buffer is first reused at kt = STAGES):
#   <2,2> KSTEP 64, 4 stages: 64, 128, 192 (prologue full, no steady trip), 256 (one trip), 320 (two trips, first buffer reuse), 576 (reused twice)
#   <1,1> KSTEP 128, 4 stages: 128, 256, 384, 512, 640, 1152       <4,2> KSTEP 64, 3 stages: 64, 128, 192, 256, 448
# M, N: <2,2> {128, 256, 384} (+ 3 x 5 and 2 x 4 tiles: hg_tile_of_block's remainder branch / a multiple of 8), <1,1> {64, 128, 192}
# (+ 3 x 5, 2 x 4), <4,2> M {256, 512}, N {128, 256} (+ 768 x 640 = 3 x 5, 512 x 512 = 2 x 4)
BIG_SHAPES = [(128, 128, 64), (256, 384, 128), (384, 128, 192), (128, 256, 256), (256, 256, 320), (384, 384, 576), (384, 640, 64), (256, 512, 64)]
SMALL_SHAPES = [(64, 64, 128), (128, 192, 256), (192, 64, 384), (64, 128, 512), (128, 128, 640), (192, 192, 1152), (192, 320, 128), (128, 256, 128)]
HUGE_SHAPES = [(256, 128, 64), (512, 256, 128), (256, 256, 192), (512, 128, 256), (256, 128, 448), (768, 640, 64), (512, 512, 64)]


def single_cases():
    """(id, form, fn(regime, pad) -> [HProblem]) of every single-problem launch"""
    out = []

    def add(form, kind, M, N, K, variant="", **kw):
        out.append((f"{FORM_NAME[form]}-{M}x{N}x{K}" + (f"-{variant}" if variant else ""), form,
                    lambda regime, pad: [make(form, kind, M, N, K, regime, pad, variant, **kw)]))

    for forms, shapes in (((NT_BIG_FWD, NT_BIG_DGRAD, NT_BIG_WGRAD), BIG_SHAPES), ((NT_SMALL_FWD, NT_SMALL_DGRAD, NT_SMALL_WGRAD), SMALL_SHAPES)):
        f_fwd, f_dg, f_wg = forms
        bn = TILE[f_fwd][1]
        for i, (M, N, K) in enumerate(shapes):
            add(f_fwd, FWD, M, N, K)
            add(f_dg, DGRAD, M, N, K)                                   # mask -> C16, ldm != ldc16
            add(f_wg, WGRAD, M, N, K)                                   # n_valid32 = N
        M, N, K = shapes[1]
        add(f_fwd, FWD, M, N, K, "seed", seed_w=True)                   # the critic(s, mu(s)) pass's top layer: seed_w / CS16
        add(f_fwd, FWD, M, N, K, "c16c32", c32=True)                    # C16 and C32 together
        add(f_fwd, FWD, *shapes[4], "seed", seed_w=True)
        add(f_fwd, FWD, *shapes[0], "seedkink", seed_w=True, kink=True)  # elements whose positive fp32 value rounds to fp16 zero
        for (M, N, K) in (shapes[0], shapes[3], shapes[5]):
            add(f_dg, DGRAD, M, N, K, "l0", l0=True)                    # no mask, C32 only, scale32 = 1 / 4096
        for (M, N, K) in (shapes[1], shapes[4]):
            add(f_wg, WGRAD, M, N, K, "nv", n_valid32=N - 64)           # columns beyond n_valid32 stay untouched
    # wgrad grids hg_tile_2d accepts ((tiles_m / 2) * (tiles_n / 4) % 8 == 0), K at its smallest; every other wgrad grid above is one it refuses
    add(NT_BIG_WGRAD, WGRAD, 512, 2048, 64, "2d")
    add(NT_SMALL_WGRAD, WGRAD, 256, 1024, 128, "2d")
    for (M, N, K) in HUGE_SHAPES:
        add(NT_HUGE_FWD, FWD, M, N, K)
    add(NT_HUGE_FWD, FWD, 512, 256, 128, "seed", seed_w=True)
    add(NT_HUGE_FWD, FWD, 256, 128, 64, "seedkink", seed_w=True, kink=True)
    add(NT_HUGE_FWD, FWD, 256, 256, 192, "c16c32", c32=True)
    return out


def grouped_cases():
    """(id, form, fn(regime, pad) -> [HProblem]): 2, 3 and 4 problems of DIFFERENT shapes in one launch (tile_end), the learner's pairs"""
    out = []

    def add(name, form, specs):
        out.append((f"{FORM_NAME[form]}-{name}", form,
                    lambda regime, pad: [make(form, kind, M, N, K, regime, pad, f"{name}{i}{v}", **kw) for i, (kind, M, N, K, v, kw) in enumerate(specs)]))

    for (f_fwd, f_dg, f_wg), sh in (((NT_BIG_FWD, NT_BIG_DGRAD, NT_BIG_WGRAD), BIG_SHAPES), ((NT_SMALL_FWD, NT_SMALL_DGRAD, NT_SMALL_WGRAD), SMALL_SHAPES)):
        for n in (2, 3, 4):
            pick = [sh[1], sh[0], sh[4], sh[2]][:n]
            add(f"g{n}", f_fwd, [(FWD, M, N, K, "", dict(seed_w=(i == 1))) for i, (M, N, K) in enumerate(pick)])
            add(f"g{n}", f_dg, [(DGRAD, M, N, K, "", dict(l0=(i == 2))) for i, (M, N, K) in enumerate(pick)])
            add(f"g{n}", f_wg, [(WGRAD, M, N, K, "", dict(n_valid32=N - 64) if i == 1 and N > 64 else {}) for i, (M, N, K) in enumerate(pick)])
    # tower_backward16's per-layer pair: dgrad (rows, k_in, n_out) and wgrad (n_out, k_in, rows) share dY; once the dgrad has more tiles, once the wgrad
    add("pair-nd12-nw6", NT_SMALL_BWD, [(DGRAD, 256, 192, 128, "", {}), (WGRAD, 128, 192, 256, "", {})])
    add("pair-nd4-nw12", NT_SMALL_BWD, [(DGRAD, 128, 128, 256, "", {}), (WGRAD, 256, 192, 128, "", {})])
    add("pair-l0", NT_SMALL_BWD, [(DGRAD, 128, 128, 384, "", dict(l0=True)), (WGRAD, 384, 128, 128, "", {})])
    # tower_forward16_pair: the online and the target net's same layer
    add("pair", NT_HUGE_FWD, [(FWD, 512, 256, 128, "", {}), (FWD, 512, 256, 128, "", {})])
    add("g3", NT_HUGE_FWD, [(FWD, 256, 128, 192, "", {}), (FWD, 512, 128, 64, "", {}), (FWD, 256, 256, 448, "", {})])
    return out


# hgemm_group_db: rows -> (wgrad shapes as (M = n_out, N = k_in) in units of the tile, column-sum layer widths, H of the head rider).
# head_wsum_block takes 256 rows per trip for nh = 1 and 128 for nh = 10, then 32-row steps; db16_cols_block 128 per trip, then 32-row
# steps: rows 128 / 256 / 384 / 640 = (tail only | one trip), (one | two), (trip + tail | three), (two + tail | five).
GROUP_ROWS = {128: ([(1, 2)], [128], 64), 256: ([(1, 1), (2, 1), (1, 3)], [128, 256, 64, 192], 192),
              384: ([(2, 2), (1, 1), (3, 1), (1, 2)], [64, 128, 192, 256], 64), 640: ([(2, 1)], [192, 64, 128, 64], 192)}
GROUP_CASES = [(form, rows, nh) for form in (GROUP_DB_BIG, GROUP_DB_SMALL) for rows in GROUP_ROWS for nh in (1, 10)] + \
              [(GROUP_DB_BIG, 256, 0), (GROUP_DB_SMALL, 256, 0)]


def group_case(form, rows, nh, regime, pad):
    """-> (wgrads, DbRider, HeadRider or None)"""
    shapes, widths, H = GROUP_ROWS[rows]
    t = TILE[form][0]
    name = f"group-{form}-{rows}-{nh}"
    wg = [make(form, WGRAD, m * t, n * t, rows, regime, pad, f"{name}-{i}") for i, (m, n) in enumerate(shapes)]
    db = DbRider(rows, widths, seed_of(name + "-db"), regime, pad)
    head = HeadRider(rows, H, nh, seed_of(name + "-head"), regime) if nh else None
    return wg, db, head


DB16_ROWS = [64, 128, 192, 256, 384, 640]      # db16_cols_block alone: tail steps only (64), one trip, trip + tail, two, three, five trips
DB16_WIDTHS = [[128], [192, 64, 128, 256]]


def db16_case(rows, widths, regime, pad):
    return DbRider(rows, widths, seed_of(f"db16-{rows}-{len(widths)}"), regime, pad)


# three entries of different shapes: 68 of 128 columns (the critic's first panel) with the loss scale, cols == ld16 at scale 1, and rows
# that end inside a 64-row tile
CVT_ENTRIES = [(128, 68, 128, 4096.0), (192, 192, 192, 1.0), (96, 100, 128, 1.0)]


def cvt_case(regime, pad):
    return CvtRider(CVT_ENTRIES, seed_of("cvt16"), regime, pad)
