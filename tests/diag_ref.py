"""Reference for the update diagnostics (dqnhip_diag_collect / DQN.diagnostics()), numpy + math.fsum, no GPU.  The definitions are
restated here from their description alone, not from the library's code:

moments of a set x   count; n_zero (+-0); n_nonfinite (NaN, +-Inf); over the finite elements sum_abs = sum |x| and sum_sq = sum x^2
                     (double; a float's square is exact in double); max_abs as a float, 0 when no element is finite
exponent histogram   64 int32 bins over the finite non-zero elements: e = biased exponent field of the float32 bits (denormals
                     e = 0), bin = min(max(e - 87, 0), 63); sum of bins + n_zero + n_nonfinite = count
blobs                dense Caffe order: the actor's ip1 .. ipL, action_layer, actionpara_layer, then the critic's ip1 .. ipL,
                     q_values_layer, weight before bias; moments of w, of g (with its histogram), of lag = (double)w - (double)w'
                     (exact differences; max_abs rounded to float) and of step = s * (m / (sqrt(v) + delta)) in float32,
                     s = lr * float32(sqrt(1 - beta2^t) / (1 - beta1^t)), t the net's iteration; all zero while t == 0
panels               the stored post-ReLU values of pass p, layer i: moments, histogram, n_negative (x < 0), dead_units (columns
                     whose value is < 0 in every row)
rows                 q_target, y, q_train, q_policy, td = q_train - y (float32): min / max / sum / sum_sq over the finite values
                     (min = max = 0 when none is finite), n_nonfinite; n_terminal; per actor-output column min / max / sum over the
                     finite values and n_out_of_bounds against [-1, 1] (j < 4), [0, 100] (parameters 0 and 4), [-180, 180] (the
                     others), a NaN being outside; sum_abs / max_abs of the finite dq_da; prioritized: min / sum of the weights,
                     min of prob, max of td_abs
The result has the shape of DQN.diagnostics().

compare(dev, ref)    integers, bins, max_abs, min, max: exact.  A double sum of n terms: |dev - ref| <= 2 n 2^-53 sum |term|, ref the
                     fsum of the exact double terms — n - 1 double additions in whatever order, each within 2^-53 relative of a
                     partial sum that sum |term| bounds; the factor 2 covers the second-order terms and the reference's own final
                     rounding.  step: the per-element value passes through about nine float32 roundings (the correction's
                     conversion and product with lr, then sqrt, add, divide, multiply; a not-correctly-rounded sqrt / divide counts
                     as 2 each): 12 2^-24 relative on sum_abs and max_abs, twice that on sum_sq, plus the double bound."""
import math

import numpy as np

F = np.float32
BINS = 64
U53, U24 = 2.0 ** -53, 2.0 ** -24
ACTOR, CRITIC = 0, 1


# ---- the blob table ------------------------------------------------------------------------------------------------------------
def blob_table(S, hidden):
    """[{net, layer, is_bias, shape, offset, count}] — offset into the net's dense parameter vector"""
    out = []
    for net, in_dim, heads in ((ACTOR, S, (("action_layer", 4), ("actionpara_layer", 6))), (CRITIC, S + 10, (("q_values_layer", 1),))):
        off, k = 0, in_dim
        layers = [("ip%d_layer" % (i + 1), n) for i, n in enumerate(hidden)]
        for li, (name, n) in enumerate(layers + list(heads)):
            kk = k if li <= len(hidden) else hidden[-1]
            for is_bias, shape in ((False, (n, kk)), (True, (n,))):
                cnt = int(np.prod(shape))
                out.append({"net": net, "layer": name, "is_bias": is_bias, "shape": shape, "offset": off, "count": cnt})
                off += cnt
            if li < len(hidden):
                k = n
    return out


def param_count(S, hidden, net):
    """dqnhip_param_count's closed form"""
    k, total = (S if net == ACTOR else S + 10), 0
    for n in hidden:
        total += n * k + n
        k = n
    return total + (10 * k + 10 if net == ACTOR else k + 1)


# ---- moments, histogram -----------------------------------------------------------------------------------------------------------
def moments(x, as_float32_max=True):
    """x: float32 or float64 values (float64: exact differences).  Sums by fsum over the exact double terms."""
    x = np.asarray(x).ravel()
    x64 = x.astype(np.float64)
    fin = np.isfinite(x64)
    v = x64[fin & (x64 != 0)]
    a = np.abs(v)
    return {"count": int(x.size), "n_zero": int((x64 == 0).sum()), "n_nonfinite": int((~fin).sum()),
            "sum_abs": math.fsum(a), "sum_sq": math.fsum(v * v), "max_abs": float(F(a.max())) if a.size else 0.0}


def bin_of(x):
    """bin of ONE finite non-zero float32 value"""
    e = (int(np.array(x, F).view(np.uint32)) >> 23) & 0xFF
    return min(max(e - 87, 0), 63)


def histogram(x):
    x = np.ascontiguousarray(np.asarray(x, F).ravel())
    bits = x.view(np.uint32)
    e = ((bits >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64)
    keep = (e != 255) & ((bits & np.uint32(0x7FFFFFFF)) != 0)
    return np.bincount(np.clip(e[keep] - 87, 0, 63), minlength=BINS).astype(np.int32)


def adam_step(m, v, lr, beta1, beta2, delta, t):
    """the float32 expression, element for element"""
    m, v = np.asarray(m, F), np.asarray(v, F)
    if t == 0:
        return np.zeros(m.shape, F)
    b1, b2 = float(F(beta1)), float(F(beta2))
    s = F(lr) * F(math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))
    with np.errstate(all="ignore"):
        return (s * (m / (np.sqrt(v) + F(delta)))).astype(F)


def blob_record(entry, w, wt, g, m, v, lr, beta1, beta2, delta, t):
    with np.errstate(all="ignore"):
        lag = np.asarray(w, F).astype(np.float64) - np.asarray(wt, F).astype(np.float64)
    return {"net": entry["net"], "layer": entry["layer"], "is_bias": entry["is_bias"], "count": entry["count"],
            "w": moments(w), "g": moments(g), "lag": moments(lag), "step": moments(adam_step(m, v, lr, beta1, beta2, delta, t)),
            "g_hist": histogram(g)}


def panel_record(p, i, a):
    a = np.asarray(a, F)
    return {"pass": p, "layer": i, "rows": a.shape[0], "cols": a.shape[1], "a": moments(a), "hist": histogram(a),
            "n_negative": int((a < 0).sum()), "dead_units": int((a < 0).all(axis=0).sum())}


def row_record(x):
    x = np.asarray(x, F).ravel()
    v = x[np.isfinite(x)].astype(np.float64)
    return {"min": float(v.min()) if v.size else 0.0, "max": float(v.max()) if v.size else 0.0, "sum": math.fsum(v),
            "sum_sq": math.fsum(v * v), "n_nonfinite": int(x.size - v.size), "_n": int(v.size), "_abs": math.fsum(np.abs(v))}


def bounds(j):
    if j < 4:
        return -1.0, 1.0
    return (0.0, 100.0) if j - 4 in (0, 4) else (-180.0, 180.0)


def action_record(col, j):
    col = np.asarray(col, F)
    v = col[np.isfinite(col)].astype(np.float64)
    lo, hi = bounds(j)
    with np.errstate(invalid="ignore"):
        inside = (col >= F(lo)) & (col <= F(hi))
    return {"min": float(v.min()) if v.size else 0.0, "max": float(v.max()) if v.size else 0.0, "sum": math.fsum(v),
            "n_out_of_bounds": int((~inside).sum()), "_n": int(v.size), "_abs": math.fsum(np.abs(v))}


def reference(S, hidden, cfg, w, g, m, v, iters, panels, rows, per=None):
    """cfg: lr (actor, critic), beta1, beta2, delta, clip.  w[net] for the four nets, g / m / v[net] for the two online nets: dense
    vectors as get_params returns them.  iters: (actor, critic).  panels[(p, i)]: [B][width].  rows: q_target, y, q_train, q_policy,
    terminal, actor_out [B][10], dq_da [B][10].  per: None or {w, prob, td_abs}."""
    blobs = []
    for e in blob_table(S, hidden):
        n, sl = e["net"], slice(e["offset"], e["offset"] + e["count"])
        blobs.append(blob_record(e, w[n][sl], w[n + 2][sl], g[n][sl], m[n][sl], v[n][sl], cfg["lr"][n], cfg["beta1"], cfg["beta2"],
                                 cfg["delta"], iters[n]))
    out = {"blobs": blobs, "panels": [panel_record(p, i, panels[(p, i)]) for p in range(5) for i in range(1, len(hidden) + 1)]}
    with np.errstate(all="ignore"):
        td = np.asarray(rows["q_train"], F) - np.asarray(rows["y"], F)
    r = {k: row_record(rows[k]) for k in ("q_target", "y", "q_train", "q_policy")}
    r["td"] = row_record(td)
    r["n_terminal"] = int((np.asarray(rows["terminal"]) != 0).sum())
    r["actor_out"] = [action_record(np.asarray(rows["actor_out"])[:, j], j) for j in range(10)]
    d = np.asarray(rows["dq_da"], F).ravel()
    d = np.abs(d[np.isfinite(d)]).astype(np.float64)
    r["dq_da"] = {"sum_abs": math.fsum(d), "max_abs": float(d.max()) if d.size else 0.0, "_n": int(d.size)}
    if per is None:
        r["per"] = None
    else:
        fin = {k: np.asarray(per[k], F)[np.isfinite(np.asarray(per[k], F))].astype(np.float64) for k in ("w", "prob", "td_abs")}
        r["per"] = {"w_min": float(fin["w"].min()) if fin["w"].size else 0.0, "w_sum": math.fsum(fin["w"]),
                    "prob_min": float(fin["prob"].min()) if fin["prob"].size else 0.0,
                    "td_abs_max": float(fin["td_abs"].max()) if fin["td_abs"].size else 0.0, "_n": int(fin["w"].size)}
    out["rows"] = r
    out["has_per"] = per is not None
    out["actor_iter"], out["critic_iter"] = int(iters[0]), int(iters[1])
    out["grad_norm"], out["clip_scale"] = {}, {}
    for n in (ACTOR, CRITIC):
        norm = math.sqrt(math.fsum(b["g"]["sum_sq"] for b in blobs if b["net"] == n))
        out["grad_norm"][n] = norm
        out["clip_scale"][n] = cfg["clip"] / norm if cfg["clip"] >= 0 and norm > cfg["clip"] else 1.0
    return out


# ---- the comparator ----------------------------------------------------------------------------------------------------------
class Mismatch(AssertionError):
    pass


def _exact(where, dev, ref):
    if isinstance(ref, np.ndarray) or isinstance(dev, np.ndarray):
        if not np.array_equal(np.asarray(dev), np.asarray(ref)):
            raise Mismatch("%s: %s != %s" % (where, np.asarray(dev).tolist(), np.asarray(ref).tolist()))
    elif not (dev == ref):
        raise Mismatch("%s: %r != %r" % (where, dev, ref))


def _sum(where, dev, ref, n, sum_abs_terms, rel=0.0):
    """a double sum of n terms whose absolute values sum to sum_abs_terms; rel: an additional relative bound on the terms themselves"""
    bound = 2.0 * max(n, 1) * U53 * sum_abs_terms + rel * sum_abs_terms
    if not abs(dev - ref) <= bound:
        raise Mismatch("%s: |%r - %r| = %g > %g (n = %d)" % (where, dev, ref, abs(dev - ref), bound, n))


def compare_moments(where, dev, ref, step=False):
    for k in ("count", "n_zero", "n_nonfinite"):
        _exact(where + "." + k, dev[k], ref[k])
    n = ref["count"] - ref["n_zero"] - ref["n_nonfinite"]
    _sum(where + ".sum_abs", dev["sum_abs"], ref["sum_abs"], n, ref["sum_abs"], 12 * U24 if step else 0.0)
    _sum(where + ".sum_sq", dev["sum_sq"], ref["sum_sq"], n, ref["sum_sq"], 24 * U24 if step else 0.0)
    if step:
        if not abs(dev["max_abs"] - ref["max_abs"]) <= 12 * U24 * ref["max_abs"]:
            raise Mismatch("%s.max_abs: %r vs %r" % (where, dev["max_abs"], ref["max_abs"]))
    else:
        _exact(where + ".max_abs", F(dev["max_abs"]), F(ref["max_abs"]))


def compare(dev, ref):
    """raises Mismatch naming the first field that is outside its bound"""
    _exact("n_blobs", len(dev["blobs"]), len(ref["blobs"]))
    for i, (d, r) in enumerate(zip(dev["blobs"], ref["blobs"])):
        where = "blob %d (net %d %s %s)" % (i, r["net"], r["layer"], "bias" if r["is_bias"] else "weight")
        for k in ("net", "layer", "is_bias", "count"):
            _exact(where + "." + k, d[k], r[k])
        for k in ("w", "g", "lag"):
            compare_moments(where + "." + k, d[k], r[k])
        compare_moments(where + ".step", d["step"], r["step"], step=True)
        _exact(where + ".g_hist", d["g_hist"], r["g_hist"])
        if int(np.asarray(d["g_hist"]).sum()) + d["g"]["n_zero"] + d["g"]["n_nonfinite"] != d["g"]["count"]:
            raise Mismatch(where + ": bins + n_zero + n_nonfinite != count")
    _exact("n_panels", len(dev["panels"]), len(ref["panels"]))
    for d, r in zip(dev["panels"], ref["panels"]):
        where = "panel (pass %d, layer %d)" % (r["pass"], r["layer"])
        for k in ("pass", "layer", "rows", "cols", "n_negative", "dead_units"):
            _exact(where + "." + k, d[k], r[k])
        compare_moments(where + ".a", d["a"], r["a"])
        _exact(where + ".hist", d["hist"], r["hist"])
        if int(np.asarray(d["hist"]).sum()) + d["a"]["n_zero"] + d["a"]["n_nonfinite"] != d["a"]["count"]:
            raise Mismatch(where + ": bins + n_zero + n_nonfinite != count")
    dr, rr = dev["rows"], ref["rows"]
    for k in ("q_target", "y", "q_train", "q_policy", "td"):
        for f in ("min", "max"):
            _exact("rows.%s.%s" % (k, f), F(dr[k][f]), F(rr[k][f]))
        _exact("rows.%s.n_nonfinite" % k, dr[k]["n_nonfinite"], rr[k]["n_nonfinite"])
        _sum("rows.%s.sum" % k, dr[k]["sum"], rr[k]["sum"], rr[k]["_n"], rr[k]["_abs"])
        _sum("rows.%s.sum_sq" % k, dr[k]["sum_sq"], rr[k]["sum_sq"], rr[k]["_n"], rr[k]["sum_sq"])
    _exact("rows.n_terminal", dr["n_terminal"], rr["n_terminal"])
    for j, (d, r) in enumerate(zip(dr["actor_out"], rr["actor_out"])):
        for f in ("min", "max"):
            _exact("rows.actor_out[%d].%s" % (j, f), F(d[f]), F(r[f]))
        _exact("rows.actor_out[%d].n_out_of_bounds" % j, d["n_out_of_bounds"], r["n_out_of_bounds"])
        _sum("rows.actor_out[%d].sum" % j, d["sum"], r["sum"], r["_n"], r["_abs"])
    _exact("rows.dq_da.max_abs", F(dr["dq_da"]["max_abs"]), F(rr["dq_da"]["max_abs"]))
    _sum("rows.dq_da.sum_abs", dr["dq_da"]["sum_abs"], rr["dq_da"]["sum_abs"], rr["dq_da"]["_n"], rr["dq_da"]["sum_abs"])
    _exact("has_per", bool(dev["has_per"]), bool(ref["has_per"]))
    if ref["has_per"]:
        for f in ("w_min", "prob_min", "td_abs_max"):
            _exact("rows.per." + f, F(dr["per"][f]), F(rr["per"][f]))
        _sum("rows.per.w_sum", dr["per"]["w_sum"], rr["per"]["w_sum"], rr["per"]["_n"], rr["per"]["w_sum"])
    else:
        _exact("rows.per", dr["per"], None)
    for k in ("actor_iter", "critic_iter"):
        _exact(k, dev[k], ref[k])
    for n in (ACTOR, CRITIC):
        cnt = sum(b["count"] for b in ref["blobs"] if b["net"] == n)
        # the norm is the square root of a double sum of `cnt` terms: half the sum's relative bound, plus the root's and the quotient's roundings
        for k in ("grad_norm", "clip_scale"):
            if not abs(dev[k][n] - ref[k][n]) <= (cnt * U53 + 4 * U53) * abs(ref[k][n]):
                raise Mismatch("%s[%d]: %r vs %r" % (k, n, dev[k][n], ref[k][n]))
