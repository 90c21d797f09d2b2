"""Reference for the replay sweep's report (dqnhip_evaluate_memory / DQN.evaluate_memory()), numpy + math.fsum, no GPU.  Restated from
the description in include/dqnhip.h alone, not from the library's code.

Input: per-row float32 arrays over the WHOLE memory (logical order) — q, y, q_policy, mc, reward, terminal — the actor's outputs mu(s)
[N][10] and the stored actor outputs [N][10], plus the window (first, n) and the minibatch B.  Over the window's n rows:
  td = q - y and q_minus_mc = q - mc, one float32 subtraction each
  each of q, y, td, q_policy, mc, q_minus_mc, reward: min / max / sum / sum_sq over the finite values (min = max = 0 when none is
  finite; double sums of the exact double terms, a float's square being exact in double), n_nonfinite
  td_hist: diag_ref's exponent histogram of td (finite, non-zero values)
  n_terminal; n_action_match: GetAction's index — argmax over the four logits with logit 2 (TACKLE) replaced by -99999, the first
  maximum winning — agrees between mu(s) and the stored output
  n_chunks = ceil(n / B); pad rows of the last chunk are counted nowhere
The result has the shape of DQN.evaluate_memory().

compare(dev, ref)    diag_ref's rules: integers, bins, min and max exact; a double sum of n terms within 2 n 2^-53 sum |term| of the
                     fsum of the exact terms.

refreshed_leaf(td, eps, alpha)    what dqnhip_per_refresh stores for a finite td: float32((|td| + eps)^alpha) — the sum in float32,
                     the power by powf, which is not correctly rounded: leaf_matches allows 2 ulp of the float32 result around the
                     double-precision power of the float32 sum."""
import math

import numpy as np

import diag_ref as R

F = np.float32
QUANTITIES = ("q", "y", "td", "q_policy", "mc", "q_minus_mc", "reward")


def get_action(ao):
    """GetAction's index for every row of ao [N][>= 4]"""
    c = np.array(np.asarray(ao, F)[:, :4], F)
    c[:, 2] = F(-99999.0)
    best, bv = np.zeros(len(c), np.int64), c[:, 0].copy()
    for j in (1, 2, 3):
        with np.errstate(invalid="ignore"):
            up = c[:, j] > bv
        best[up] = j
        bv[up] = c[up, j]
    return best


def rows_of(q, y, q_policy, mc, reward, terminal, mu, stored):
    """the per-row quantities over whatever rows the arrays hold"""
    q, y, mc = np.asarray(q, F), np.asarray(y, F), np.asarray(mc, F)
    with np.errstate(all="ignore"):
        td, qmm = (q - y).astype(F), (q - mc).astype(F)
    return {"q": q, "y": y, "td": td, "q_policy": np.asarray(q_policy, F), "mc": mc, "q_minus_mc": qmm, "reward": np.asarray(reward, F),
            "terminal": np.asarray(terminal) != 0, "action_match": (get_action(mu) == get_action(stored)).astype(np.int32)}


def report(rows, first, n, B, iters=(0, 0)):
    """rows: rows_of(...) over the whole memory"""
    w = slice(first, first + n)
    out = {k: R.row_record(rows[k][w]) for k in QUANTITIES}
    out.update({"first": int(first), "n": int(n), "n_chunks": (n + B - 1) // B, "n_terminal": int(rows["terminal"][w].sum()),
                "n_action_match": int(rows["action_match"][w].sum()), "td_hist": R.histogram(rows["td"][w]),
                "actor_iter": int(iters[0]), "critic_iter": int(iters[1])})
    return out


def compare(dev, ref):
    """raises diag_ref.Mismatch naming the first field that is outside its bound"""
    for k in ("first", "n", "n_chunks", "n_terminal", "n_action_match", "actor_iter", "critic_iter"):
        R._exact(k, dev[k], ref[k])
    R._exact("td_hist", np.asarray(dev["td_hist"], np.int32), np.asarray(ref["td_hist"], np.int32))
    for k in QUANTITIES:
        d, r = dev[k], ref[k]
        for f in ("min", "max"):
            R._exact("%s.%s" % (k, f), F(d[f]), F(r[f]))
        R._exact("%s.n_nonfinite" % k, d["n_nonfinite"], r["n_nonfinite"])
        R._sum("%s.sum" % k, d["sum"], r["sum"], r["_n"], r["_abs"])
        R._sum("%s.sum_sq" % k, d["sum_sq"], r["sum_sq"], r["_n"], r["sum_sq"])


def refreshed_leaf(td, eps, alpha):
    """double-precision (|td| + eps)^alpha of the float32 sum, per element (td finite)"""
    s = (np.abs(np.asarray(td, F)) + F(eps)).astype(F)
    return np.ones(s.shape) if alpha == 0 else s.astype(np.float64) ** float(F(alpha))


def leaf_matches(leaf, td, eps, alpha, ulps=2):
    """per element: is the stored float32 leaf within `ulps` float32 steps of the correctly rounded power?  (positive floats order
    as their bit patterns: the distance in steps is the difference of the patterns)"""
    want = np.ascontiguousarray(refreshed_leaf(td, eps, alpha).astype(F))
    got = np.ascontiguousarray(np.asarray(leaf, F))
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)) <= ulps
