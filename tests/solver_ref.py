"""Float64 reference and per-element comparator for the optimiser pass of every solver (numpy only; imports nothing of the package).

Adam is tests/adam_ref.py, unchanged: `reference` and `check` here delegate to it.  The other five are the rules of
dqn-hfo_amd/csrc/solver_bodies.hip.h (sgd_step .. adadelta_step, carried by k_solver_soft<> / k_solver_soft_gather<>), in the float32
expression order include/dqnhip.h fixes.  A test snapshots before = (w, h, h2, wt) — adam_ref.State, h / h2 = history 1 / 2 =
DQNHIP_KIND_M / KIND_V — runs an update, reads the gradient the pass consumed and the state after, and calls `check`.

Constants as the kernel forms them: lr, mom, delta, rho, tau, clip are float32 values; c1 = fl32(1 + mom), omm = fl32(1 - mom),
omr = fl32(1 - rho), omt = fl32(1 - tau) are float32 operations whose RESULT the reference takes as the constant (as adam_ref does with
omb1, omb2).  There is no bias correction and no use of the iteration.  s_ref = clip / ||g|| when clip >= 0 and ||g|| > clip, else 1.

THE RULES, per element, every operation one float32 rounding of relative size u = 2**-24 (fmaf one; sqrtf and / one each: hipcc's
default is the correctly rounded pair; contraction is off inside the rules, so no other fusing happens):

    gs = fl(g * s)                                              all solvers (exact when s == 1)
    SGD       h1 = fma(lr, gs, fl(mom h0));                                     w1 = fl(w0 - h1)
    Nesterov  h1 as SGD;  un = fma(c1, h1, -fl(mom h0));                        w1 = fl(w0 - un)
    AdaGrad   h1 = fma(gs, gs, h0);  den = fl(fl(sqrt(h1)) + delta);            w1 = fl(w0 - fl(lr fl(gs / den)))
    RMSProp   h1 = fma(omr, fl(gs gs), fl(rho h0));  den as AdaGrad;            w1 likewise
    AdaDelta  h1 = fma(omm, fl(gs gs), fl(mom h0));  a = fl(h2 + delta);  b = fl(h1 + delta);
              un = fl(gs fl(sqrt(fl(a / b))));  h2' = fma(omm, fl(un un), fl(mom h2));   w1 = fl(w0 - fl(lr un))
    target    wt1 = fma(tau, w1, fl(omt wt0))                   only when the soft switch is on

BOUNDS.  Built the way adam_ref.check builds them: one u per rounding, taken against the magnitude of that rounding's RESULT in the
reference (the kernel's own result differs from it by the error accumulated so far, so u |result_kernel| <= u |result_ref| + u x that
error: a second-order term), propagated to first order through the later operations, every bound multiplied by
adam_ref.SECOND_ORDER = 1 + 2**-16 (the relative errors involved stay below 1e-5, their products below 2**-16 of a first-order term).
A rounding whose result is subnormal is off by at most 2**-150 absolute instead: ETA = 2**-149 is added once per rounding.

With G = |g| s_ref, ds = the relative error bound of the kernel's float32 clip scale (adam_ref.delta_s of the launch form's depth,
unchanged; 0 when s_ref == 1), ug = u when s_ref != 1 (the rounding of g * s) else 0, and eg = ug + ds the relative error of gs:

    SGD       lr gs inherits eg;  fl(mom h0) one rounding of that term;  the fma one rounding of h1:
              bh = eg lr G + u mom |h0| + u |h1|
              bw = bh + u |w1|                                   (bw bounds |(w0 - w1) - step_ref|, the quantity adam_ref compares)
    Nesterov  bh as SGD;  un = c1 h1 - mom h0:  c1 times h1's error, the rounding of fl(mom h0) again, the fma's own:
              bu = c1 bh + u mom |h0| + u |un|;   bw = bu + u |w1|
    AdaGrad   gs gs is exact inside the fma and carries 2 eg;  the fma rounds h1 (all terms non-negative):
              bh = 2 eg G^2 + u h1,   rh = bh / h1
              r = sqrt(h1): sqrt halves rh and rounds;  den = r + delta rounds:   bden = r (rh / 2 + u) + u den,   rd = bden / den
              q = gs / den: eg + rd + u;  lr q one more:      bu = |step_ref| (eg + rd + 2 u);   bw = bu + u |w1|
    RMSProp   fl(gs gs) carries 2 eg + u;  fl(rho h0) one rounding of that term;  the fma one of h1:
              bh = omr G^2 (2 eg + u) + u rho h0 + u h1;      the rest as AdaGrad
    AdaDelta  bh as RMSProp with mom for rho;  a = h2 + delta: inputs exact, relative u;  b = h1 + delta: relative rb = bh / b + u;
              a / b: rq = u + rb + u;  sqrt: rq / 2 + u;  gs x root: ru = eg + rq / 2 + 2 u relative on un
              bh2 = omm un^2 (2 ru + u) + u mom h2 + u h2'
              step = lr un rounds once more:  bu = |step_ref| (ru + u);   bw = bu + u |w1|
    target    the fma takes the kernel's own w1 (tau times w's error), fl(omt wt0) one rounding of that term, the fma one of wt1:
              bt = tau bw + u omt |wt0| + u |wt1|

THE APPLIED SCALE, as in adam_ref: a least-squares estimate of the factor the launch multiplied the gradient with, from history 1 —
SGD / Nesterov: <h1 - mom h0, g> / (lr <g, g>);  AdaGrad / RMSProp / AdaDelta: sqrt(<h1 - d h0, g^2> / (c <g^2, g^2>)) with (d, c) =
(1, 1), (rho, omr), (mom, omm).  It must sit within ds s_ref of s_ref; when the clip does not rescale (ds = 0) within six standard
deviations of the estimate's own rounding noise (the per-element roundings of h1 at eg = 0, independent in sign, summed with the
estimator's weights).

Without bounds: a single-history solver leaves history 2 bit-identical; the target is bit-identical when the switch is off.
"""
import collections
import math

import numpy as np

import adam_ref as A

F32, F64 = np.float32, np.float64
U = A.U
SECOND_ORDER = A.SECOND_ORDER
ETA = 2.0 ** -149
State = A.State

SOLVERS = ("Adam", "SGD", "Nesterov", "AdaGrad", "RMSProp", "AdaDelta")        # DQNHIP_SOLVER_*, by value
TWO_HISTORIES = ("Adam", "AdaDelta")

Hyper = collections.namedtuple("Hyper", "lr mom mom2 delta rho tau clip soft_update_freq")


def hyper(lr, mom=0.95, mom2=0.999, delta=1e-8, rho=0.99, tau=0.001, clip=10.0, soft_update_freq=1):
    """the hyper-parameters as the float32 values the kernel receives"""
    return Hyper(F32(lr), F32(mom), F32(mom2), F32(delta), F32(rho), F32(tau), F32(clip), int(soft_update_freq))


def adam_hyper(hp):
    return A.Hyper(hp.lr, hp.mom, hp.mom2, hp.delta, hp.tau, hp.clip, hp.soft_update_freq)


def default_momentum(solver):
    """Caffe refuses a momentum with AdaGrad and RMSProp"""
    return 0.0 if solver in ("AdaGrad", "RMSProp") else 0.95


def reference(solver, hp, before, g, soft, s, t=None):
    """float64 evaluation of one step with clip scale s -> ({"h", "h2", "upd", "w", "target"}, bounds(ds) -> {"h", "h2", "step", "target"})"""
    if solver == "Adam":
        ref, bounds = A.reference(adam_hyper(hp), before, g, t, soft, s)
        return ({"h": ref["m"], "h2": ref["v"], "upd": ref["upd"], "w": ref["w"], "target": ref["target"]},
                lambda ds: (lambda b: {"h": b["m"], "h2": b["v"], "step": b["step"], "target": b["target"]})(bounds(ds)))
    assert solver in SOLVERS, solver
    w0, h0, k0, wt0 = (np.asarray(a, F64) for a in before)
    g64 = np.asarray(g, F64)
    lr, mom, delta, rho, tau = F64(hp.lr), F64(hp.mom), F64(hp.delta), F64(hp.rho), F64(hp.tau)
    c1, omm, omr, omt = F64(F32(1) + hp.mom), F64(F32(1) - hp.mom), F64(F32(1) - hp.rho), F64(F32(1) - hp.tau)
    gs = g64 * s
    G = np.abs(gs)
    k1 = k0
    if solver == "SGD":
        h1 = lr * gs + mom * h0
        upd = h1
    elif solver == "Nesterov":
        h1 = lr * gs + mom * h0
        upd = c1 * h1 - mom * h0
    elif solver in ("AdaGrad", "RMSProp"):
        h1 = gs * gs + h0 if solver == "AdaGrad" else omr * gs * gs + rho * h0
        r = np.sqrt(h1)
        den = r + delta
        upd = lr * (gs / den)
    else:
        h1 = omm * gs * gs + mom * h0
        a, b = k0 + delta, h1 + delta
        un = gs * np.sqrt(a / b)
        k1 = omm * un * un + mom * k0
        upd = lr * un
    w1 = w0 - upd
    wt1 = tau * w1 + omt * wt0 if soft else wt0

    def bounds(ds):
        ug = U if s != 1.0 else 0.0
        eg = ug + ds
        S = SECOND_ORDER
        bh2 = np.zeros_like(h1)
        if solver in ("SGD", "Nesterov"):
            bh = (eg * lr * G + U * mom * np.abs(h0) + U * np.abs(h1) + 3 * ETA) * S
            bu = bh if solver == "SGD" else (c1 * bh + U * mom * np.abs(h0) + U * np.abs(upd) + ETA) * S
        elif solver in ("AdaGrad", "RMSProp"):
            if solver == "AdaGrad":
                bh = (2 * eg * G * G + U * h1 + 2 * ETA) * S
            else:
                bh = (omr * G * G * (2 * eg + U) + U * rho * h0 + U * h1 + 4 * ETA) * S
            with np.errstate(divide="ignore", invalid="ignore"):
                rh = np.where(h1 > 0, bh / h1, 0.0)
                rd = (r * (rh / 2 + U) + U * den + 2 * ETA) / den
            bu = (np.abs(upd) * (eg + rd + 2 * U) + 2 * ETA) * S
        else:
            bh = (omm * G * G * (2 * eg + U) + U * mom * h0 + U * h1 + 4 * ETA) * S
            rb = bh / b + U
            rq = U + rb + U
            ru = eg + rq / 2 + 2 * U
            bh2 = (omm * un * un * (2 * ru + U) + U * mom * k0 + U * k1 + 3 * ETA) * S
            bu = (np.abs(upd) * (ru + U) + ETA) * S
        bw = (bu + U * np.abs(w1) + ETA) * S
        bt = (tau * bw + U * omt * np.abs(wt0) + U * np.abs(wt1) + 2 * ETA) * S
        return {"h": bh, "h2": bh2, "step": bw, "target": bt}
    return {"h": h1, "h2": k1, "upd": upd, "w": w1, "target": wt1}, bounds


def applied_scale(solver, hp, g, h0, h1):
    """-> (the least-squares estimate of the applied clip scale from history 1, six standard deviations of its rounding noise at s = 1)"""
    g64, a0, a1 = np.asarray(g, F64), np.asarray(h0, F64), np.asarray(h1, F64)
    lr, mom, rho = F64(hp.lr), F64(hp.mom), F64(hp.rho)
    omm, omr = F64(F32(1) - hp.mom), F64(F32(1) - hp.rho)
    if solver in ("SGD", "Nesterov"):
        gg = float(np.dot(g64, g64))
        est = float(np.dot(a1 - mom * a0, g64) / (lr * gg))
        n = U * mom * np.abs(a0) + U * np.abs(a1)
        return est, 6 * math.sqrt(float(np.sum((n * g64) ** 2))) / (float(lr) * gg)
    d, c = {"AdaGrad": (1.0, 1.0), "RMSProp": (rho, omr), "AdaDelta": (mom, omm)}[solver]
    g2 = g64 * g64
    gg = float(np.dot(g2, g2))
    est2 = float(np.dot(a1 - d * a0, g2) / (c * gg))
    n = U * a1 + (0.0 if solver == "AdaGrad" else c * g2 * U + U * d * a0)
    return math.sqrt(max(est2, 0.0)), 6 * math.sqrt(float(np.sum((n * g2) ** 2))) / (float(c) * gg) / 2


def check(tag, solver, hp, lay, before, g, after, soft, ds, t=None, estimate_scale=True):
    """One net's pass against the float64 rule of (before, g).  before / after: State(w, h, h2, wt), dense float32; soft: the switch;
    ds: adam_ref.delta_s(D) of the launch form's clip norm (taken as 0 when the clip does not rescale); t = iter + 1 (Adam only).
    Raises AssertionError naming every rule that failed, each with its margin; returns the worst error / bound per array and the scales."""
    if solver == "Adam":
        r = A.check(tag, adam_hyper(hp), lay, before, g, after, t, soft, ds, estimate_scale)
        r["h"], r["h2"] = r["m"], r["v"]
        return r
    g = np.asarray(g, F32)
    s_ref, nrm = A.clip_scale(hp, g)
    if s_ref == 1.0:
        ds = 0.0
    ref, bounds = reference(solver, hp, before, g, soft, s_ref)
    b = bounds(ds)
    fail, out = [], {"s_ref": s_ref, "norm": nrm, "ds": ds}
    a = State(*(np.asarray(x, F32) for x in after))
    for x, name in zip(a, ("w", "h", "h2", "wt")):
        if not np.isfinite(x).all():
            fail.append("%s %s holds %d non-finite elements" % (tag, name, int((~np.isfinite(x)).sum())))
    if estimate_scale and float(np.dot(g.astype(F64), g.astype(F64))) > 0:
        s_app, noise = applied_scale(solver, hp, g, before.m, a.m)
        out["s_applied"], out["s_err"], out["s_noise"] = s_app, abs(s_app - s_ref) / s_ref, noise
        tol = ds * s_ref if ds > 0 else noise
        if not abs(s_app - s_ref) <= tol:
            fail.append("%s applied clip scale %.9e, reference %.9e (||g|| = %.6e): |difference| %.3e > %.3e (margin %.3e, %.1f x the tolerance)"
                        % (tag, s_app, s_ref, nrm, abs(s_app - s_ref), tol, abs(s_app - s_ref) - tol, abs(s_app - s_ref) / tol))
    out["h"] = A._worst(tag, "history 1", np.abs(a.m.astype(F64) - ref["h"]), b["h"], fail)
    if solver in TWO_HISTORIES:
        out["h2"] = A._worst(tag, "history 2", np.abs(a.v.astype(F64) - ref["h2"]), b["h2"], fail)
    else:
        out["h2"] = 0.0
        touched = a.v.view(np.uint32) != np.asarray(before.v, F32).view(np.uint32)
        if touched.any():
            i = int(np.argmax(touched))
            fail.append("%s history 2[%d] changed from %r to %r under a single-history solver (margin: %d elements, by at most %.3e)"
                        % (tag, i, float(before.v[i]), float(a.v[i]), int(touched.sum()), float(np.abs(a.v.astype(F64) - np.asarray(before.v, F64)).max())))
    w0 = np.asarray(before.w, F64)
    out["step"] = A._worst(tag, "step (w0 - w1)", np.abs((w0 - a.w.astype(F64)) - ref["upd"]), b["step"], fail)
    moved = a.wt.view(np.uint32) != np.asarray(before.wt, F32).view(np.uint32)
    if soft:
        out["target"] = A._worst(tag, "target", np.abs(a.wt.astype(F64) - ref["target"]), b["target"], fail)
        if not moved.any():
            fail.append("%s target: the switch is on and no element of the target moved (margin: %d of %d elements)" % (tag, 0, moved.size))
    else:
        out["target"] = 0.0
        if moved.any():
            i = int(np.argmax(moved))
            fail.append("%s target[%d] moved from %r to %r while the switch is off (margin: %d elements moved, by at most %.3e)"
                        % (tag, i, float(before.wt[i]), float(a.wt[i]), int(moved.sum()), float(np.abs(a.wt.astype(F64) - np.asarray(before.wt, F64)).max())))
    if fail:
        raise AssertionError("\n".join(fail))
    return out


# ---- a float32 numpy evaluation of the kernel's own sequence (the host test's stand-in for the kernel, with its planted faults) ---------------
FAULTS = ("nesterov_as_sgd", "delta_inside_root", "adagrad_decay", "adadelta_swapped", "adadelta_lr_first", "touch_h2", "stale_target_row")


def simulate32(solver, hp, before, g, soft, s32, t=None, fault=None, stale=slice(0, 64)):
    """the rules in float32 numpy, operation for operation (fma: evaluated in float64 and rounded once — the products are exact there)"""
    assert fault is None or fault in FAULTS, fault
    if solver == "Adam":
        return A.simulate32(adam_hyper(hp), before, g, t, soft, s32)
    w0, h0, k0, wt0 = (np.asarray(a, F32) for a in before)
    g = np.asarray(g, F32)
    lr, mom, delta, rho = hp.lr, hp.mom, hp.delta, hp.rho
    c1, omm, omr, omt = F32(1) + mom, F32(1) - mom, F32(1) - rho, F32(1) - hp.tau
    fl = lambda x: np.asarray(x, F32)
    fma = lambda a, b, c: (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)
    gs = fl(g * F32(s32))
    k1 = k0.copy()
    if solver in ("SGD", "Nesterov"):
        mh0 = fl(mom * h0)
        h1 = fma(lr, gs, mh0)
        upd = h1 if (solver == "SGD" or fault == "nesterov_as_sgd") else fma(c1, h1, -mh0)
    elif solver in ("AdaGrad", "RMSProp"):
        if solver == "AdaGrad":
            h1 = fma(gs, gs, fl(F32(0.99) * h0) if fault == "adagrad_decay" else h0)
        else:
            h1 = fma(omr, fl(gs * gs), fl(rho * h0))
        den = fl(np.sqrt(fl(h1 + delta))) if fault == "delta_inside_root" else fl(fl(np.sqrt(h1)) + delta)
        upd = fl(lr * fl(gs / den))
    else:
        if fault == "adadelta_swapped":
            h0, k0 = k0, h0
        h1 = fma(omm, fl(gs * gs), fl(mom * h0))
        un = fl(gs * fl(np.sqrt(fl(fl(k0 + delta) / fl(h1 + delta)))))
        if fault == "adadelta_lr_first":
            un = fl(lr * un)
            upd = un
        else:
            upd = fl(lr * un)
        k1 = fma(omm, fl(un * un), fl(mom * k0))
        if fault == "adadelta_swapped":
            h1, k1 = k1, h1
    if fault == "touch_h2":
        k1 = fl(k1 + fl(gs * gs))
    w1 = fl(w0 - upd)
    wt1 = fma(hp.tau, w1, fl(omt * wt0)) if soft else wt0.copy()
    if fault == "stale_target_row":
        wt1[stale] = wt0[stale]
    return State(w1, h1, k1, wt1)
