"""Float64 reference and per-element comparator for the optimiser pass of a learner with an lr policy and / or a weight decay (numpy
only; imports nothing of the package).  tests/solver_ref.py and tests/adam_ref.py are used unchanged: the six rules and their bounds
are theirs, this module puts Caffe's GetLearningRate and Regularize in front of them.

THE RATE (dqn-hfo_amd/csrc/lr_schedule.hip.h).  `it` is the net's solver iteration before its increment, every
parameter the float32 value the library receives, the expression evaluated in float64 and rounded to float32 ONCE:

    fixed base                               step      base gamma^(it // stepsize)         exp   base gamma^it
    inv   base (1 + gamma it)^(-power)       multistep base gamma^#{stepvalue <= it}       poly  base max(0, 1 - it / max_iter)^power
    sigmoid base / (1 + exp(-gamma (it - stepsize)))

The library's pow / exp are good to a few float64 ulps; such a value can land on the other side of a float32 rounding boundary and
can do no more than that: a rate is accepted within 1 float32 ulp (RATE_ULP), relative size at most ULR = 2**-23.

THE REGULARISED GRADIENT, after the clip, per element:  gd = fma(decay, r, fl(g s)),  r = w0 (L2) or sign(w0) with
sign(0) = 0 (L1) — r and decay r are exact inside the fma; the clip norm is that of g alone.  With decay == 0 the fma returns fl(g s).
Its error against the float64 gd_ref = decay r + g s_ref:

    e_gd = (ug + ds) |g| s_ref + (u |gd_ref| if decay != 0 else 0) + ETA        ug = u when s_ref != 1 (the rounding of g s), ds: the clip scale's

THE RULES run on gd with lr = the rate (Adam: step = fl(rate fl(correction)), Caffe's local_rate * correction).  The reference is
solver_ref.reference / adam_ref.reference on (gd_ref, s = 1, lr = fl32(rate_ref)); their bounds take the gradient's relative error as
`ds`, per element here: eg = e_gd / |gd_ref| (times 1 + eg: the squared-gradient rules' second-order term where a decay cancels most
of a gradient).  A rate that is 1 ulp off adds, to first order:

    SGD, Nesterov        lr gd is a term of the history: eg + ULR in place of eg
    AdaGrad, RMSProp, AdaDelta   lr scales the finished update: ULR |upd| on the step, tau times that on the target
    Adam                 (ULR + u) |upd| likewise (the product rate x correction rounds once more, from another operand)

The k_sched_soft<> family evaluates Adam's rule with contraction off (w0 - fl(step q)), the tuned kernels may contract it: both are
inside adam_ref's bound (adam_ref.py says so).

THE ONE BIT-EXACT STATEMENT (SGD, momentum 0, clip off, no decay, the k_sched_soft<kSolverSGD> kernel):
    h1 = fl(rate g)  (fmaf(rate, g, fl(0 h0)) with h0 finite: one rounding of the product);  w1 = fl(w0 - h1)
`sgd_plain32` evaluates exactly that.
"""
import collections
import math

import numpy as np

import adam_ref as A
import solver_ref as R

F32, F64 = np.float32, np.float64
U = A.U
ULR = 2.0 ** -23
ETA = R.ETA
SECOND_ORDER = A.SECOND_ORDER
State = A.State

POLICIES = ("fixed", "step", "exp", "inv", "multistep", "poly", "sigmoid")      # DQNHIP_LR_*, by value
REGULARIZATIONS = ("L2", "L1")

Schedule = collections.namedtuple("Schedule", "policy gamma power stepsize max_iter stepvalues")


def schedule(policy="fixed", gamma=0.0, power=0.0, stepsize=0, max_iter=0, stepvalues=()):
    """the schedule as the float32 / int32 values the library receives"""
    assert policy in POLICIES, policy
    return Schedule(policy, F32(gamma), F32(power), int(stepsize), int(max_iter), tuple(int(v) for v in stepvalues))


FIXED = schedule()


def dqn_kwargs(s, decay=0.0, kind="L2"):
    """the DQN(...) keyword arguments of a schedule and a decay"""
    return dict(lr_policy=s.policy, lr_gamma=float(s.gamma), lr_power=float(s.power), lr_stepsize=s.stepsize, lr_max_iter=s.max_iter,
                lr_stepvalues=s.stepvalues, weight_decay=decay, regularization=kind)


def current_step(s, it):
    """Caffe's current_step_ as GetLearningRate leaves it at iteration `it` (an exact integer)"""
    if s.policy == "step":
        return it // s.stepsize
    if s.policy == "multistep":
        return sum(1 for v in s.stepvalues if v <= it)
    return 0


def rate64(s, base_lr, it):
    base, g, p = float(F32(base_lr)), float(s.gamma), float(s.power)
    pw = lambda x, y: float(np.power(F64(x), F64(y)))          # (numpy: inf where Python's ** raises)
    if s.policy == "fixed":
        return base
    with np.errstate(over="ignore", under="ignore"):
        if s.policy in ("step", "multistep"):
            return base * pw(g, current_step(s, it))
        if s.policy == "exp":
            return base * pw(g, it)
        if s.policy == "inv":
            return base * pw(1.0 + g * it, -p)
        if s.policy == "poly":
            return base * pw(max(0.0, 1.0 - it / s.max_iter), p)
    if s.policy == "sigmoid":
        x = -g * (it - s.stepsize)
        return base / (1.0 + math.exp(x)) if x < 700 else 0.0
    raise ValueError(s.policy)


def rate(s, base_lr, it):
    """the float32 rate of iteration `it`"""
    with np.errstate(over="ignore", under="ignore"):
        return F32(rate64(s, base_lr, it))


def ulps32(a, b):
    """distance of two finite float32 values of one sign in units in the last place"""
    ia, ib = int(np.asarray(a, F32).view(np.int32)), int(np.asarray(b, F32).view(np.int32))
    return abs(ia - ib)


RATE_ULP = 1


def sign0(w):
    return np.sign(np.asarray(w, F64))          # numpy: sign(0) = 0


def reg_gradient(g, w0, s, decay, kind):
    """float64 gd = decay r + g s"""
    assert kind in REGULARIZATIONS, kind
    r = np.asarray(w0, F64) if kind == "L2" else sign0(w0)
    return F64(F32(decay)) * r + np.asarray(g, F64) * s


def reference(solver, hp, sched, decay, kind, before, g, it, soft, s):
    """-> (ref, bounds(ds), rate_ref): solver_ref.reference of the regularised gradient under the scheduled rate.  hp.lr is the BASE rate."""
    rate_ref = rate(sched, hp.lr, it)
    gd = reg_gradient(g, before.w, s, decay, kind)
    hp_eff = hp._replace(lr=rate_ref)
    ref, inner = R.reference(solver, hp_eff, before, gd, soft, 1.0, t=it + 1)
    G = np.abs(np.asarray(g, F64)) * s
    absgd = np.abs(gd)
    scheduled = sched.policy != "fixed"

    def bounds(ds):
        ug = U if s != 1.0 else 0.0
        e_gd = (ug + ds) * G + (U * absgd if float(decay) != 0.0 else 0.0) + ETA
        with np.errstate(divide="ignore", invalid="ignore"):
            eg = np.where(absgd > 0, e_gd / absgd, 0.0)
        eg = eg * (1.0 + eg)
        ulr = ULR if scheduled else 0.0
        b = dict(inner(eg + ulr if solver in ("SGD", "Nesterov") else eg))
        if solver not in ("SGD", "Nesterov") and scheduled:
            extra = (ulr + (U if solver == "Adam" else 0.0)) * np.abs(ref["upd"]) * SECOND_ORDER
            b["step"] = b["step"] + extra
            b["target"] = b["target"] + float(hp.tau) * extra
        return b
    return ref, bounds, rate_ref


def check(tag, solver, hp, sched, decay, kind, lay, before, g, after, it, soft, ds):
    """One net's pass against the float64 rule.  before / after: State(w, h, h2, wt), dense float32; hp: solver_ref.Hyper with the BASE rate;
    it: the net's iteration before the update; ds: adam_ref.delta_s(D) of the launch form's clip norm (taken as 0 when the clip does not
    rescale).  Raises AssertionError naming every rule that failed, each with its margin; returns the worst error / bound per array."""
    g = np.asarray(g, F32)
    s_ref, nrm = A.clip_scale(hp, g)            # the norm of the UNREGULARISED gradient
    if s_ref == 1.0:
        ds = 0.0
    ref, bounds, rate_ref = reference(solver, hp, sched, decay, kind, before, g, it, soft, s_ref)
    b = bounds(ds)
    fail, out = [], {"s_ref": s_ref, "norm": nrm, "ds": ds, "rate": float(rate_ref)}
    a = State(*(np.asarray(x, F32) for x in after))
    for x, name in zip(a, ("w", "h", "h2", "wt")):
        if not np.isfinite(x).all():
            fail.append("%s %s holds %d non-finite elements" % (tag, name, int((~np.isfinite(x)).sum())))
    out["h"] = A._worst(tag, "history 1", np.abs(a.m.astype(F64) - ref["h"]), b["h"], fail)
    if solver in R.TWO_HISTORIES:
        out["h2"] = A._worst(tag, "history 2", np.abs(a.v.astype(F64) - ref["h2"]), b["h2"], fail)
    else:
        out["h2"] = 0.0
        touched = a.v.view(np.uint32) != np.asarray(before.v, F32).view(np.uint32)
        if touched.any():
            fail.append("%s history 2 changed under a single-history solver (margin: %d elements)" % (tag, int(touched.sum())))
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
            fail.append("%s target moved while the switch is off (margin: %d elements moved)" % (tag, int(moved.sum())))
    if fail:
        raise AssertionError("\n".join(fail))
    return out


# ---- a float32 numpy evaluation of the kernel's own sequence, with planted faults -------------------------------------------------------------
FAULTS = ("decay_dropped", "l1_for_l2", "decay_before_clip", "sign0_is_1", "stale_rate", "no_bias_correction", "rate_1pct")


def simulate32(solver, hp, sched, decay, kind, before, g, it, soft, s32, fault=None):
    """the scheduled, regularised pass in float32 numpy, operation for operation (hp.lr: the base rate)"""
    assert fault is None or fault in FAULTS, fault
    w0 = np.asarray(before.w, F32)
    g = np.asarray(g, F32)
    fma = lambda a, b, c: (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)
    lr = rate(sched, hp.lr, it - 1 if fault == "stale_rate" else it)
    if fault == "rate_1pct":
        lr = F32(lr * F32(1.01))
    if fault == "no_bias_correction":
        assert solver == "Adam"
        lr = F32(lr / A.correction(R.adam_hyper(hp), it + 1))
    if fault == "l1_for_l2":
        kind = "L1" if kind == "L2" else "L2"
    r = w0 if kind == "L2" else np.sign(w0).astype(F32)
    if fault == "sign0_is_1":
        assert kind == "L1"
        r = np.where(w0 >= 0, F32(1), F32(-1)).astype(F32)
    d = F32(0) if fault == "decay_dropped" else F32(decay)
    gs = (g * F32(s32)).astype(F32)
    gd = (fma(d, r, g) * F32(s32)).astype(F32) if fault == "decay_before_clip" else fma(d, r, gs)
    return R.simulate32(solver, hp._replace(lr=lr), before, gd, soft, F32(1), t=it + 1)


def sgd_plain32(rate32, w0, g):
    """the one bit-exact statement of the docstring: -> (h1, w1)"""
    h1 = (np.asarray(rate32, F64) * np.asarray(g, F32).astype(F64)).astype(F32)
    return h1, (np.asarray(w0, F32) - h1).astype(F32)
