"""The cases of tests/test_gpu_lr_policy.py (numpy only: tests/test_sched_ref_host.py runs the float32 stand-in and the planted faults on
the same inputs, on the CPU — which is where the schedules and the decay below were chosen: every fault of sched_ref.FAULTS that
applies to a case is rejected on that case, at the case's first tested iteration).

Shapes, clip, soft switch and inputs are tests/optimizer_forms_lib.py's, WARMUP = 2 updates first, so the tested updates run at
iterations 2, 3, ...  The schedules put a boundary there: every one of them gives iteration 2 another rate than iteration 1 (a stale
DevState slot shows), and `exp` halves the rate with every update of a multi-update case.

    step       gamma 0.5, stepsize 2          rate(1) = base,        rate(2) = base / 2
    exp        gamma 0.5                       base / 2,              base / 4, / 8, ...
    inv        gamma 0.5, power 1              base / 1.5,            base / 2
    multistep  gamma 0.1, stepvalues (2, 4)    base,                  base / 10        (the issue's (3, 5) moved onto the tested iteration)
    poly       max_iter 8, power 2             base (7/8)^2,          base (6/8)^2
    sigmoid    gamma 1, stepsize 2             base / (1 + e),        base / 2

weight_decay = 1e-2: against clipped gradients of norm 0.02 over 1e4 .. 1e6 elements and weights of order 0.1 the decay term is as large
as the gradient (L2) or far larger (L1) — dropping it, taking the other kind, or scaling it by the clip (s_ref of order 1e-2) each move
every history by many bounds.

`family`: "adam" — an Adam learner with a policy and no decay, on the tuned Adam kernels with their riders; "sched" — k_sched_soft<>."""
import collections

import optimizer_forms_lib as L
import sched_ref as SR
import solver_forms_lib as SL
import solver_ref as R

WARMUP = L.WARMUP
DECAY = 1e-2

SCHEDULES = {
    "fixed": SR.FIXED,
    "step": SR.schedule("step", gamma=0.5, stepsize=2),
    "exp": SR.schedule("exp", gamma=0.5),
    "inv": SR.schedule("inv", gamma=0.5, power=1.0),
    "multistep": SR.schedule("multistep", gamma=0.1, stepvalues=(2, 4)),
    "poly": SR.schedule("poly", max_iter=8, power=2.0),
    "sigmoid": SR.schedule("sigmoid", gamma=1.0, stepsize=2),
}
HYPER = dict(SL.HYPER, Adam=dict(actor_lr=1e-5, critic_lr=1e-3, momentum=0.95))

SchedCase = collections.namedtuple("SchedCase", "name solver case per sched decay kind family")

# form -> (mode, B, S, hidden, keyword arguments of optimizer_forms_lib._case)
FORMS = {
    "eager": ("eager", 32, 59, (64, 128), {}),
    "graph": ("graph", 32, 59, (64, 128), {}),
    "indexed": ("indexed", 32, 59, (64, 128), dict(freq=3, tau=0.25, n_updates=4)),
    "chained": ("chained", 32, 59, (64, 128), dict(freq=3, tau=0.25, n_updates=2)),
    "fwd1_k64_4riders": ("eager", 32, 54, (64, 128), {}),
    "second_round": ("eager", 32, 59, (1024, 1024, 512), {}),
    "shared_prefix": ("shared", 32, 59, (64, 128), {}),
    "fp16_static": ("eager", 128, 59, (256, 128, 128), dict(precision="fp16", want=("fp16",), loss_scale=0.0625, freq=2, tau=0.25, n_updates=2)),
    "fp16_dynamic": ("eager", 128, 59, (256, 128, 128), dict(precision="fp16", want=("fp16",), loss_scale=0.0625, loss_mode="dynamic", freq=2, tau=0.25,
                                                             n_updates=2)),
    "prioritized": ("eager", 32, 59, (64, 128), {}),
}
# seeds by form: the cases of one form share their inputs (and the host test its oracle gradients)
SEED = {f: 300 + i for i, f in enumerate(FORMS)}
# AdaGrad's and Adam's warm-up leave action.b below the clip-scale coverage on the shared second_round inputs (solver_forms_lib has the
# story; Adam here: 3.0e-5 of the actor's sum g^2 against adam_ref.COVER * delta_s = 6.4e-5): the inputs of optimizer_forms_lib's own case
SEED_OWN_SECOND_ROUND = L.CASE_BY_NAME["second_round"].seed


def hypers(sc):
    """{net: solver_ref.Hyper} of a case, lr = the BASE rate"""
    kw = HYPER[sc.solver]
    c = sc.case
    common = dict(mom=kw["momentum"], delta=kw.get("delta", 1e-8), rho=kw.get("rms_decay", 0.99), clip=c.clip, tau=c.tau, soft_update_freq=c.freq)
    return {0: R.hyper(kw["actor_lr"], **common), 1: R.hyper(kw["critic_lr"], **common)}


def dqn_kwargs(sc):
    return dict(HYPER[sc.solver], solver=sc.solver, **SR.dqn_kwargs(sc.sched, sc.decay, sc.kind))


def _cases():
    out = []

    def add(solver, policy, form, decay=0.0, kind="L2"):
        mode, B, S, hidden, kw = FORMS[form]
        name = "%s_%s_%s%s" % (solver, policy, form, "_%s" % kind if decay else "")
        seed = SEED_OWN_SECOND_ROUND if (solver in ("AdaGrad", "Adam") and form == "second_round") else SEED[form]
        kw = dict(kw)
        family = "sched" if (decay or solver != "Adam") else "adam"
        if family == "adam" and "precision" not in kw:
            kw["want"] = ("critic_l0_rides",) + (("early_gather_l0",) if mode in ("indexed", "chained") else ())
        out.append(SchedCase(name, solver, L._case(name, mode, B, S, hidden, seed=seed, **kw), form == "prioritized", SCHEDULES[policy], decay, kind, family))

    # policies on Adam: the tuned kernels, riders present in the plan
    for policy in SR.POLICIES[1:]:
        add("Adam", policy, "eager")
        add("Adam", policy, "graph")
    for form in ("indexed", "chained", "fwd1_k64_4riders", "second_round", "fp16_static", "fp16_dynamic"):
        add("Adam", "exp", form)
    # the new family: a policy on the five other solvers ...
    for solver in SL.NEW:
        add(solver, "exp", "eager")
        add(solver, "multistep", "eager")
    # ... and a decay on all six, with and without a policy, the forms dealt out in turn, one further every eight (each form three
    # times: with both kinds, with and without a policy, under three solvers)
    forms = ("eager", "graph", "indexed", "chained", "second_round", "shared_prefix", "fp16_static", "fp16_dynamic")
    k = 0
    for solver in R.SOLVERS:
        for kind in SR.REGULARIZATIONS:
            for policy in ("fixed", "exp"):
                add(solver, policy, forms[(k + k // 8) % len(forms)], DECAY, kind)
                k += 1
    add("RMSProp", "exp", "prioritized", DECAY, "L2")
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
