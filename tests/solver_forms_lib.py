"""The cases of tests/test_gpu_solvers.py (numpy only: tests/test_solver_ref_host.py runs the float32 stand-in on the same inputs).

Per solver the launch forms of tests/optimizer_forms_lib.py that a learner without first-layer riders takes — shapes, clip, soft
switch and inputs are that module's (`make_inputs`), WARMUP = 2 updates first.  Hyper-parameters per solver: momentum 0 where Caffe
demands it; learning rates at which one step moves a weight by many float32 ulps, so that the step check has something to measure
(AdaDelta's step does not scale with the gradient: lr times sqrt(h2 + delta) / sqrt(h + delta) of order 1e-3 .. 1, Caffe's examples
run it at lr 1 and delta 1e-6)."""
import collections

import optimizer_forms_lib as L
import solver_ref as R

WARMUP = L.WARMUP

# solver -> DQN keyword arguments
HYPER = {
    "SGD": dict(actor_lr=1e-3, critic_lr=1e-2, momentum=0.95),
    "Nesterov": dict(actor_lr=1e-3, critic_lr=1e-2, momentum=0.95),
    "AdaGrad": dict(actor_lr=1e-5, critic_lr=1e-3, momentum=0.0),
    "RMSProp": dict(actor_lr=1e-5, critic_lr=1e-3, momentum=0.0, rms_decay=0.99),
    "AdaDelta": dict(actor_lr=1e-2, critic_lr=0.5, momentum=0.95, delta=1e-6),
}
NEW = tuple(s for s in R.SOLVERS if s != "Adam")

SCase = collections.namedtuple("SCase", "name solver case per")


def hypers(sc):
    """{net: solver_ref.Hyper} of a case"""
    kw = HYPER[sc.solver]
    c = sc.case
    common = dict(mom=kw["momentum"], delta=kw.get("delta", 1e-8), rho=kw.get("rms_decay", 0.99), clip=c.clip, tau=c.tau, soft_update_freq=c.freq)
    return {0: R.hyper(kw["actor_lr"], **common), 1: R.hyper(kw["critic_lr"], **common)}


def _cases():
    out = []
    for solver in NEW:
        first = len(out)

        def add(tag, mode, B, S, hidden, per=False, **kw):
            name = "%s_%s" % (solver, tag)
            # (the seed goes by the form, not the solver: the five solvers' cases of one form share their inputs)
            out.append(SCase(name, solver, L._case(name, mode, B, S, hidden, seed=100 + len(out) - first, **kw), per))
        add("eager", "eager", 32, 59, (64, 128))
        add("graph", "graph", 32, 59, (64, 128))
        # k_solver_soft_gather<>: both DevState slots, the switch on and off
        add("indexed", "indexed", 32, 59, (64, 128), freq=3, tau=0.25, n_updates=4)
        add("chained", "chained", 32, 59, (64, 128), freq=3, tau=0.25, n_updates=2)
        # the 1536-block cap: a second, short and ragged strided round
        add("second_round", "eager", 32, 59, (1024, 1024, 512))
        if solver == "AdaGrad":
            # on the shared inputs AdaGrad's two warm-up steps leave action.b 6e-6 of the actor's sum g^2, below the coverage condition of the
            # clip-scale check (adam_ref.COVER * delta_s = 6.4e-5); the inputs of optimizer_forms_lib's own second_round case instead
            out[-1] = out[-1]._replace(case=out[-1].case._replace(seed=L.CASE_BY_NAME["second_round"].seed))
        add("exact_clip_disabled", "eager", 32, 59, (64, 128), clip=-1.0)
        add("exact_norm_below_clip", "eager", 32, 59, (64, 128), clip=1e6)
        add("shared_prefix", "shared", 32, 59, (64, 128))
        add("fp16_static", "eager", 128, 59, (256, 128, 128), precision="fp16", want=("fp16",), loss_scale=0.0625, freq=2, tau=0.25, n_updates=2)
        add("fp16_dynamic", "eager", 128, 59, (256, 128, 128), precision="fp16", want=("fp16",), loss_scale=0.0625, loss_mode="dynamic", freq=2, tau=0.25,
            n_updates=2)
        if solver == "RMSProp":
            add("prioritized", "eager", 32, 59, (64, 128), per=True)
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
