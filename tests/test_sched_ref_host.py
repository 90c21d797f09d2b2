"""tests/sched_ref.py without a GPU, in the manner of tests/test_solver_ref_host.py: on the inputs of every case of
tests/sched_forms_lib.py (gradients from the C oracle's backward pass) the float32 stand-in of the scheduled, regularised pass is
accepted, and every planted fault that applies to the case is rejected — the decay dropped, L1 where L2 was asked for (and the
reverse), the decay scaled by the clip, sign(0) = 1, the previous iteration's rate (a stale DevState slot), Adam's step without the
bias correction, a rate off by 1 %.  This is where the schedules and the decay of sched_forms_lib were chosen: the GPU test then
cannot hide one of these behind its bounds."""
import functools

import numpy as np
import pytest

import adam_ref as A
import optimizer_forms_lib as L
import sched_forms_lib as SF
import sched_ref as SR
import solver_ref as R
from oracle import c_oracle

F32, F64 = np.float32, np.float64
IT = SF.WARMUP                  # the first tested iteration


@functools.lru_cache(maxsize=None)
def _inputs(B, S, hidden, seed, n_updates):
    case = L._case("host", "eager", B, S, hidden, seed=seed, n_updates=n_updates)
    inp = L.make_inputs(case)
    o = c_oracle.Oracle(B=B, S=S, hidden=hidden, capacity=2 * L.REPLAY, clip=-1.0)
    try:
        for net in range(4):
            o.set_params(net, inp["w"][net])
        o.add_transitions(inp["s"], inp["a"], inp["r"], inp["mc"], inp["nx"], inp["term"])
        row, g = inp["idx"][0], {}
        o.update_phase(0, row); g[1] = o.grad_view(1).copy()
        o.update_phase(1, row); g[0] = o.grad_view(0).copy()
        o.update_phase(2, row)
    finally:
        o.close()
    return inp["w"], g


def _layouts(case):
    fp16 = case.precision == "fp16"
    return {0: A.layout(case.S, case.hidden, True, fp16), 1: A.layout(case.S + L.NO, case.hidden, False, fp16)}


def _warm_state(sc, hp, w, wt, g, s32):
    """WARMUP float32 steps of the case's own pass at iterations 0, 1: histories of real magnitude; then exact zeros planted in w, so that
    sign(0) is asked for"""
    st = R.State(w, np.zeros_like(w), np.zeros_like(w), wt)
    for it in range(SF.WARMUP):
        st = SR.simulate32(sc.solver, hp, sc.sched, sc.decay, sc.kind, st, g, it, True, s32)
    w0 = st.w.copy()
    w0[::97] = 0
    return st._replace(w=w0)


def _faults(sc):
    out = ["rate_1pct"]
    if sc.decay:
        out += ["decay_dropped", "l1_for_l2", "decay_before_clip"]
        if sc.kind == "L1":
            out.append("sign0_is_1")
    if sc.sched.policy != "fixed":
        out.append("stale_rate")
    if sc.solver == "Adam":
        out.append("no_bias_correction")
    return out


@pytest.mark.parametrize("name", [c.name for c in SF.CASES])
def test_stand_in_accepted_and_every_fault_rejected(name):
    sc = SF.CASE_BY_NAME[name]
    case = sc.case
    w, g = _inputs(case.B, case.S, case.hidden, case.seed, case.n_updates)
    lays, hps = _layouts(case), SF.hypers(sc)
    for net in (0, 1):
        hp, lay = hps[net], lays[net]
        ds = A.delta_s(A.depth_update(lay, case.precision))
        s32 = A.scale32(hp, g[net])
        assert s32 < 0.5, (name, net, "the clip must rescale, or a decay applied before it cannot show")
        before = _warm_state(sc, hp, w[net], w[net + 2], g[net], s32)
        args = (sc.solver, hp, sc.sched, sc.decay, sc.kind)
        for soft in (True, False):
            after = SR.simulate32(*args, before, g[net], IT, soft, s32)
            r = SR.check("%s net %d" % (name, net), *args, lay, before, g[net], after, IT, soft, ds)
            assert max(r["h"], r["h2"], r["step"], r["target"]) <= 1.0
            print("SCHEDSIM %-40s net %d soft %d  h %.3f h2 %.3f step %.3f target %.3f rate %.4e" % (name, net, soft, r["h"], r["h2"], r["step"], r["target"], r["rate"]))
        for fault in _faults(sc):
            bad = SR.simulate32(*args, before, g[net], IT, True, s32, fault=fault)
            with pytest.raises(AssertionError, match="margin") as e:
                SR.check("%s net %d %s" % (name, net, fault), *args, lay, before, g[net], bad, IT, True, ds)
            print("%-60s %s" % ("%s net %d: %s" % (name, net, fault), str(e.value).splitlines()[0][:160]))


def test_every_fault_is_planted_somewhere():
    seen = set()
    for sc in SF.CASES:
        seen.update(_faults(sc))
    assert seen == set(SR.FAULTS)
    # every schedule gives the first tested iteration another rate than the one before it, and exp every later one too
    for policy, s in SF.SCHEDULES.items():
        if policy != "fixed":
            assert SR.rate(s, 1e-3, IT) != SR.rate(s, 1e-3, IT - 1), policy
    rates = [SR.rate(SF.SCHEDULES["exp"], 1e-3, it) for it in range(8)]
    assert len(set(rates)) == 8


def test_rates_closed_forms():
    b = F32(1e-3)
    assert SR.rate(SR.schedule("step", gamma=0.5, stepsize=3), b, 8) == F32(b * F32(0.25))
    assert SR.rate(SR.schedule("multistep", gamma=0.5, stepvalues=(3, 5)), b, 4) == F32(b * F32(0.5))
    assert SR.rate(SR.schedule("multistep", gamma=0.5, stepvalues=(3, 5)), b, 5) == F32(b * F32(0.25))
    assert SR.rate(SR.schedule("poly", max_iter=10, power=1.0), b, 10) == 0 and SR.rate(SR.schedule("poly", max_iter=10, power=0.5), b, 11) == 0
    assert SR.rate(SR.schedule("sigmoid", gamma=1.0, stepsize=7), b, 7) == F32(b / 2)
    assert SR.rate(SR.schedule("inv", gamma=1.0, power=1.0), b, 3) == F32(float(b) / 4)
    assert SR.current_step(SR.schedule("step", stepsize=4), 11) == 2 and SR.current_step(SR.schedule("exp", gamma=0.5), 11) == 0
    # the regularised gradient: sign(0) = 0
    g = SR.reg_gradient(np.array([1.0, 1.0, 1.0], F32), np.array([0.0, -2.0, 3.0], F32), 0.5, 0.25, "L1")
    np.testing.assert_array_equal(g, [0.5, 0.25, 0.75])
    g = SR.reg_gradient(np.array([1.0, 1.0, 1.0], F32), np.array([0.0, -2.0, 3.0], F32), 0.5, 0.25, "L2")
    np.testing.assert_array_equal(g, [0.5, 0.0, 1.25])
    h1, w1 = SR.sgd_plain32(F32(0.5), np.array([1.0], F32), np.array([0.25], F32))
    assert h1[0] == 0.125 and w1[0] == 0.875
