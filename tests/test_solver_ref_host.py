"""tests/solver_ref.py without a GPU: closed forms of the five rules in float64, the float32 stand-in of the kernel accepted on the
inputs of every GPU case (tests/solver_forms_lib.py; gradients from the C oracle's backward pass on those inputs), planted faults
rejected with their margins, and the configuration surface of the library (defaults, refusals with Caffe's wording, names, ABI size)."""
import ctypes as C
import functools

import numpy as np
import pytest

import adam_ref as A
import optimizer_forms_lib as L
import solver_forms_lib as SL
import solver_ref as R
from oracle import c_oracle

F32, F64 = np.float32, np.float64


# ---- 1. closed forms --------------------------------------------------------------------------------------------------------------------------
def _run(solver, hp, g, n, w0=0.5):
    """n float64 steps of the reference from zero histories under the constant gradient g (no clip, no soft update) -> [State]"""
    g = np.asarray(g, F64)
    st = R.State(np.full(g.shape, w0, F64), np.zeros_like(g), np.zeros_like(g), np.full(g.shape, w0, F64))
    out = []
    for _ in range(n):
        ref, _b = R.reference(solver, hp, st, g, False, 1.0)
        st = R.State(ref["w"], ref["h"], ref["h2"], ref["target"])
        out.append(st)
    return out


G = np.array([0.3, -0.02, 1e-4, -7.0, 0.0])
WTOL = 8 * 2.0 ** -52 * 4.0      # w0 - w_n is read off weights of magnitude < 4 that took up to 7 float64 roundings and one subtraction


def test_sgd_and_nesterov_geometric_sums():
    hp = R.hyper(1e-2, mom=0.9, clip=-1.0)
    lr, mu = F64(hp.lr), F64(hp.mom)
    c1 = F64(F32(1) + hp.mom)
    n = 7
    sgd, nes = _run("SGD", hp, G, n), _run("Nesterov", hp, G, n)
    h = lambda k: lr * G * (1 - mu ** k) / (1 - mu)                     # h_k = lr g (1 + mu + .. + mu^(k-1))
    for k in range(1, n + 1):
        np.testing.assert_allclose(sgd[k - 1].m, h(k), rtol=1e-13, atol=0)
        np.testing.assert_allclose(nes[k - 1].m, h(k), rtol=1e-13, atol=0)
    np.testing.assert_allclose(0.5 - sgd[-1].w, sum(h(k) for k in range(1, n + 1)), rtol=1e-12, atol=WTOL)
    np.testing.assert_allclose(0.5 - nes[-1].w, sum(c1 * h(k) - mu * h(k - 1) for k in range(1, n + 1)), rtol=1e-12, atol=WTOL)
    for s in sgd + nes:
        assert not s.v.any()
    # Nesterov at momentum 0 is SGD
    hp0 = R.hyper(1e-2, mom=0.0, clip=-1.0)
    for a, b in zip(_run("SGD", hp0, G, 4), _run("Nesterov", hp0, G, 4)):
        np.testing.assert_array_equal(a.w, b.w); np.testing.assert_array_equal(a.m, b.m)


def test_adagrad_and_rmsprop_histories():
    hp = R.hyper(1e-2, mom=0.0, rho=0.9, delta=1e-8, clip=-1.0)
    n = 6
    rho, omr = F64(hp.rho), F64(F32(1) - hp.rho)
    ada, rms = _run("AdaGrad", hp, G, n), _run("RMSProp", hp, G, n)
    for k in range(1, n + 1):
        np.testing.assert_allclose(ada[k - 1].m, k * G * G, rtol=1e-13)                               # h = n g^2
        np.testing.assert_allclose(rms[k - 1].m, omr * (1 - rho ** k) / (1 - rho) * G * G, rtol=1e-13)  # = (1 - rho^n) g^2 with omr = 1 - rho
    assert abs(omr / (1 - rho) - 1) < 1e-6                 # (fl32(1 - rho) against 1 - rho: the constant the kernel forms)
    lr, d = F64(hp.lr), F64(hp.delta)
    np.testing.assert_allclose(0.5 - ada[0].w, lr * G / (np.abs(G) + d), rtol=1e-13, atol=WTOL)
    # RMSProp at rho = 0 steps lr g / (|g| + delta), every time
    hp0 = R.hyper(1e-2, mom=0.0, rho=0.0, delta=1e-8, clip=-1.0)
    r0 = _run("RMSProp", hp0, G, 3)
    np.testing.assert_allclose(0.5 - r0[-1].w, 3 * lr * G / (np.abs(G) + d), rtol=1e-12, atol=WTOL)
    for s in ada + rms:
        assert not s.v.any()


def test_adadelta_first_step_from_zero_histories():
    hp = R.hyper(0.5, mom=0.95, delta=1e-6, clip=-1.0)
    mu, omm, d, lr = F64(hp.mom), F64(F32(1) - hp.mom), F64(hp.delta), F64(hp.lr)
    s = _run("AdaDelta", hp, G, 1)[0]
    u = G * np.sqrt(d / (omm * G * G + d))
    np.testing.assert_allclose(s.m, omm * G * G, rtol=1e-14)
    np.testing.assert_allclose(s.v, omm * u * u, rtol=1e-13)
    np.testing.assert_allclose(0.5 - s.w, lr * u, rtol=1e-12, atol=WTOL)          # lr scales the step, not the update history


# ---- 2. the float32 stand-in on the inputs of the GPU cases -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(B, S, hidden, seed, n_updates):
    """(weights, the C oracle's two gradients on the case's first tested minibatch): shared by the solvers' cases of one shape"""
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


def _warm_state(solver, hp, w, wt, g, s32):
    """WARMUP float32 steps under the case's gradient: histories of real magnitude"""
    st = R.State(w, np.zeros_like(w), np.zeros_like(w), wt)
    for _ in range(SL.WARMUP):
        st = R.simulate32(solver, hp, st, g, True, s32)
    return st


@pytest.mark.parametrize("name", [c.name for c in SL.CASES])
def test_simulated_kernel_is_accepted_on_the_gpu_cases(name):
    sc = SL.CASE_BY_NAME[name]
    case = sc.case
    w, g = _inputs(case.B, case.S, case.hidden, case.seed, case.n_updates)
    lays, hps = _layouts(case), SL.hypers(sc)
    for net in (0, 1):
        hp, lay = hps[net], lays[net]
        assert lay.dense == w[net].size
        ds = A.delta_s(A.depth_update(lay, case.precision))
        s32 = A.scale32(hp, g[net])
        before = _warm_state(sc.solver, hp, w[net], w[net + 2], g[net], s32)
        if sc.solver not in R.TWO_HISTORIES:
            assert not before.v.any()
        for soft in (True, False):
            after = R.simulate32(sc.solver, hp, before, g[net], soft, s32)
            r = R.check("%s net %d" % (name, net), sc.solver, hp, lay, before, g[net], after, soft, ds)
            assert (r["s_ref"] < 1) == (0 <= case.clip < 1e3), (name, net, r)
            assert max(r["h"], r["h2"], r["step"], r["target"]) <= 1.0
            print("SOLVERSIM %-32s net %d soft %d  h %.3f h2 %.3f step %.3f target %.3f  s_ref %.4e s_err %.2e ds %.2e"
                  % (name, net, soft, r["h"], r["h2"], r["step"], r["target"], r["s_ref"], r["s_err"], r["ds"]))


def test_adam_delegates_to_adam_ref():
    sc = SL.CASE_BY_NAME["SGD_eager"]
    case = sc.case
    w, g = _inputs(case.B, case.S, case.hidden, case.seed, case.n_updates)
    hp = R.hyper(1e-3, clip=case.clip, tau=0.25)
    lay = _layouts(case)[1]
    rng = np.random.default_rng(3)
    before = R.State(w[1], rng.normal(0, 1e-4, w[1].size).astype(F32), (rng.uniform(0, 1, w[1].size) ** 4 * 1e-6).astype(F32), w[3])
    after = R.simulate32("Adam", hp, before, g[1], True, A.scale32(hp, g[1]), t=3)
    ds = A.delta_s(A.depth_update(lay))
    r = R.check("adam", "Adam", hp, lay, before, g[1], after, True, ds, t=3)
    assert r == dict(A.check("adam", R.adam_hyper(hp), lay, before, g[1], after, 3, True, ds), h=r["m"], h2=r["v"])
    with pytest.raises(AssertionError, match="margin"):
        R.check("adam t off by one", "Adam", hp, lay, before, g[1], after, True, ds, t=4)


# ---- 3. planted faults ------------------------------------------------------------------------------------------------------------------------
def _base(solver, soft=True):
    sc = SL.CASE_BY_NAME[solver + "_eager"]
    case = sc.case
    w, g = _inputs(case.B, case.S, case.hidden, case.seed, case.n_updates)
    hp = SL.hypers(sc)[1]._replace(tau=F32(0.25))
    lay = _layouts(case)[1]
    s32 = A.scale32(hp, g[1])
    assert s32 < 1
    before = _warm_state(solver, hp, w[1], w[3], g[1], s32)
    return lay, hp, before, g[1], s32, A.delta_s(A.depth_update(lay))


def _expect(tag, solver, lay, hp, before, g, after, soft, ds, what):
    with pytest.raises(AssertionError, match="margin") as e:
        R.check(tag, solver, hp, lay, before, g, after, soft, ds)
    assert what in str(e.value), (tag, str(e.value))
    print("%-44s %s" % (tag, str(e.value).splitlines()[0]))


def test_planted_faults_are_rejected():
    for solver, fault, what in (("Nesterov", "nesterov_as_sgd", "step"), ("RMSProp", "delta_inside_root", "step"), ("AdaGrad", "adagrad_decay", "history 1"),
                                ("AdaDelta", "adadelta_swapped", "history"), ("AdaDelta", "adadelta_lr_first", "history 2"),
                                ("SGD", "touch_h2", "single-history"), ("RMSProp", "touch_h2", "single-history"), ("SGD", "stale_target_row", "target"),
                                ("AdaDelta", "stale_target_row", "target")):
        lay, hp, before, g, s32, ds = _base(solver)
        R.check("good", solver, hp, lay, before, g, R.simulate32(solver, hp, before, g, True, s32), True, ds)
        _expect("%s: %s" % (solver, fault), solver, lay, hp, before, g, R.simulate32(solver, hp, before, g, True, s32, fault=fault), True, ds, what)
    # delta inside the root, where delta matters: histories far below delta^2 are not what training produces; a larger delta shows it on every element
    lay, hp, before, g, s32, ds = _base("RMSProp")
    hp6 = hp._replace(delta=F32(1e-4))
    _expect("RMSProp: delta 1e-4 inside the root", "RMSProp", lay, hp6, before, g, R.simulate32("RMSProp", hp6, before, g, True, s32, fault="delta_inside_root"), True, ds, "step")
    for solver in SL.NEW:
        lay, hp, before, g, s32, ds = _base(solver)
        # a clip scale of 1 where the norm exceeds the clip
        _expect("%s: clip scale 1" % solver, solver, lay, hp, before, g, R.simulate32(solver, hp, before, g, True, F32(1)), True, ds, "applied clip scale")
        # the clip scale off by 4 delta_s
        s = F32(F64(s32) * (1 + 4 * ds))
        _expect("%s: scale off by 4 delta_s" % solver, solver, lay, hp, before, g, R.simulate32(solver, hp, before, g, True, s), True, ds, "applied clip scale")
        # the target against its switch
        good, off = R.simulate32(solver, hp, before, g, True, s32), R.simulate32(solver, hp, before, g, False, s32)
        _expect("%s: target moved, switch off" % solver, solver, lay, hp, before, g, good, False, ds, "while the switch is off")
        _expect("%s: target not moved, switch on" % solver, solver, lay, hp, before, g, off, True, ds, "target")
        # one float4 left unstepped
        one = R.State(*(x.copy() for x in good))
        for a, b in zip(one, before):
            a[1000:1004] = b[1000:1004]
        _expect("%s: one float4 unstepped" % solver, solver, lay, hp, before, g, one, True, ds, "history 1")


# ---- 4. the configuration surface ----------------------------------------------------------------------------------------------------------------
def _cfg(pkg, **kw):
    lib = pkg.capi.load()
    cfg = pkg.capi.Config()
    lib.dqnhip_default_config(C.byref(cfg), 59)
    cfg.num_hidden = 2
    cfg.hidden[0], cfg.hidden[1] = 64, 128
    for k, v in kw.items():
        setattr(cfg, k, v)
    return lib, cfg


def test_defaults_names_and_struct_size(pkg):
    lib, cfg = _cfg(pkg)
    assert cfg.struct_size == C.sizeof(pkg.capi.Config)
    assert cfg.solver_type == 0 and pkg.capi.SOLVERS[0] == "Adam"
    assert cfg.rms_decay == F32(0.99)
    assert [lib.dqnhip_solver_name(i) for i in range(6)] == [s.encode() for s in R.SOLVERS] == [s.encode() for s in pkg.capi.SOLVERS]
    assert lib.dqnhip_solver_name(-1) is None and lib.dqnhip_solver_name(6) is None
    assert lib.dqnhip_grad_arena_bytes(C.byref(cfg)) > 0
    # a zero-filled pair of new fields is an Adam learner
    lib, cfg = _cfg(pkg, solver_type=0, rms_decay=0.0)
    assert lib.dqnhip_grad_arena_bytes(C.byref(cfg)) > 0


@pytest.mark.parametrize("solver", SL.NEW)
def test_each_solver_is_accepted(pkg, solver):
    lib, cfg = _cfg(pkg, solver_type=R.SOLVERS.index(solver), momentum=SL.HYPER[solver]["momentum"])
    assert lib.dqnhip_grad_arena_bytes(C.byref(cfg)) > 0, lib.dqnhip_last_error()


@pytest.mark.parametrize("kw,message", [
    (dict(solver_type=3), b"Momentum cannot be used with AdaGrad."),
    (dict(solver_type=4), b"Momentum cannot be used with RMSProp."),
    (dict(solver_type=4, momentum=0.0, rms_decay=1.0), b"rms_decay"),
    (dict(solver_type=4, momentum=0.0, rms_decay=-0.1), b"rms_decay"),
    (dict(solver_type=4, momentum=0.0, rms_decay=float("nan")), b"rms_decay"),
    (dict(solver_type=6), b"unknown solver_type"),
    (dict(solver_type=-1), b"unknown solver_type"),
    (dict(solver_type=1, dp_world=2), b"SGD"),
    (dict(solver_type=5, dp_world=2), b"AdaDelta"),
])
def test_refusals(pkg, kw, message):
    lib, cfg = _cfg(pkg, **kw)
    assert lib.dqnhip_grad_arena_bytes(C.byref(cfg)) == 0
    assert message in lib.dqnhip_last_error(), lib.dqnhip_last_error()
    if "dp_world" in kw:
        assert b"dp_world" in lib.dqnhip_last_error()


def test_python_constructor_refuses_an_unknown_name(pkg):
    with pytest.raises(pkg.DQNFatal, match="Unknown solver type: Bogus"):
        pkg.DQN(59, solver="Bogus")
