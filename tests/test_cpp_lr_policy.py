"""Caffe's lr policies and weight decay through the adaptor (include/dqn.hpp + dqn_dropin.cpp, tests/cpp/lr_policy_smoke.cpp).  The solver
parameters are filled as the reference's driver fills them (-lr_policy and -max_iter reach SolverParameter, src/dqn_main.cpp:249-256); the
adaptor's own flags supply the policy's other parameters and the decay.  Without a GPU: the refusals abort in the adaptor's constructor
with the library's wording — the unchanged driver's `-lr_policy step` and nothing else stops on stepsize.  On the GPU: the flags reach
the learner's configuration, and `-lr_policy exp -lr_gamma ...` with a decay ends, after six updates on given weights, replay memory and
indices, on the bits of the Python learner with the same configuration."""
import os
import re
import subprocess

import numpy as np
import pytest

import optimizer_forms_lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_dropin", "lr_policy_smoke")
ARGS = ["-seed", "7", "-memory", "512", "-memory_threshold", "50", "-loss_display_iter", "1000", "-minibatch", "32", "-snapshot_freq", "100000"]
HIDDEN = (128, 128, 128, 128)


def _build(pkg):
    lib = pkg.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "shim"),
           "-o", EXE, os.path.join(ROOT, "tests", "cpp", "lr_policy_smoke.cpp"), os.path.join(ROOT, "dqn-hfo_amd", "csrc", "dqn_dropin.cpp"),
           lib, "-Wl,-rpath," + os.path.dirname(lib)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def _run(exe, extra, tmp_path):
    return subprocess.run([exe] + ARGS + ["-prefix", str(tmp_path / "agent0")] + extra, capture_output=True, text=True, timeout=300)


def test_refusals_abort_in_the_constructor(pkg, tmp_path):
    """no device needed: the adaptor's CHECKs, and the library's validator (which runs before dqnhip_create looks for a device)"""
    exe = _build(pkg)
    for extra, what in (
            (["-policy", "step"], "lr_policy step: stepsize > 0"),                                   # the unchanged driver's -lr_policy step and nothing else
            (["-policy", "step", "-lr_stepsize", "100"], "lr_policy step: gamma > 0"),
            (["-policy", "exp"], "lr_policy exp: gamma > 0"),
            (["-policy", "multistep", "-lr_gamma", "0.1"], "lr_policy multistep: 1 to 16 stepvalues"),
            (["-policy", "multistep", "-lr_gamma", "0.1", "-lr_stepvalues", "5,3"], "strictly increasing"),
            (["-policy", "multistep", "-lr_gamma", "0.1", "-lr_stepvalues", "5,x"], "-lr_stepvalues: 'x' is not an integer"),
            (["-policy", "multistep", "-lr_gamma", "0.1", "-lr_stepvalues", ",".join(str(i) for i in range(1, 18))], "1 to 16 stepvalues"),
            (["-policy", "poly", "-solver_max_iter", "0"], "lr_policy poly: max_iter > 0"),
            (["-policy", "bogus"], "Unknown learning rate policy: bogus"),
            (["-weight_decay", "-0.5"], "weight_decay >= 0"),
            (["-weight_decay", "0.01", "-regularization_type", "L3"], "Unknown regularization type: L3"),
            (["-policy", "exp", "-sp_gamma", "0.5", "-sp_critic_gamma", "0.25"], "actor and critic solvers must share lr_policy"),
            (["-policy", "exp", "-lr_gamma", "0.5", "-debug_info_iter", "10"], "-debug_info_iter is not available with -lr_policy exp"),
            (["-weight_decay", "0.01", "-dp_world", "2", "-dp_rendezvous", str(tmp_path / "rv")], "single-learner options")):
        r = _run(exe, extra, tmp_path)
        assert r.returncode != 0 and "lr policy smoke OK" not in r.stdout, (extra, r.returncode, r.stdout)
        assert what in r.stderr, (extra, r.stderr[-2000:])


@pytest.mark.gpu
def test_flags_reach_the_learner(pkg, gpu, tmp_path):
    exe = _build(pkg)
    for extra, want in (
            ([], "config: lr_policy fixed gamma 0 power 0 stepsize 0 max_iter 10000000 stepvalues weight_decay 0 regularization L2"),
            (["-policy", "step", "-lr_gamma", "0.5", "-lr_stepsize", "1000"], "lr_policy step gamma 0.5 power 0 stepsize 1000 "),
            (["-policy", "inv", "-lr_gamma", "0.0001", "-lr_power", "0.75"], "lr_policy inv gamma 9.99999975e-05 power 0.75 "),
            (["-policy", "multistep", "-lr_gamma", "0.1", "-lr_stepvalues", "1000,5000,20000"], "lr_policy multistep gamma 0.100000001 power 0 stepsize 0 max_iter 10000000 stepvalues 1000,5000,20000 "),
            (["-policy", "poly", "-lr_power", "2", "-solver_max_iter", "5000"], "lr_policy poly gamma 0 power 2 stepsize 0 max_iter 5000 "),
            (["-policy", "sigmoid", "-lr_gamma", "-0.001", "-lr_stepsize", "4000"], "lr_policy sigmoid gamma -0.00100000005 power 0 stepsize 4000 "),
            (["-weight_decay", "0.0005", "-regularization_type", "L1"], "weight_decay 0.000500000024 regularization L1"),
            # the SolverParameter fields themselves (a caller of the adaptor that fills them), and a flag over them
            (["-policy", "step", "-sp_gamma", "0.25", "-sp_stepsize", "7", "-sp_weight_decay", "0.125"], "lr_policy step gamma 0.25 power 0 stepsize 7 "),
            (["-policy", "step", "-sp_gamma", "0.25", "-sp_stepsize", "7", "-lr_stepsize", "9", "-sp_weight_decay", "0.125"], "stepsize 9 max_iter 10000000 stepvalues weight_decay 0.125 regularization L2")):
        r = _run(exe, extra, tmp_path)
        assert r.returncode == 0 and "lr policy smoke OK" in r.stdout, (extra, r.returncode, r.stdout, r.stderr[-2000:])
        assert want in r.stdout, (extra, r.stdout)


@pytest.mark.gpu
@pytest.mark.parametrize("solver,extra,kw", [
    ("Adam", ["-policy", "exp", "-lr_gamma", "0.5"], dict(lr_policy="exp", lr_gamma=0.5)),
    ("RMSProp", ["-policy", "exp", "-lr_gamma", "0.5", "-weight_decay", "0.01", "-regularization_type", "L1"],
     dict(lr_policy="exp", lr_gamma=0.5, weight_decay=0.01, regularization="L1")),
])
def test_adaptor_and_python_learner_end_on_the_same_weights(pkg, gpu, tmp_path, solver, extra, kw):
    n_updates = 6
    case = L._case("adaptor", "eager", 32, 59, HIDDEN, seed=77, n_updates=n_updates)
    inp = L.make_inputs(case)
    d = tmp_path / "io"
    d.mkdir()
    for net in range(4):
        inp["w"][net].tofile(d / ("w%d.bin" % net))
    for k in ("s", "a", "r", "mc", "nx", "term"):
        np.ascontiguousarray(inp[k]).tofile(d / (k + ".bin"))
    inp["idx"].astype(np.int32).tofile(d / "idx.bin")
    momentum = 0.0 if solver == "RMSProp" else 0.95
    r = _run(_build(pkg), ["-solver_type", solver, "-solver_momentum", str(momentum), "-dir", str(d), "-updates", str(n_updates)] + extra, tmp_path)
    assert r.returncode == 0 and "lr policy smoke OK" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
    rates = [tuple(float(x) for x in m.groups()) for m in re.finditer(r"update \d+: rates (\S+) (\S+) ", r.stdout)]
    assert len(rates) == n_updates and all(abs(a / (1e-5 * 0.5 ** u) - 1) < 1e-6 and abs(c / (1e-3 * 0.5 ** u) - 1) < 1e-6 for u, (a, c) in enumerate(rates)), rates
    py = pkg.DQN(59, minibatch=32, hidden=HIDDEN, memory=512, solver=solver, momentum=momentum, **kw)
    try:
        for net in range(4):
            py.set_params(net, inp["w"][net])
        py.add_transitions_arrays(inp["s"], inp["a"], inp["r"], inp["mc"], inp["nx"], inp["term"])
        for row in inp["idx"]:
            py.UpdateActorCritic(row)
        for net in range(4):
            got = np.fromfile(d / ("out%d.bin" % net), np.float32)
            assert np.array_equal(got.view(np.uint32), py.get_params(net).view(np.uint32)), (solver, net)
            assert (got != inp["w"][net]).any()
    finally:
        py.close()
