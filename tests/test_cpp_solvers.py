"""SolverParameter::type through the adaptor (include/dqn.hpp + dqn_dropin.cpp, tests/cpp/solver_smoke.cpp) — what the reference
driver's -solver flag sets on both solvers (src/dqn_main.cpp:30, src/dqn.cpp:628-629): every Caffe type trains, snapshots, restores
into a second learner and continues; the combinations Caffe's solver constructors refuse abort with Caffe's wording, and an unknown
type aborts as Caffe's registry does — in the adaptor's constructor, before the device is touched."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_dropin", "solver_smoke")
ARGS = ["-seed", "7", "-memory", "5000", "-memory_threshold", "50", "-loss_display_iter", "1000", "-minibatch", "32", "-snapshot_freq", "100000"]


def _build(pkg):
    lib = pkg.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "shim"),
           "-o", EXE, os.path.join(ROOT, "tests", "cpp", "solver_smoke.cpp"), os.path.join(ROOT, "dqn-hfo_amd", "csrc", "dqn_dropin.cpp"),
           lib, "-Wl,-rpath," + os.path.dirname(lib)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def _run(exe, extra, tmp_path):
    return subprocess.run([exe] + ARGS + ["-prefix", str(tmp_path / "agent0")] + extra, capture_output=True, text=True, timeout=300)


@pytest.mark.gpu
@pytest.mark.parametrize("solver,momentum", [("Nesterov", "0.95"), ("SGD", "0.95"), ("AdaGrad", "0"), ("RMSProp", "0"), ("AdaDelta", "0.95"), ("Adam", "0.95")])
def test_type_trains_snapshots_restores_and_continues(pkg, gpu, tmp_path, solver, momentum):
    r = _run(_build(pkg), ["-solver_type", solver, "-solver_momentum", momentum], tmp_path)
    assert r.returncode == 0 and "solver smoke OK" in r.stdout, (solver, r.returncode, r.stdout, r.stderr)
    lines = dict(l.split(": ", 1) for l in r.stdout.splitlines() if ": actor_iter" in l)
    assert re.match(r"actor_iter 8 critic_iter 8 q:( \S+){4}$", lines["trained"]), lines
    assert lines["restored"] == lines["trained"]                      # the online nets, and both iterations
    assert re.match(r"actor_iter 12 critic_iter 12 q:", lines["trained+4"]) and lines["trained+4"] != lines["trained"]
    assert "nan" not in r.stdout and "inf" not in r.stdout
    # (the restored learner re-clones its targets, as the reference does: its next updates are not the trained learner's)
    assert re.match(r"actor_iter 12 critic_iter 12 q:( \S+){4}$", lines["restored+4"]), lines


def test_refusals_abort_with_caffes_wording(pkg, tmp_path):
    """the CHECKs fire in the constructor, before dqnhip_create: no device needed"""
    exe = _build(pkg)
    for extra, what in ((["-solver_type", "RMSProp", "-solver_momentum", "0.95"], "Momentum cannot be used with RMSProp."),
                        (["-solver_type", "AdaGrad", "-solver_momentum", "0.95"], "Momentum cannot be used with AdaGrad."),
                        (["-solver_type", "RMSProp", "-solver_momentum", "0", "-solver_rms_decay", "1.5"], "rms_decay"),
                        (["-solver_type", "Bogus"], "Unknown solver type: Bogus"),
                        (["-solver_type", "SGD", "-dp_world", "2", "-dp_rendezvous", str(tmp_path / "rv")], "-solver SGD is a single-learner option")):
        r = _run(exe, extra, tmp_path)
        assert r.returncode != 0 and "solver smoke OK" not in r.stdout, (extra, r.returncode, r.stdout)
        assert "Check failed" in r.stderr and what in r.stderr, (extra, r.stderr)
