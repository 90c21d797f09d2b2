"""-target_noise_sigma / -target_noise_clip through the adaptor (include/dqn.hpp + dqn_dropin.cpp), driven by tests/cpp/nstep_smoke.cpp's
episode loop with bursts of Update(): with the flag on the 40 updates train on smoothed targets (Update() goes through the unchained
dqnhip_update on the indices random_engine draws), the log lines keep their format, the run is repeatable and differs from the plain
one; 0 is off.  The flag is CHECKed against -deferred_updates, -pipelined_stats, -dp_world > 1 and -precision fp16 in the
constructor, before the device is touched."""
import os
import subprocess

import pytest

from test_cpp_nstep import ARGS, ROOT, _agent_lines, _check_format

EXE = os.path.join(ROOT, "tests", "cpp", "_dropin", "target_noise_smoke")


def _build(pkg):
    lib = pkg.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "shim"),
           "-o", EXE, os.path.join(ROOT, "tests", "cpp", "nstep_smoke.cpp"), os.path.join(ROOT, "dqn-hfo_amd", "csrc", "dqn_dropin.cpp"),
           lib, "-Wl,-rpath," + os.path.dirname(lib)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def _run(exe, extra, tmp_path):
    r = subprocess.run([exe] + ARGS + ["-prefix", str(tmp_path / "agent0")] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (extra, r.returncode, r.stdout, r.stderr)
    assert "nstep smoke OK" in r.stdout and "digest: actor_iter 40 critic_iter 40 memory_size 120" in r.stdout, r.stdout
    return r


@pytest.mark.gpu
def test_flag_trains_and_keeps_the_log_format(pkg, gpu, tmp_path):
    exe = _build(pkg)
    off = _run(exe, [], tmp_path)
    assert "target smoothing" not in off.stderr
    assert _run(exe, ["-target_noise_sigma", "0"], tmp_path).stdout == off.stdout            # 0 is off: nothing is called
    for extra in ([], ["-hip_graph=false"], ["-prioritized_replay"], ["-n_step", "3"], ["-target_noise_clip", "0"]):
        on = _run(exe, ["-target_noise_sigma", "0.1"] + extra, tmp_path)
        _check_format([l for l in _agent_lines(on.stderr) if "target smoothing" not in l])
        assert "[Agent0] target smoothing: sigma = 0.1" in on.stderr
    on1, on2 = _run(exe, ["-target_noise_sigma", "0.1"], tmp_path), _run(exe, ["-target_noise_sigma", "0.1"], tmp_path)
    assert on1.stdout == on2.stdout and on1.stdout != off.stdout


def test_flag_is_checked_in_the_constructor(pkg, tmp_path):
    exe = _build(pkg)
    for extra, what in ((["-target_noise_sigma", "0.1", "-deferred_updates=true"], "-target_noise_sigma cannot be combined with -deferred_updates"),
                        (["-target_noise_sigma", "0.1", "-pipelined_stats=true"], "-target_noise_sigma cannot be combined with -pipelined_stats"),
                        (["-target_noise_sigma", "0.1", "-dp_world", "2", "-dp_rendezvous", str(tmp_path / "rv")], "-target_noise_sigma is a single-learner option"),
                        (["-target_noise_sigma", "0.1", "-precision", "fp16"], "-target_noise_sigma needs -precision fp32"),
                        (["-target_noise_sigma", "-1"], "-target_noise_sigma must be >= 0"),
                        (["-target_noise_sigma", "0.1", "-target_noise_clip", "-1"], "-target_noise_clip must be >= 0")):
        r = subprocess.run([exe] + ARGS + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "nstep smoke OK" not in r.stdout, (extra, r.returncode, r.stdout)
        assert "Check failed" in r.stderr and what in r.stderr, (extra, r.stderr)
