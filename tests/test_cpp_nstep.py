"""-n_step / -n_step_validate_on_load through the adaptor (include/dqn.hpp + dqn_dropin.cpp, tests/cpp/nstep_smoke.cpp): with -n_step 3
the episode loop trains its 40 updates on n-step targets (Update() goes through the unchained dqnhip_update on the indices
random_engine draws, so the engine's call order is the reference's), the log lines keep the format of src/dqn.cpp:806-818, and the
flag is CHECKed against -deferred_updates, -pipelined_stats and -dp_world > 1 in the constructor, before the device is touched."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_dropin", "nstep_smoke")
ARGS = ["-seed", "7", "-memory", "5000", "-memory_threshold", "50", "-loss_display_iter", "7", "-minibatch", "32", "-snapshot_freq", "100000"]


def _build(pkg):
    lib = pkg.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "shim"),
           "-o", EXE, os.path.join(ROOT, "tests", "cpp", "nstep_smoke.cpp"), os.path.join(ROOT, "dqn-hfo_amd", "csrc", "dqn_dropin.cpp"),
           lib, "-Wl,-rpath," + os.path.dirname(lib)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def _agent_lines(stderr):
    return [l[l.index("[Agent"):] for l in stderr.splitlines() if "[Agent" in l and "Seeding" not in l and "n-step returns" not in l and "[Memory]" not in l]


def _run(exe, extra, tmp_path):
    r = subprocess.run([exe] + ARGS + ["-prefix", str(tmp_path / "agent0")] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (extra, r.returncode, r.stdout, r.stderr)
    assert "nstep smoke OK" in r.stdout and "digest: actor_iter 40 critic_iter 40 memory_size 120" in r.stdout, r.stdout
    return r


def _check_format(lines):
    assert len(lines) == 2 * (40 // 7), lines
    for i, l in enumerate(lines):
        it = 7 * (i // 2 + 1)
        want = r"\[Agent0\] Critic Iteration %d, loss = \S+$" % it if i % 2 == 0 else r"\[Agent0\] Actor Iteration %d, avg_q_value = \S+$" % it
        assert re.match(want, l), (i, l)
        assert all(c in "0123456789.e+-" for c in l.split("= ")[1]), l      # a finite number


@pytest.mark.gpu
def test_flag_trains_and_keeps_the_log_format(pkg, gpu, tmp_path):
    exe = _build(pkg)
    off = _run(exe, [], tmp_path)
    _check_format(_agent_lines(off.stderr))
    assert "n-step returns" not in off.stderr
    # -n_step 1 is off: nothing is called, the run is the plain one
    assert _run(exe, ["-n_step", "1"], tmp_path).stdout == off.stdout
    for extra in ([], ["-hip_graph=false"], ["-prioritized_replay"], ["-n_step_validate_on_load", "-reload_memory"]):
        on = _run(exe, ["-n_step", "3"] + extra, tmp_path)
        _check_format(_agent_lines(on.stderr))
        assert "[Agent0] n-step returns: n = 3" in on.stderr
        if "-n_step_validate_on_load" in extra:
            assert "[Agent0] [Memory] 120 transitions validated" in on.stderr
    # other targets, other numbers; the same run twice gives the same ones
    on1, on2 = _run(exe, ["-n_step", "3"], tmp_path), _run(exe, ["-n_step", "3"], tmp_path)
    assert on1.stdout == on2.stdout and on1.stdout != off.stdout


def test_flag_is_checked_against_deferred_pipelined_and_data_parallel(pkg, tmp_path):
    """the CHECKs fire in the constructor, before dqnhip_create: no device needed"""
    exe = _build(pkg)
    for extra, what in ((["-n_step", "3", "-deferred_updates=true"], "-n_step cannot be combined with -deferred_updates"),
                        (["-n_step", "3", "-pipelined_stats=true"], "-n_step cannot be combined with -pipelined_stats"),
                        (["-n_step", "3", "-dp_world", "2", "-dp_rendezvous", str(tmp_path / "rv")], "-n_step is a single-learner option"),
                        (["-n_step", "3", "-evaluate_memory_freq", "10"], "-n_step cannot be combined with -evaluate_memory_freq"),
                        (["-n_step", "65"], "-n_step must lie in [1, 64]"),
                        (["-n_step", "0"], "-n_step must lie in [1, 64]")):
        r = subprocess.run([exe] + ARGS + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "nstep smoke OK" not in r.stdout, (extra, r.returncode, r.stdout)
        assert "Check failed" in r.stderr and what in r.stderr, (extra, r.stderr)
