"""-native_state through the adaptor (include/dqn.hpp + dqn_dropin.cpp, tests/cpp/state_smoke.cpp): a run that is stopped after its
snapshot at iteration 20 and resumed by a NEW process through the driver's own sequence (FindLatestSnapshot, RestoreActorSolver,
RestoreCriticSolver, LoadReplayMemory; src/dqn_main.cpp:213-220, 268-286) ends, twenty updates later, with the digest of the run
that never stopped, and logs the same "[Agent0] Critic / Actor Iteration" lines from iteration 21 on, text for text.  Without the flag
the digests differ (the targets are re-cloned, the engine restarts), no .learnerstate file is written and no log line mentions one.

-device_sampling -seed 0: "-seed 0" seeds from the clock, so no second process can repeat the first twenty updates of the
uninterrupted run.  There the stopped run IS the uninterrupted one: it keeps its snapshots (-remove_old_snapshots=false) and the
files of iteration 20 are copied to a directory of their own, which is what a process killed after that snapshot leaves."""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_dropin", "state_smoke")
ARGS = ["-memory", "5000", "-memory_threshold", "50", "-loss_display_iter", "7", "-minibatch", "32", "-snapshot_freq", "20"]

pytestmark = pytest.mark.gpu


def _build(pkg):
    lib = pkg.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "shim"),
           "-o", EXE, os.path.join(ROOT, "tests", "cpp", "state_smoke.cpp"), os.path.join(ROOT, "dqn-hfo_amd", "csrc", "dqn_dropin.cpp"),
           lib, "-Wl,-rpath," + os.path.dirname(lib)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def _agent_lines(stderr, first_iter=0):
    lines = [l[l.index("[Agent"):] for l in stderr.splitlines() if "[Agent" in l and " Iteration " in l]
    return [l for l in lines if int(l.split(" Iteration ")[1].split(",")[0]) >= first_iter]


def _run(exe, prefix, extra):
    r = subprocess.run([exe] + ARGS + ["-prefix", prefix] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "state smoke OK" in r.stdout, (extra, r.returncode, r.stdout, r.stderr)
    digest = [l for l in r.stdout.splitlines() if l.startswith("digest:")]
    assert len(digest) == 1, r.stdout
    return digest[0], r.stderr


def _three_runs(exe, tmp_path, name, mode, native):
    flags = mode + (["-native_state"] if native else [])
    dirs = [tmp_path / ("%s_run%d" % (name, k)) for k in (1, 2)]
    for d in dirs:
        d.mkdir()
    p1, p2 = (str(d / "agent0") for d in dirs)
    if "-seed" in mode and mode[mode.index("-seed") + 1] == "0":
        full, full_err = _run(exe, p1, flags + ["-stop_at", "40", "-remove_old_snapshots=false"])
        at20 = glob.glob(p1 + "*_iter_20.*")
        assert len(at20) >= 5, at20
        for f in at20:
            shutil.copy(f, str(dirs[1]))
    else:
        full, full_err = _run(exe, p1, flags + ["-stop_at", "40"])
        half, _ = _run(exe, p2, flags + ["-stop_at", "20"])
        assert "actor_iter 20 critic_iter 20" in half
    assert "actor_iter 40 critic_iter 40 memory_size 120" in full
    resumed, resumed_err = _run(exe, p2, flags + ["-stop_at", "40", "-resume"])
    assert "actor_iter 40 critic_iter 40" in resumed
    return full, full_err, resumed, resumed_err, dirs


@pytest.mark.parametrize("name,mode", [("host", ["-seed", "7"]), ("per", ["-seed", "7", "-prioritized_replay"]),
                                       ("device", ["-device_sampling", "-seed", "0"])])
def test_resumed_run_equals_the_uninterrupted_one(pkg, gpu, tmp_path, name, mode):
    exe = _build(pkg)
    full, full_err, resumed, resumed_err, dirs = _three_runs(exe, tmp_path, name, mode, native=True)
    assert resumed == full, (full, resumed)
    want, got = _agent_lines(full_err, 21), _agent_lines(resumed_err, 21)
    assert len(want) == 2 * 3 and got == want, (want, got)          # iterations 21, 28, 35
    assert "-native_state: resumed from" in resumed_err and "Skipping" in resumed_err and ".replaymemory: the learner state already restored" in resumed_err
    # the reference's files are there as always, the learner state beside them; older ones went with the .replaymemory files
    left = sorted(os.path.basename(f) for f in glob.glob(str(dirs[1] / "agent0*")))
    assert left == ["agent0_actor_iter_40.caffemodel", "agent0_actor_iter_40.solverstate", "agent0_critic_iter_40.caffemodel",
                    "agent0_critic_iter_40.solverstate", "agent0_iter_40.learnerstate", "agent0_iter_40.replaymemory"], left
    info = pkg.state_info(str(dirs[1] / "agent0_iter_40.learnerstate"))
    assert (info["actor_iter"], info["critic_iter"], info["has_memory"], info["has_per"]) == (40, 40, 1, int("-prioritized_replay" in mode))
    assert pkg.state_user(str(dirs[1] / "agent0_iter_40.learnerstate")).startswith(b"dqn_dropin_state 1\n")


def test_without_the_flag_the_resume_loses_state_and_nothing_new_appears(pkg, gpu, tmp_path):
    exe = _build(pkg)
    full, full_err, resumed, resumed_err, dirs = _three_runs(exe, tmp_path, "off", ["-seed", "7"], native=False)
    assert resumed != full                                       # the test can see the loss
    for d in dirs:
        assert not glob.glob(str(d / "*.learnerstate*"))
    for err in (full_err, resumed_err):
        assert "learnerstate" not in err and "native_state" not in err and "learner state" not in err
    # ... and the flag with -snapshot_memory=false: the state file carries no memory, the .replaymemory load is not skipped
    d = tmp_path / "nomem"
    d.mkdir()
    _run(exe, str(d / "agent0"), ["-seed", "7", "-native_state", "-snapshot_memory=false", "-stop_at", "20"])
    assert pkg.state_info(str(d / "agent0_iter_20.learnerstate"))["has_memory"] == 0
    assert not glob.glob(str(d / "*.replaymemory"))
