"""-native_state_async and -native_state_only_memory through the adaptor (include/dqn.hpp + dqn_dropin.cpp), with tests/cpp/state_smoke.cpp
unchanged and the scheme of tests/test_cpp_state.py: a run stopped at iteration 20 and resumed by a new process ends, at iteration
40, on the digest and the log lines of the run that never stopped.  The yardstick of the asynchronous save is the synchronous one:
the .learnerstate a run with -native_state_async leaves at iteration 40 is, byte for byte, the one a run without it leaves."""
import glob
import os
import subprocess

import pytest

from test_cpp_state import ARGS, _agent_lines, _build, _run, _three_runs

pytestmark = pytest.mark.gpu

SEED = ["-seed", "7"]
FILES_40 = ["agent0_actor_iter_40.caffemodel", "agent0_actor_iter_40.solverstate", "agent0_critic_iter_40.caffemodel",
            "agent0_critic_iter_40.solverstate", "agent0_iter_40.learnerstate"]


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _left(d):
    return sorted(os.path.basename(f) for f in glob.glob(str(d / "agent0*")))


def test_async_resume_equals_the_uninterrupted_run_and_the_synchronous_file(pkg, gpu, tmp_path):
    exe = _build(pkg)
    mode = SEED + ["-native_state", "-native_state_async", "-remove_old_snapshots"]
    full, full_err, resumed, resumed_err, dirs = _three_runs(exe, tmp_path, "async", mode, native=False)
    assert resumed == full, (full, resumed)
    want, got = _agent_lines(full_err, 21), _agent_lines(resumed_err, 21)
    assert len(want) == 2 * 3 and got == want, (want, got)
    assert "-native_state: resumed from" in resumed_err and "Snapshotting learner state to" in full_err
    # -remove_old_snapshots: the file of iteration 20 went at the join of the save that superseded it, the newest is complete
    for d in dirs:
        assert _left(d) == sorted(FILES_40 + ["agent0_iter_40.replaymemory"]), _left(d)
        assert not glob.glob(str(d / "*.tmp"))
        info = pkg.state_info(str(d / "agent0_iter_40.learnerstate"))
        assert (info["actor_iter"], info["critic_iter"], info["has_memory"], info["memory_size"]) == (40, 40, 1, 120)
    # the synchronous save of the same run is the yardstick
    sync_dir = tmp_path / "sync"
    sync_dir.mkdir()
    sync, _ = _run(exe, str(sync_dir / "agent0"), SEED + ["-native_state", "-stop_at", "40"])
    assert sync == full
    assert _read(str(dirs[0] / "agent0_iter_40.learnerstate")) == _read(str(sync_dir / "agent0_iter_40.learnerstate"))


@pytest.mark.parametrize("extra", [[], ["-native_state_async"]], ids=["sync", "async"])
def test_only_memory_writes_no_replaymemory_and_still_resumes(pkg, gpu, tmp_path, extra):
    exe = _build(pkg)
    mode = SEED + ["-native_state", "-native_state_only_memory"] + extra
    full, full_err, resumed, resumed_err, dirs = _three_runs(exe, tmp_path, "only", mode, native=False)
    assert resumed == full, (full, resumed)
    assert _agent_lines(resumed_err, 21) == _agent_lines(full_err, 21)
    for d in dirs:
        assert _left(d) == FILES_40, _left(d)
    for err in (full_err, resumed_err):
        assert "Snapshotting memory to" not in err and "Loading replay memory" not in err
    assert "(with the replay memory: replay_mem_size = " in resumed_err
    # the same learner as without the flag
    plain_dir = tmp_path / "plain"
    plain_dir.mkdir()
    plain, _ = _run(exe, str(plain_dir / "agent0"), SEED + ["-native_state", "-stop_at", "40"])
    assert plain == full


def test_each_flag_needs_native_state(pkg, gpu, tmp_path):
    exe = _build(pkg)
    for flag in ("-native_state_async", "-native_state_only_memory"):
        r = subprocess.run([exe] + ARGS + ["-prefix", str(tmp_path / "agent0"), "-seed", "7", flag, "-stop_at", "20"], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "state smoke OK" not in r.stdout, (flag, r.returncode, r.stdout)
        assert "Check failed" in r.stderr and flag + " needs -native_state" in r.stderr, r.stderr
    assert not glob.glob(str(tmp_path / "agent0*"))
