"""-deferred_updates through the adaptor (include/dqn.hpp + dqn_dropin.cpp): Update() only draws its indices, sixteen at a time run as
one multi-update graph, and the log lines / snapshots are replayed when the pairs are collected.  Everything the driver can observe
- iteration counters, weights (through Q values and actions), log text, snapshot names - must be what the blocking form gives."""
import glob
import os
import re
import subprocess

import pytest

import test_cpp_adaptor

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE2 = os.path.join(ROOT, "tests", "cpp", "_dropin", "deferred_smoke")


def _log_lines(stderr):
    return [l[l.index("[Agent"):] for l in stderr.splitlines() if "[Agent" in l and ("Critic Iteration" in l or "Actor Iteration" in l)]


def _both(cmd):
    runs = []
    for flag in ("-deferred_updates=true", "-deferred_updates=false"):
        r = subprocess.run(cmd + [flag], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (flag, r.returncode, r.stdout, r.stderr)
        runs.append(r)
    return runs


def test_adaptor_smoke_is_unchanged_by_the_flag(pkg, gpu):
    """submitting before SelectAction, AddTransitions, Snapshot, Restore*, sharing (deferral off from there on), UpdateActorCritic()"""
    exe = test_cpp_adaptor._build(pkg)
    on, off = _both([exe, "-seed", "7", "-memory", "5000", "-memory_threshold", "100", "-loss_display_iter", "3"])
    ok = [[l for l in r.stdout.splitlines() if "adaptor smoke OK" in l] for r in (on, off)]
    assert ok[0] == ok[1] and len(ok[0]) == 1, ok
    assert _log_lines(on.stderr) == _log_lines(off.stderr) and len(_log_lines(off.stderr)) >= 6


def test_long_bursts_with_snapshot_and_log_cadence_inside_graphs(pkg, gpu, tmp_path):
    """tests/cpp/deferred_smoke.cpp: bursts of 40 Update() calls, DQN::Benchmark(40) through the deferred path, one more burst"""
    lib = pkg.build()
    os.makedirs(os.path.dirname(EXE2), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "shim"),
           "-o", EXE2, os.path.join(ROOT, "tests", "cpp", "deferred_smoke.cpp"), os.path.join(ROOT, "dqn-hfo_amd", "csrc", "dqn_dropin.cpp"),
           lib, "-Wl,-rpath," + os.path.dirname(lib)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    prefix = str(tmp_path / "deferred_agent0")
    on, off = _both([EXE2, "-seed", "7", "-memory", "5000", "-memory_threshold", "100", "-loss_display_iter", "7", "-snapshot_freq", "25",
                     "-remove_old_snapshots=false", "-prefix", prefix])
    assert on.stdout == off.stdout, (on.stdout, off.stdout)
    assert "deferred smoke OK" in on.stdout and "digest: actor_iter 210 critic_iter 210 memory_size 300" in on.stdout
    # snapshots written mid-burst carry the iteration numbers the blocking form's carry: 25, 50, .. 150, then 201 - the first
    # Update() behind Benchmark(40), whose 40 updates (161 .. 200) do none of Update()'s bookkeeping in either form
    iters = sorted({int(m) for m in re.findall(r"_actor_iter_(\d+)\.solverstate", on.stdout)})
    assert iters == [25, 50, 75, 100, 125, 150, 201], on.stdout
    lines = _log_lines(off.stderr)
    assert _log_lines(on.stderr) == lines and len(lines) == 2 * (160 // 7 + 2)       # (+ 203, 210)
    for r in (on, off):
        assert "*** Benchmark begins ***" in r.stderr and "Average Update: " in r.stderr
    assert not glob.glob(prefix + "_*")                  # (the program removed them: RemoveFilesMatchingRegexp)


def test_unchanged_driver_learn_offline_leg(pkg, gpu, tmp_path):
    """the reference's unchanged driver binary (built only where the reference sources are present): a state saved by a short online
    run, then one -learn_offline leg of 40 updates (src/dqn_main.cpp:340-348) on a copy of it with and without the flag - the final
    .solverstate names are equal.  The command line is the one tests/test_dropin_driver.py uses."""
    import shutil
    from oracle import dropin_build as db
    if db.reference_present():
        db.build(pkg.build())                            # this tree's adaptor, whatever was there before
    elif not os.path.exists(db.EXE):
        pytest.skip("the driver binary oracle/_ref/dropin is built only where the reference sources are present")
    else:
        # a binary that travelled here has its own copy of dqn_dropin.cpp compiled in.  Whether that copy has the deferred path at all is
        # read off its import table, not off the flag under test: an adaptor from before this feature never calls
        # dqnhip_update_indexed_n and says nothing about it; one that does must know the flag, or the test fails below
        und = subprocess.run(["nm", "-D", "--undefined-only", db.EXE], capture_output=True, text=True).stdout
        if "dqnhip_update_indexed_n" not in und:
            pytest.skip("oracle/_ref/dropin/dqn predates the deferred path (no reference to dqnhip_update_indexed_n): rebuild it where the "
                        "reference sources are present")
    env = dict(os.environ, HFO_SHIM_P_END="0.05", HFO_SHIM_FRAMES="60", HFO_SHIM_FEATURES="59")

    def cmd(save, max_iter, extra):
        return [db.EXE, "-save", save, "-server_cmd", "true", "-seed", "3", "-memory", "20000", "-memory_threshold", "200",
                "-max_iter", str(max_iter), "-update_ratio", "0.5", "-evaluate_freq", "1000", "-repeat_games", "3", "-loss_display_iter", "50",
                "-snapshot_freq", "1000", "-explore", "100"] + extra

    base = tmp_path / "base"; base.mkdir()
    r = subprocess.run(cmd(str(base / "state"), 30, []), capture_output=True, text=True, timeout=300, env=env, cwd=str(base))
    assert r.returncode == 0, r.stderr[-3000:]
    it = max(int(f.split("_iter_")[1].split(".")[0]) for f in os.listdir(str(base)) if "_actor_iter_" in f and f.endswith(".solverstate"))
    names = []
    for flag in ("-deferred_updates=true", "-deferred_updates=false"):
        d = tmp_path / flag.strip("-").replace("=", "_")
        shutil.copytree(str(base), str(d))
        r = subprocess.run(cmd(str(d / "state"), it + 40, ["-learn_offline", flag]), capture_output=True, text=True, timeout=300, env=env, cwd=str(d))
        assert r.returncode == 0, (flag, r.stderr[-3000:])
        names.append(sorted(f for f in os.listdir(str(d)) if f.endswith(".solverstate")))
    assert names[0] == names[1], names
    assert "state_agent0_actor_iter_%d.solverstate" % (it + 40) in names[0], names
