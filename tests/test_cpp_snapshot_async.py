"""-snapshot_async through the adaptor (include/dqn.hpp + dqn_dropin.cpp), with tests/cpp/snapshot_async_smoke.cpp: over a short run with
two snapshots (iterations 20 and 40) the flag changes nothing a reader of the files or of the log can see — the same file names, the
same protobuf bytes, the same decompressed replay memory, the same "Snapshotting ..." lines — and a new process that restarts
through FindLatestSnapshot resumes from the newest complete set, a stray .tmp beside it notwithstanding.  The synchronous run is the
yardstick throughout."""
import glob
import gzip
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_dropin", "snapshot_async_smoke")
ARGS = ["-memory", "5000", "-memory_threshold", "50", "-loss_display_iter", "7", "-minibatch", "32", "-snapshot_freq", "20", "-seed", "7"]

pytestmark = pytest.mark.gpu


def _build(pkg):
    lib = pkg.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "shim"),
           "-o", EXE, os.path.join(ROOT, "tests", "cpp", "snapshot_async_smoke.cpp"), os.path.join(ROOT, "dqn-hfo_amd", "csrc", "dqn_dropin.cpp"),
           lib, "-Wl,-rpath," + os.path.dirname(lib)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def _run(exe, prefix, extra):
    r = subprocess.run([exe] + ARGS + ["-prefix", prefix] + extra, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "snapshot async smoke OK" in r.stdout, (extra, r.returncode, r.stdout, r.stderr)
    digest = [l for l in r.stdout.splitlines() if l.startswith("digest:")]
    assert len(digest) == 1, r.stdout
    return digest[0], r.stderr


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _left(d):
    return sorted(os.path.basename(f) for f in glob.glob(str(d / "*")))


def _snapshot_lines(stderr, d):
    return [l[l.index("Snapshotting"):].replace(str(d), "<dir>") for l in stderr.splitlines() if "Snapshotting" in l]


def test_same_names_bytes_and_log_text(pkg, gpu, tmp_path):
    exe = _build(pkg)
    dirs = {m: tmp_path / m for m in ("syn", "asy")}           # (names of one length: the solverstates hold the save path)
    out = {}
    for m, d in dirs.items():
        d.mkdir()
        out[m] = _run(exe, str(d / "agent0"), ["-stop_at", "40", "-remove_old_snapshots=false"] + (["-snapshot_async"] if m == "asy" else []))
    assert out["asy"][0] == out["syn"][0] and "actor_iter 40 critic_iter 40 memory_size 120" in out["syn"][0]
    files = _left(dirs["syn"])
    assert _left(dirs["asy"]) == files
    assert files == sorted("agent0_%s_iter_%d.%s" % (net, it, ext) for net in ("actor", "critic") for it in (20, 40) for ext in ("caffemodel", "solverstate")) + \
        ["agent0_iter_20.replaymemory", "agent0_iter_40.replaymemory"]
    for f in files:
        a, b = _read(str(dirs["syn"] / f)), _read(str(dirs["asy"] / f))
        if f.endswith(".replaymemory"):
            assert gzip.decompress(a) == gzip.decompress(b), f
        else:
            assert a.replace(b"/syn/", b"/asy/") == b, f
    want, got = _snapshot_lines(out["syn"][1], dirs["syn"]), _snapshot_lines(out["asy"][1], dirs["asy"])
    assert got == want and len(want) == 4, (want, got)          # "Snapshotting memory to ..." and "Snapshotting Finished!", twice
    assert "snapshot_async" not in out["asy"][1]                # (no fall-back line: the library took both snapshots)
    # with -remove_old_snapshots the older set goes only behind the newer one: the same files are left
    for m in dirs:
        d = tmp_path / (m + "_rm")
        d.mkdir()
        _run(exe, str(d / "agent0"), ["-stop_at", "40", "-remove_old_snapshots"] + (["-snapshot_async", "-snapshot_async_threads", "2"] if m == "asy" else []))
        assert _left(d) == [f for f in files if "_40." in f], (m, _left(d))


def test_restart_through_find_latest_snapshot(pkg, gpu, tmp_path):
    exe = _build(pkg)
    resumed = {}
    for m in ("syn", "asy"):
        d = tmp_path / m
        d.mkdir()
        flags = ["-snapshot_async"] if m == "asy" else []
        half, _ = _run(exe, str(d / "agent0"), flags + ["-stop_at", "20"])
        assert "actor_iter 20 critic_iter 20" in half
        assert not glob.glob(str(d / "*.tmp"))
        # what a process killed inside a later snapshot would leave: a partial file under a .tmp name
        for name in ("agent0_actor_iter_99.solverstate.tmp", "agent0_iter_99.replaymemory.tmp"):
            (d / name).write_bytes(b"partial")
        resumed[m], err = _run(exe, str(d / "agent0"), flags + ["-stop_at", "40", "-resume"])
        assert "actor_iter 40 critic_iter 40" in resumed[m]
        assert "Loading replay memory from " + str(d / "agent0_iter_20.replaymemory") in err
    assert resumed["asy"] == resumed["syn"]
