"""The asynchronous Caffe snapshot (dqnhip_snapshot_async) against the synchronous one, in ONE process on ONE learner at the headline
shape: B = 256, 4 x 1024, S = 58, 1 M transitions filled.  Alternating repetitions of
   * the wall time of dqnhip_snapshot with the memory;
   * the time until dqnhip_snapshot_async returns, the stream time of its launches (an event pair on the learner's stream around the
     call: parameter pack, guard fill, k_snap_pack_replay and k_state_crc together; once more without the memory, so the difference is
     the replay memory's share), and the time from the call to completion (dqnhip_snapshot_wait) at 8 compressor threads;
   * the update rate over a window of --window updates (dqnhip_update_async_n, read_stats at its end) that starts with an asynchronous
     snapshot in flight, against the same window of the same learner with none: the second column's spread is the learner's own
     run-to-run spread;
then the call-to-completion time and the window with a snapshot in flight for 1 / 2 / 4 / 8 compressor threads, and the stream time
of the launches of dqnhip_save_state_async on the same ring in the same process as the yardstick of the pack.
The decompressed .replaymemory of each repetition's pair is compared byte for byte, the protobuf files as they are.
After the learner is closed, in processes of their own, one after the other:
   * --pack-forms EXE (scripts/snap_pack_forms.hip, built as its header says): both forms of the pack kernel and k_state_pack_ring, each
     launch between its own pair of events, on a ring of --fill records;
   * --adaptor EXE (scripts/snapshot_async_adaptor.cpp): the adaptor's loop of --adaptor-updates Update() calls on a full memory of
     --fill transitions at the driver's default -snapshot_freq 10000, three runs — no snapshot inside the run, the synchronous
     snapshot, -snapshot_async.
--bench-parent / --bench-tree: the updates/s of `python bench.py` runs of the parent commit and of this tree, alternating on one box
(comma-separated; they are made outside this script, which only prints the two lists side by side).  With --only-bench nothing is
measured: that section of an existing --out file is replaced.
Writes every section of profiles/snapshot_async_ab.md (--out); nothing in that file is written by hand:
   python scripts/snapshot_async_ab.py [--reps 5] [--fill 1000000] [--window 8000] [--dir /tmp] [--pack-forms EXE] [--adaptor EXE]
          [--bench-parent a,b,c --bench-tree a,b,c] [--out profiles/snapshot_async_ab.md]"""
import argparse
import ctypes as C
import gzip
import os
import shutil
import subprocess
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--fill", type=int, default=1000000)
ap.add_argument("--minibatch", type=int, default=256)
ap.add_argument("--window", type=int, default=8000)
ap.add_argument("--dir", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--pack-forms", default=None)
ap.add_argument("--adaptor", default=None)
ap.add_argument("--adaptor-updates", type=int, default=30000)
ap.add_argument("--bench-parent", default=None)
ap.add_argument("--bench-tree", default=None)
ap.add_argument("--only-bench", action="store_true")
args = ap.parse_args()
BENCH_TITLE = "## bench.py, the parent commit and this tree alternating on one box (updates/s)"


def bench_section():
    bp, bt = [float(x) for x in args.bench_parent.split(",")], [float(x) for x in args.bench_tree.split(",")]
    return [BENCH_TITLE, "", "| parent | this tree |", "|---|---|"] + ["| %.2f | %.2f |" % (a, b) for a, b in zip(bp, bt)] + \
        ["", "Parent: %.0f ... %.0f, median %.0f; this tree: %.0f ... %.0f, median %.0f (%+.2f %% between the medians; the parent's own spread is %.2f %%)."
         % (min(bp), max(bp), sorted(bp)[len(bp) // 2], min(bt), max(bt), sorted(bt)[len(bt) // 2],
            100.0 * (sorted(bt)[len(bt) // 2] / sorted(bp)[len(bp) // 2] - 1.0), 100.0 * (max(bp) - min(bp)) / sorted(bp)[len(bp) // 2]), ""]


if args.only_bench:
    with open(args.out) as f:
        text = f.read().split(BENCH_TITLE)[0].rstrip("\n") + "\n\n"
    with open(args.out, "w") as f:
        f.write(text + "\n".join(bench_section()) + "\n")
    sys.exit(0)
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from synth import synth_replay  # noqa: E402

pkg = load_package()
hip = C.CDLL("libamdhip64.so")
S, H, B = 58, (1024, 1024, 1024, 1024), args.minibatch
work = tempfile.mkdtemp(prefix="snapshot_async_ab_", dir=args.dir)
d = pkg.DQN(S, minibatch=B, hidden=H, memory=args.fill + 1, seed=1, use_graph=True, save_path=os.path.join(work, "agent0"))
chunk = synth_replay(np.random.default_rng(7), min(100000, args.fill), S)
for _ in range(max(args.fill // 100000, 1)):
    d.add_transitions_arrays(*chunk)
d.update_async_n(32)
d.read_stats()
stream = C.c_void_p(d.stream())
p_sync, p_async = os.path.join(work, "sync"), os.path.join(work, "async")


def hipck(rc):
    assert rc == 0, rc


ev = [C.c_void_p() for _ in range(2)]
for e in ev:
    hipck(hip.hipEventCreate(C.byref(e)))


def read(path):
    with open(path, "rb") as f:
        return f.read()


def same_files(it):
    for suf in ("_actor_iter_%d.caffemodel", "_actor_iter_%d.solverstate", "_critic_iter_%d.caffemodel", "_critic_iter_%d.solverstate"):
        if read(p_sync + suf % it) != read(p_async + suf % it):
            return False
    return gzip.decompress(read(p_sync + "_iter_%d.replaymemory" % it)) == gzip.decompress(read(p_async + "_iter_%d.replaymemory" % it))


def timed_async(memory, threads):
    """-> (ms until the call returns, stream ms of its launches, s from the call to completion)"""
    hipck(hip.hipEventRecord(ev[0], stream))
    t0 = time.perf_counter()
    d.Snapshot(snapshot_prefix=p_async, remove_old=False, snapshot_memory=memory, wait=False, compress_threads=threads)
    t_call = time.perf_counter() - t0
    hipck(hip.hipEventRecord(ev[1], stream))
    d.snapshot_wait()
    t_done = time.perf_counter() - t0
    ms = C.c_float()
    hipck(hip.hipEventSynchronize(ev[1]))
    hipck(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]))
    return t_call * 1e3, ms.value, t_done


def window(threads):
    """updates / s over args.window updates; threads > 0: an asynchronous snapshot with that many compressor threads is in flight when
    the window starts"""
    d.read_stats()
    t0 = time.perf_counter()
    if threads:
        d.Snapshot(snapshot_prefix=p_async, remove_old=False, wait=False, compress_threads=threads)
    d.update_async_n(args.window)
    d.read_stats()                       # waits for the last update
    dt = time.perf_counter() - t0
    in_flight = not d.snapshot_done()
    d.snapshot_wait()
    return args.window / dt, in_flight


timed_async(True, 8)                     # first use: the staging buffer, the pinned ring and the writer thread are allocated here
window(0)
rows = []
for rep in range(args.reps):
    it = d.actor_iter()
    t0 = time.perf_counter()
    d.Snapshot(snapshot_prefix=p_sync, remove_old=False)
    t_sync = time.perf_counter() - t0
    t_call, ms, t_done = timed_async(True, 8)
    _, ms_nomem, _ = timed_async(False, 8)
    same = same_files(it)
    sizes = (os.path.getsize(p_sync + "_iter_%d.replaymemory" % it), os.path.getsize(p_async + "_iter_%d.replaymemory" % it))
    r_snap, in_flight = window(8)
    r_none, _ = window(0)
    rows.append((t_sync, t_call, ms, ms_nomem, t_done, r_snap, r_none, same, in_flight))
    print("rep %d: sync %.3f s | async call %.3f ms, stream %.3f ms (%.3f ms without the memory), done after %.3f s | %.0f updates/s with a snapshot "
          "in flight, %.0f without | same bytes %s, still in flight at the window's end %s" % ((rep + 1,) + rows[-1]), flush=True)
    for f in os.listdir(work):           # (the files of this iteration: the next repetition's are named by a later one)
        os.remove(os.path.join(work, f))

scaling = []
for threads in (1, 2, 4, 8):
    _, _, t_done = timed_async(True, threads)
    r_snap, _ = window(threads)
    scaling.append((threads, t_done, r_snap))
    for f in os.listdir(work):
        os.remove(os.path.join(work, f))
    print("%d compressor threads: call to completion %.3f s, %.0f updates/s with the snapshot in flight" % scaling[-1], flush=True)

# the yardstick of the pack: the learner-state save's launches (k_state_pack_params, k_state_pack_ring, k_state_crc) on the same ring
p_state = os.path.join(work, "yardstick.learnerstate")
d.save_state(p_state, wait=False)
d.save_state_wait()
hipck(hip.hipEventRecord(ev[0], stream))
d.save_state(p_state, wait=False)
hipck(hip.hipEventRecord(ev[1], stream))
d.save_state_wait()
ms_state = C.c_float()
hipck(hip.hipEventSynchronize(ev[1]))
hipck(hip.hipEventElapsedTime(C.byref(ms_state), ev[0], ev[1]))

med = [float(np.median([r[k] for r in rows])) for k in range(7)]
none = [r[6] for r in rows]
lost_ms = 1e3 * (args.window / med[5] - args.window / med[6])
stream_bytes = 4 + args.fill * (4 * S + 49)
lines = ["# The asynchronous Caffe snapshot against the synchronous one (scripts/snapshot_async_ab.py)", "",
         "B = %d, hidden %s, S = %d, %d transitions filled, fp32, one process, one learner, %d alternating repetitions; the uncompressed "
         "`.replaymemory` stream is %d bytes, the synchronous file %d bytes, the asynchronous one (1 MiB chunks) %d bytes.  Window: %d updates "
         "(dqnhip_update_async_n), the asynchronous snapshot (8 compressor threads) enqueued in front of it."
         % (B, "x".join(map(str, H)), S, args.fill, args.reps, stream_bytes, sizes[0], sizes[1], args.window), "",
         "| rep | dqnhip_snapshot (s) | dqnhip_snapshot_async returns after (ms) | stream time of its launches (ms) | ... without the memory (ms) | "
         "call to completion (s) | updates/s, snapshot in flight | updates/s, none | files identical |", "|---|---|---|---|---|---|---|---|---|"]
lines += ["| %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.0f | %.0f | %s |" % ((i + 1,) + r[:8]) for i, r in enumerate(rows)]
lines += ["| median | %.3f | %.3f | %.3f | %.3f | %.3f | %.0f | %.0f | |" % tuple(med), "",
          "The replay memory's share of the stream time (k_snap_pack_replay + the guard fill + k_state_crc over "
          "the stream), from the medians: %.3f ms for %.2f GB read and %.2f GB written.  Yardstick, same process, same ring: the launches of "
          "dqnhip_save_state_async (k_state_pack_params, k_state_pack_ring, k_state_crc over every section) take %.3f ms of stream time."
          % (med[2] - med[3], args.fill * (64 * 4 + 16 * 4 + 9) / 1e9, stream_bytes / 1e9, ms_state.value), "",
          "| compressor threads | call to completion (s) | updates/s with the snapshot in flight |", "|---|---|---|"]
lines += ["| %d | %.3f | %.0f |" % s for s in scaling]
lines += ["",
          "The never-snapshotting window's own spread over the repetitions: %.0f ... %.0f updates/s (%.2f %% of its median)."
          % (min(none), max(none), 100.0 * (max(none) - min(none)) / med[6]),
          "Wall time a window loses to one snapshot in flight (8 threads), from the medians: %.1f ms (window / rate with - window / rate without); "
          "the synchronous snapshot stops the learner for %.3f s." % (lost_ms, med[0]), ""]
d.close()

lines += ["## The parent's figures beside them", "", "| | parent commit | this tree |", "|---|---|---|",
          "| `dqnhip_snapshot` with the memory (s) | 7.97 (`profiles/state_file.md`) | %.2f (median above; the synchronous path is unchanged) |" % med[0],
          "| time the caller's thread is held per snapshot | 7.97 s | %.2f ms (`dqnhip_snapshot_async`) |" % med[1],
          "| `.replaymemory` size (bytes) | %d (one `gzwrite` stream) | %d (1 MiB chunks, %+.3f %%) |" % (sizes[0], sizes[1], 100.0 * (sizes[1] - sizes[0]) / sizes[0]),
          ""]

if args.pack_forms:
    r = subprocess.run([args.pack_forms, str(args.fill), str(S)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines += ["## The two forms of `k_snap_pack_replay`, each launch on its own (scripts/snap_pack_forms.hip)", "", r.stdout.strip(), "",
              "The library launches the workgroup form with 64 records per workgroup; the form with one thread per output dword is kept in "
              "scripts/snap_pack_forms.hip alone.  `k_state_pack_ring` copies whole rows with 16-byte loads and stores; the snapshot's pack "
              "funnels every output dword from two source words, because a record is 1 (mod 4) bytes long.", ""]

if args.adaptor:
    runs = {}
    for name, flags in (("no snapshot inside the run", ["-snapshot_freq", str(10 * args.adaptor_updates)]), ("synchronous snapshot", ["-snapshot_freq", "10000"]),
                        ("`-snapshot_async`", ["-snapshot_freq", "10000", "-snapshot_async"])):
        sub = tempfile.mkdtemp(prefix="adaptor_", dir=work)
        r = subprocess.run([args.adaptor, "-prefix", os.path.join(sub, "agent0"), "-memory", str(args.fill), "-minibatch", str(B), "-fill", str(args.fill),
                            "-updates", str(args.adaptor_updates), "-seed", "7"] + flags, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (name, r.stdout[-2000:], r.stderr[-2000:])
        line = [l for l in r.stdout.splitlines() if l.startswith("adaptor:")][0].split()
        runs[name] = (float(line[4]), float(line[6]), len([f for f in os.listdir(sub) if f.endswith(".replaymemory")]))
        print(name, runs[name], flush=True)
        shutil.rmtree(sub, ignore_errors=True)
    base = runs["no snapshot inside the run"][0]
    lines += ["## The adaptor's update loop: %d calls of Update() on a full memory, `-snapshot_freq 10000` (scripts/snapshot_async_adaptor.cpp)" % args.adaptor_updates, "",
              "`dqn::DQN` at B = %d, 4 x 1024, %d transitions, every other flag at the driver's default (`-snapshot_memory`, `-remove_old_snapshots`); "
              "one process per row, one run each.  Wall time: from the first Update() until the learner is destroyed, so a snapshot in flight at the end "
              "is waited for.  Share in snapshots: (wall - wall of the run without a snapshot) / wall." % (B, args.fill), "",
              "| run | wall (s) | of it the Update() loop (s) | share of wall time in snapshots | `.replaymemory` files left |", "|---|---|---|---|---|"]
    lines += ["| %s | %.2f | %.2f | %.1f %% | %d |" % (k, v[0], v[1], 100.0 * (v[0] - base) / v[0], v[2]) for k, v in runs.items()]
    lines += [""]

if args.bench_parent and args.bench_tree:
    lines += bench_section()

text = "\n".join(lines) + "\n"
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
shutil.rmtree(work, ignore_errors=True)
