"""The asynchronous learner-state save (dqnhip_save_state_async) against the synchronous one, in ONE process on ONE learner at the shape of
profiles/state_file.md: B = 256, 4 x 1024, S = 58, 1 M transitions filled, prioritized replay on.  Alternating repetitions of
   * the wall time of dqnhip_save_state;
   * the time until dqnhip_save_state_async returns, the stream time of its launches (an event pair on the learner's stream around the
     call: pack + CRC together), and the time from the call to completion (dqnhip_save_state_wait);
   * the update rate over a window of --window updates (dqnhip_update_async_n, read_stats at its end) that starts with an asynchronous
     save in flight, against the same window of the same learner with no save, alternating: the second column's spread is the
     learner's own run-to-run spread.
Yardsticks: the synchronous save and the never-saving window, same process.  The two files of a repetition are compared byte for byte
(the learner does not move between them).  --saves-only N: N asynchronous saves and nothing else (what a kernel trace is taken of).
Writes profiles/state_async_ab.md (--out):
   python scripts/state_async_ab.py [--reps 5] [--fill 1000000] [--window 8000] [--dir /tmp] [--out profiles/state_async_ab.md]"""
import argparse
import ctypes as C
import os
import shutil
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--fill", type=int, default=1000000)
ap.add_argument("--minibatch", type=int, default=256)
ap.add_argument("--window", type=int, default=8000)
ap.add_argument("--saves-only", type=int, default=0)
ap.add_argument("--dir", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from synth import synth_replay  # noqa: E402

pkg = load_package()
hip = C.CDLL("libamdhip64.so")
S, H, B = 58, (1024, 1024, 1024, 1024), args.minibatch
work = tempfile.mkdtemp(prefix="state_async_ab_", dir=args.dir)
d = pkg.DQN(S, minibatch=B, hidden=H, memory=args.fill + 1, seed=1, use_graph=True, save_path=os.path.join(work, "agent0"))
chunk = synth_replay(np.random.default_rng(7), 100000, S)
for _ in range(args.fill // 100000):
    d.add_transitions_arrays(*chunk)
d.enable_prioritized_replay()
d.update_async_n(32)
d.read_stats()
stream = C.c_void_p(d.stream())
p_sync, p_async = os.path.join(work, "sync.learnerstate"), os.path.join(work, "async.learnerstate")

if args.saves_only:
    for _ in range(args.saves_only):
        d.save_state(p_async, wait=False)
        d.save_state_wait()
    d.close()
    shutil.rmtree(work, ignore_errors=True)
    sys.exit(0)


def hipck(rc):
    assert rc == 0, rc


ev = [C.c_void_p() for _ in range(2)]
for e in ev:
    hipck(hip.hipEventCreate(C.byref(e)))


def same_bytes(a, b):
    with open(a, "rb") as fa, open(b, "rb") as fb:
        while True:
            x, y = fa.read(1 << 24), fb.read(1 << 24)
            if x != y:
                return False
            if not x:
                return True


def window(save):
    """updates / s over args.window updates; save: an asynchronous save is in flight when the window starts"""
    d.read_stats()
    t0 = time.perf_counter()
    if save:
        d.save_state(p_async, wait=False)
    d.update_async_n(args.window)
    d.read_stats()                       # waits for the last update
    dt = time.perf_counter() - t0
    in_flight = not d.save_state_done()
    d.save_state_wait()
    return args.window / dt, in_flight


d.save_state(p_async, wait=False)        # first use: the staging buffer, the pinned ring and the writer thread are allocated here
d.save_state_wait()
window(False)
rows = []
for rep in range(args.reps):
    t0 = time.perf_counter()
    d.save_state(p_sync)
    t_sync = time.perf_counter() - t0
    hipck(hip.hipEventRecord(ev[0], stream))
    t0 = time.perf_counter()
    d.save_state(p_async, wait=False)
    t_call = time.perf_counter() - t0
    hipck(hip.hipEventRecord(ev[1], stream))
    d.save_state_wait()
    t_done = time.perf_counter() - t0
    ms = C.c_float()
    hipck(hip.hipEventSynchronize(ev[1]))
    hipck(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]))
    same = same_bytes(p_sync, p_async)
    r_save, in_flight = window(True)
    r_none, _ = window(False)
    rows.append((t_sync, t_call * 1e3, ms.value, t_done, r_save, r_none, same, in_flight))
    print("rep %d: sync %.3f s | async call %.3f ms, stream %.3f ms, done after %.3f s | %.0f updates/s with a save in flight, %.0f without | "
          "same bytes %s, still in flight at the window's end %s" % ((rep + 1,) + rows[-1]), flush=True)
size = os.path.getsize(p_async)
med = [float(np.median([r[k] for r in rows])) for k in range(6)]
none = [r[5] for r in rows]
lost_s = args.window / med[4] - args.window / med[5]
lines = ["# The asynchronous learner-state save against the synchronous one (scripts/state_async_ab.py)", "",
         "B = %d, hidden %s, S = %d, %d transitions filled, prioritized replay on, fp32, one process, one learner, %d alternating repetitions; "
         "the file is %d bytes.  Window: %d updates (dqnhip_update_async_n), the asynchronous save enqueued in front of it."
         % (B, "x".join(map(str, H)), S, args.fill, args.reps, size, args.window), "",
         "| rep | dqnhip_save_state (s) | dqnhip_save_state_async returns after (ms) | stream time of its launches (ms) | call to completion (s) | "
         "updates/s, save in flight | updates/s, no save | files identical |", "|---|---|---|---|---|---|---|---|"]
lines += ["| %d | %.3f | %.3f | %.3f | %.3f | %.0f | %.0f | %s |" % ((i + 1,) + r[:7]) for i, r in enumerate(rows)]
lines += ["| median | %.3f | %.3f | %.3f | %.3f | %.0f | %.0f | |" % tuple(med), "",
          "The never-saving window's own spread over the repetitions: %.0f ... %.0f updates/s (%.2f %% of its median)."
          % (min(none), max(none), 100.0 * (max(none) - min(none)) / med[5]),
          "Wall time a window loses to one save in flight, from the medians: %.3f s (window / rate with - window / rate without); the synchronous save stops the "
          "learner for %.3f s." % (lost_s, med[0]), ""]
text = "\n".join(lines) + "\n"
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text)
d.close()
shutil.rmtree(work, ignore_errors=True)
