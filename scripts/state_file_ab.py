"""Wall time of the native learner-state file against the Caffe snapshot path, in ONE process on ONE learner at the BASELINE shape:
B = 256, 4 x 1024, S = 58, 1 M transitions filled, prioritized replay on.  Alternating repetitions of
   dqnhip_save_state / dqnhip_load_state      against      dqnhip_snapshot(..., snapshot_memory = 1) / the three restore calls
(RestoreActorSolver, RestoreCriticSolver, LoadReplayMemory), and the file sizes.  A second table estimates where the native save's time
goes: zlib.crc32 over the file's bytes and a plain write + fsync of as many bytes, timed in this process; the rest is device-to-host
copies and the dense <-> arena conversion.  Writes profiles/state_file.md (--out):
   python scripts/state_file_ab.py [--reps 5] [--fill 1000000] [--dir /tmp] [--out profiles/state_file.md]"""
import argparse
import glob
import os
import shutil
import sys
import tempfile
import time
import zlib

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--fill", type=int, default=1000000)
ap.add_argument("--minibatch", type=int, default=256)
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
S, H, B = 58, (1024, 1024, 1024, 1024), args.minibatch
work = tempfile.mkdtemp(prefix="state_file_ab_", dir=args.dir)
d = pkg.DQN(S, minibatch=B, hidden=H, memory=args.fill + 1, seed=1, use_graph=True, save_path=os.path.join(work, "agent0"))
chunk = synth_replay(np.random.default_rng(7), 100000, S)
for _ in range(args.fill // 100000):
    d.add_transitions_arrays(*chunk)
d.enable_prioritized_replay()
d.update_async_n(32)
d.read_stats()


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


native, prefix = os.path.join(work, "agent0.learnerstate"), os.path.join(work, "agent0")
rows = []
for rep in range(args.reps):
    t_save = timed(lambda: d.save_state(native))
    t_load = timed(lambda: d.load_state(native))
    t_snap = timed(lambda: d.Snapshot(prefix, True, True))
    actor, critic, memory = pkg.FindLatestSnapshot(prefix)
    t_rest = timed(lambda: (d.RestoreActorSolver(actor), d.RestoreCriticSolver(critic), d.LoadReplayMemory(memory)))
    rows.append((t_save, t_load, t_snap, t_rest))
    print("rep %d: save_state %.2f s, load_state %.2f s | snapshot %.2f s, restore x3 %.2f s" % ((rep + 1,) + rows[-1]), flush=True)
native_bytes = os.path.getsize(native)
caffe = {os.path.basename(f): os.path.getsize(f) for f in sorted(glob.glob(prefix + "_*"))}
with open(native, "rb") as f:
    data = f.read()
t_crc = timed(lambda: zlib.crc32(data))
scratch = os.path.join(work, "scratch.bin")


def plain_write():
    with open(scratch, "wb") as f:
        f.write(data)
        f.flush()
        os.fsync(f.fileno())


t_write = timed(plain_write)
t_read = timed(lambda: open(scratch, "rb").read())
med = [float(np.median([r[k] for r in rows])) for k in range(4)]
lines = ["# The learner-state file against the Caffe snapshot path (scripts/state_file_ab.py)", "",
         "B = %d, hidden %s, S = %d, %d transitions filled, prioritized replay on, fp32, one process, one learner, %d alternating repetitions; wall time in seconds."
         % (B, "x".join(map(str, H)), S, args.fill, args.reps), "",
         "| rep | dqnhip_save_state | dqnhip_load_state | dqnhip_snapshot (memory = 1) | RestoreActorSolver + RestoreCriticSolver + LoadReplayMemory |", "|---|---|---|---|---|"]
lines += ["| %d | %.2f | %.2f | %.2f | %.2f |" % ((i + 1,) + r) for i, r in enumerate(rows)]
lines += ["| median | %.2f | %.2f | %.2f | %.2f |" % tuple(med), "",
          "save: native / snapshot = %.2f; load: native / restore = %.2f" % (med[0] / med[2], med[1] / med[3]), "",
          "| file | bytes |", "|---|---|", "| agent0.learnerstate | %d |" % native_bytes]
lines += ["| %s | %d |" % kv for kv in caffe.items()]
lines += ["| the Caffe files together | %d |" % sum(caffe.values()), "",
          "Where a native save's %.2f s go (estimates from this process, same bytes): zlib.crc32 over the file %.2f s, a plain write + fsync of the file %.2f s, "
          "the rest (device-to-host copies through pageable memory, arena -> dense) about %.2f s.  A native load's %.2f s: reading the file back %.2f s, its CRC %.2f s, the rest host-to-device."
          % (med[0], t_crc, t_write, max(0.0, med[0] - t_crc - t_write), med[1], t_read, t_crc), "",
          "The Caffe files lose on resume what the learner-state file keeps (targets, counters, ring position, priorities): the two columns are not the same service."]
text = "\n".join(lines) + "\n"
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text)
d.close()
shutil.rmtree(work, ignore_errors=True)
