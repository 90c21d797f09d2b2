"""What the replay sweep costs, at the BASELINE shape: B = 256, 4 x 1024, S = 58, 1 M transitions filled, fp32, one process, after
warm-up.  Writes the table to profiles/memory_sweep_ab.md (--out):
   python scripts/memory_sweep_ab.py [--reps 5] [--updates 4000] [--fill 1000000] [--out FILE]
Per repetition, alternating: the wall time of a full-memory dqnhip_evaluate_memory, of a full-memory dqnhip_per_refresh on a
prioritized learner of the same shape, and of `updates` update_async_n updates on the first learner — the time per chunk beside the
time per update."""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--updates", type=int, default=4000)
ap.add_argument("--fill", type=int, default=1000000)
ap.add_argument("--minibatch", type=int, default=256)
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
chunk = synth_replay(np.random.default_rng(7), 100000, S)
lines = []


def emit(s=""):
    print(s, flush=True)
    lines.append(s)


def make(per):
    d = pkg.DQN(S, minibatch=B, hidden=H, memory=args.fill + 1, seed=1, use_graph=True)
    for _ in range(args.fill // 100000):
        d.add_transitions_arrays(*chunk)
    if per:
        d.enable_prioritized_replay()
    return d


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def burst(d, n):
    d.update_async_n(n)
    d.read_stats()


plain, prio = make(False), make(True)
burst(plain, 64)
plain.evaluate_memory(0, 64 * B)
prio.per_refresh(0, 64 * B)
emit("# Replay sweep: full-memory wall times, B = %d, 4 x 1024, S = %d, %d transitions" % (B, S, plain.memory_size()))
emit()
emit("| rep | evaluate_memory s | us / chunk | per_refresh s | us / chunk | update_async_n us / update | chunk / update |")
emit("|---|---|---|---|---|---|---|")
for rep in range(args.reps):
    te, r = timed(lambda: plain.evaluate_memory_raw())
    tr, _ = timed(lambda: prio.per_refresh())
    tu, _ = timed(lambda: burst(plain, args.updates))
    ce, cr, cu = 1e6 * te / r.n_chunks, 1e6 * tr / r.n_chunks, 1e6 * tu / args.updates
    emit("| %d | %.3f | %.1f | %.3f | %.1f | %.1f | %.2f |" % (rep, te, ce, tr, cr, cu, ce / cu))
emit()
emit("%d chunks per sweep.  Wall times as the caller sees them (the call blocks until the report is there)." % r.n_chunks)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
