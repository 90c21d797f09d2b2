"""N-step returns against the 1-step learner, updates per second inside ONE process (alternating rounds of update_async_n bursts), at
the BASELINE shape: B = 256, 4 x 1024, S = 58, 1 M transitions filled.  Five learners take turns: the default plan, a plain learner
forced onto the schedule an n-step learner runs (TUNE_SEPARATE_Q_TRAIN | TUNE_SEPARATE_FIRST_LAYER | TUNE_LATE_GATHER), n-step
(n = 5), prioritized, and prioritized + n-step.  Writes the table to --out:
   python scripts/nstep_ab.py [--rounds 5] [--updates 1600] [--fill 1000000] [--n 5] [--out profiles/nstep_ab.md]
The gather kernels' own durations come from a kernel trace, one run per n (the kernel's name does not carry n):
   rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/nstep_ab.py --trace-n 5
runs 300 eager updates of a plain learner (k_gather) and of an n-step learner (k_gather_n) and nothing else.
n = 5 is the literature's customary value (D4PG, Rainbow), not measured on this workload."""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--updates", type=int, default=1600)
ap.add_argument("--fill", type=int, default=1000000)
ap.add_argument("--minibatch", type=int, default=256)
ap.add_argument("--n", type=int, default=5)
ap.add_argument("--trace-n", type=int, default=0, help="kernel-trace mode: eager updates of a plain and an n-step learner with this n")
ap.add_argument("--out", default=None)
args = ap.parse_args()
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from synth import synth_replay  # noqa: E402

pkg = load_package()
T = pkg.capi
S, H, B = 58, (1024, 1024, 1024, 1024), args.minibatch
chunk = synth_replay(np.random.default_rng(7), 100000, S)      # (episodes of ~100 steps, the last record terminal: chunks append whole episodes)


def make(n_step=None, prioritized=False, tuning=0, use_graph=True):
    d = pkg.DQN(S, minibatch=B, hidden=H, memory=args.fill + 1, seed=1, use_graph=use_graph, tuning=tuning)
    for _ in range(args.fill // 100000):
        d.add_transitions_arrays(*chunk)
    if prioritized:
        d.enable_prioritized_replay()
    if n_step:
        d.enable_n_step(n_step)
    return d


if args.trace_n:
    for d in (make(use_graph=False), make(n_step=args.trace_n, use_graph=False)):
        for _ in range(300):
            d.update_async(None)
        d.read_stats()
        print("n_step", d.n_step(), "steps of the last minibatch", np.bincount(d.n_step_debug_read("steps")) if d.n_step() else "-", flush=True)
        d.close()
    sys.exit(0)

lines = []


def emit(s=""):
    print(s, flush=True)
    lines.append(s)


FORCED = T.TUNE_SEPARATE_Q_TRAIN | T.TUNE_SEPARATE_FIRST_LAYER | T.TUNE_LATE_GATHER
learners = [("default", make()), ("forced", make(tuning=FORCED)), ("n_step", make(n_step=args.n)),
            ("per", make(prioritized=True)), ("per+n_step", make(n_step=args.n, prioritized=True))]
emit("# N-step returns against the 1-step learner (scripts/nstep_ab.py)")
emit()
emit("B = %d, hidden %s, S = %d, %d transitions filled, fp32, one process, %d alternating rounds of update_async_n(%d) bursts, n = %d." %
     (B, "x".join(map(str, H)), S, learners[0][1].memory_size(), args.rounds, args.updates, args.n))
emit("`forced`: a plain learner with TUNE_SEPARATE_Q_TRAIN | TUNE_SEPARATE_FIRST_LAYER | TUNE_LATE_GATHER.  n = %d is the literature's value, not measured on this workload." % args.n)
emit()
for name, d in learners:
    p = d.update_plan()
    emit("plan (%s): launches single %d, graph first %d, in graph %d; forms %s" % (name, p["launches_single"], p["launches_graph_first"], p["launches_in_graph"], " ".join(p["forms"])))
emit()
emit("memory: %s violations of the contiguity invariant (validate_memory)" % (learners[2][1].validate_memory(),))
for _, d in learners:
    d.update_async_n(64)
    d.read_stats()
emit()
emit("| round | " + " | ".join("%s updates/s" % n for n, _ in learners) + " |")
emit("|---|" + "---|" * len(learners))
rates = {n: [] for n, _ in learners}
for r in range(args.rounds):
    for name, d in learners:
        t0 = time.perf_counter()
        d.update_async_n(args.updates)
        d.read_stats()
        rates[name].append(args.updates / (time.perf_counter() - t0))
    emit("| %d | " % (r + 1) + " | ".join("%.0f" % rates[n][-1] for n, _ in learners) + " |")
med = {n: float(np.median(v)) for n, v in rates.items()}
emit()
emit("| learner | median updates/s | min | max | us per update |")
emit("|---|---|---|---|---|")
for n, _ in learners:
    emit("| %s | %.0f | %.0f | %.0f | %.1f |" % (n, med[n], min(rates[n]), max(rates[n]), 1e6 / med[n]))
emit()
us = lambda a, b: 1e6 / med[a] - 1e6 / med[b]
emit("n_step against forced: %+.1f us per update (ratio %.3f); against default: %+.1f us (ratio %.3f)" %
     (us("n_step", "forced"), med["n_step"] / med["forced"], us("n_step", "default"), med["n_step"] / med["default"]))
emit("per+n_step against per: %+.1f us per update (ratio %.3f)" % (us("per+n_step", "per"), med["per+n_step"] / med["per"]))
emit("steps of the n-step learner's last minibatch (count by m = 1 ..): %s" % np.bincount(learners[2][1].n_step_debug_read("steps"))[1:])
for _, d in learners:
    d.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
