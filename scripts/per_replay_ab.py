"""Prioritized replay against the plain learner, updates per second inside ONE process (alternating pairs of update_async_n bursts),
at the BASELINE shape: B = 256, 4 x 1024, S = 58, 1 M transitions filled.  Then the three replay-side kernels' own durations from the
library's timing mode (eager launches).  Writes the table to profiles/per_replay_ab.md (--out):
   python scripts/per_replay_ab.py [--pairs 5] [--updates 1600] [--fill 1000000] [--out profiles/per_replay_ab.md]
The defaults of dqnhip_per_default_config are used: the paper's customary values, not measured on this workload."""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--updates", type=int, default=1600)
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


def make(prioritized, use_graph=True):
    d = pkg.DQN(S, minibatch=B, hidden=H, memory=args.fill + 1, seed=1, use_graph=use_graph)
    for _ in range(args.fill // 100000):
        d.add_transitions_arrays(*chunk)
    if prioritized:
        d.enable_prioritized_replay()
    return d


lines = []


def emit(s=""):
    print(s, flush=True)
    lines.append(s)


plain, prio = make(False), make(True)
emit("# Prioritized replay against the plain learner (scripts/per_replay_ab.py)")
emit()
emit("B = %d, hidden %s, S = %d, %d transitions filled, fp32, one process, %d alternating pairs of update_async_n(%d) bursts." %
     (B, "x".join(map(str, H)), S, plain.memory_size(), args.pairs, args.updates))
emit("Priority parameters: dqnhip_per_default_config (alpha 0.6, beta 0.4 constant, eps 1e-6) - the paper's customary values, not measured on this workload.")
emit()
emit("plan (plain):       %s" % plain.update_plan())
emit("plan (prioritized): %s" % prio.update_plan())
emit()
for d in (plain, prio):
    d.update_async_n(64)
    d.read_stats()
emit("| pair | plain updates/s | prioritized updates/s | prioritized / plain |")
emit("|---|---|---|---|")
ratios = []
for p in range(args.pairs):
    rate = {}
    for name, d in (("plain", plain), ("prio", prio)):
        t0 = time.perf_counter()
        d.update_async_n(args.updates)
        d.read_stats()
        rate[name] = args.updates / (time.perf_counter() - t0)
    ratios.append(rate["prio"] / rate["plain"])
    emit("| %d | %.0f | %.0f | %.3f |" % (p + 1, rate["plain"], rate["prio"], ratios[-1]))
emit()
emit("prioritized / plain: median %.3f (min %.3f, max %.3f); us per update added: %.1f" %
     (float(np.median(ratios)), min(ratios), max(ratios), 0.0 if not ratios else 1e6 * (1 / rate["prio"] - 1 / rate["plain"])))
st = prio.per_state()
emit("tree after the bursts: levels %d, total %.6g, p_max %.6g, syncs %d" % (st["levels"], st["total"], st["p_max"], st["syncs"]))
plain.close(); prio.close()

# the kernels' own durations: timing mode, eager launches (timed launches are never captured)
timed = make(True, use_graph=False)
timed.UpdateActorCritic()
timed.set_kernel_timing(True)
for _ in range(50):
    timed.update_async(None)
timed.add_transitions_arrays(*[x[:4096] for x in chunk])       # one sync over 4096 appended (and as many evicted) slots
timed.update_async(None)
timed.read_stats()
emit()
emit("| kernel (timing family) | launches | avg us |")
emit("|---|---|---|")
for fam in ("per_sample", "per_update", "per_sync"):
    ms, n = timed.kernel_timing(fam)
    emit("| %s | %d | %.2f |" % (fam, n, ms * 1e3))
timed.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
