"""Caffe's other solvers against Adam inside ONE process at the BASELINE shape (B = 256, 4 x 1024, S = 58, fp32):
  1. the optimiser launches' own duration from the library's timing mode (family "adam": k_adam_soft for the Adam learner,
     k_solver_soft<> for the others; eager launches, two per update), alternating rounds over the six learners;
  2. updates per second of update_async_n bursts, alternating rounds.
The Adam learner runs with DQNHIP_TUNE_SEPARATE_FIRST_LAYER | DQNHIP_TUNE_LATE_GATHER: the schedule the other solvers' learners take
(no first-layer riders in the optimiser launches), so its optimiser launches are plain k_adam_soft / k_adam_soft_gather on the same
arenas — the fair yardstick.  A second Adam learner with the default plan is listed beside it.
Writes the tables to --out:
   python scripts/solvers_ab.py [--rounds 5] [--updates 800] [--timed 40] [--fill 100000] [--out profiles/solvers_ab.md]"""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--updates", type=int, default=800)
ap.add_argument("--timed", type=int, default=40)
ap.add_argument("--fill", type=int, default=100000)
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
chunk = synth_replay(np.random.default_rng(7), args.fill, S)
SAME_SCHEDULE = pkg.capi.TUNE_SEPARATE_FIRST_LAYER | pkg.capi.TUNE_LATE_GATHER
# name -> DQN keyword arguments (learning rates small enough that 10^4 steps on synthetic data stay finite under every rule)
LEARNERS = [
    ("Adam (same schedule)", dict(solver="Adam", tuning=SAME_SCHEDULE)),
    ("Adam (default plan)", dict(solver="Adam")),
    ("SGD", dict(solver="SGD", momentum=0.95)),
    ("Nesterov", dict(solver="Nesterov", momentum=0.95)),
    ("AdaGrad", dict(solver="AdaGrad", momentum=0.0)),
    ("RMSProp", dict(solver="RMSProp", momentum=0.0, actor_lr=1e-6, critic_lr=1e-5)),
    ("AdaDelta", dict(solver="AdaDelta", momentum=0.95, delta=1e-6, actor_lr=1e-3, critic_lr=1e-2)),
]


def make(kw, use_graph):
    d = pkg.DQN(S, minibatch=B, hidden=H, memory=args.fill + 1, seed=1, use_graph=use_graph, **kw)
    d.add_transitions_arrays(*chunk)
    return d


lines = []


def emit(s=""):
    print(s, flush=True)
    lines.append(s)


def spread(v):
    return "%.2f (min %.2f, max %.2f)" % (float(np.median(v)), min(v), max(v))


emit("# Caffe's other solvers against Adam (scripts/solvers_ab.py)")
emit()
emit("B = %d, hidden %s, S = %d, %d transitions, fp32, one process, %d alternating rounds." % (B, "x".join(map(str, H)), S, args.fill, args.rounds))
emit()

# ---- 1. the optimiser launches' own duration -----------------------------------------------------------------------------------------
timed = [(name, make(kw, False)) for name, kw in LEARNERS]
for name, d in timed:
    emit("plan (%s): %s" % (name, d.update_plan()))
    d.UpdateActorCritic()
    d.set_kernel_timing(True)
emit()
us = {name: [] for name, _ in timed}
for r in range(args.rounds):
    for name, d in timed:
        d.kernel_timing("adam", reset=True)
        for _ in range(args.timed):
            d.update_async(None)
        d.read_stats()
        ms, n = d.kernel_timing("adam", reset=True)
        assert n == 2 * args.timed, (name, n)
        us[name].append(ms * 1e3)
base = float(np.median(us["Adam (same schedule)"]))
emit("Optimiser launch, average over the actor's and the critic's (%d launches per round; the default-plan Adam learner's critic launch also" % (2 * args.timed))
emit("carries critic(s, mu(s))'s first layer):")
emit()
emit("| learner | us per launch: median (min, max) over rounds | / Adam (same schedule) | B/param | expected from bytes |")
emit("|---|---|---|---|---|")
for name, d in timed:
    nb = 36 if name.startswith("Adam") or name == "AdaDelta" else 28
    emit("| %s | %s | %.3f | %d | %.3f |" % (name, spread(us[name]), float(np.median(us[name])) / base, nb, nb / 36.0))
    d.close()
emit()

# ---- 2. update rate ------------------------------------------------------------------------------------------------------------------
burst = [(name, make(kw, True)) for name, kw in LEARNERS]
for name, d in burst:
    d.update_async_n(64)
    d.read_stats()
rate = {name: [] for name, _ in burst}
for r in range(args.rounds):
    for name, d in burst:
        t0 = time.perf_counter()
        d.update_async_n(args.updates)
        d.read_stats()
        rate[name].append(args.updates / (time.perf_counter() - t0))
base = float(np.median(rate["Adam (same schedule)"]))
emit("update_async_n(%d) bursts:" % args.updates)
emit()
emit("| learner | updates/s: median (min, max) over rounds | spread (max - min) / median | / Adam (same schedule) |")
emit("|---|---|---|---|")
for name, d in burst:
    v = rate[name]
    emit("| %s | %s | %.2f %% | %.3f |" % (name, spread(v), 100 * (max(v) - min(v)) / float(np.median(v)), float(np.median(v)) / base))
    d.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
