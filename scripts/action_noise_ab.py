"""Action noise, measured inside ONE process.  (1) Exploration noise of the env front-end against the plain step, env steps per second: per worker count two
synthetic handles on two learners of the same shape — noise off, noise on (the defaults: theta 0.15, sigma 0.1 on the parameters) —
take turns in alternating rounds of dqnhip_env_step bursts, replayed as captured graphs (hidden 1024x512x256x128, S = 58, fp32
acting, max_steps 100, p_end 0.01).  (2) Target policy smoothing against the plain learner, updates per second at the BASELINE
shape (B = 256, 4 x 1024, S = 58, --fill transitions): the default plan, a plain learner forced onto the schedule a smoothing
learner runs (TUNE_SEPARATE_CRITIC_FIRST_LAYERS) and a smoothing learner take turns in alternating rounds of update_async_n bursts.
Writes the tables to --out:
   python scripts/action_noise_ab.py [--rounds 5] [--steps 1600] [--workers 64,2048] [--updates 1600] [--fill 1000000] [--out profiles/action_noise_ab.md]"""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=1600)
ap.add_argument("--workers", default="64,2048")
ap.add_argument("--updates", type=int, default=1600)
ap.add_argument("--fill", type=int, default=1000000)
ap.add_argument("--out", default=None)
args = ap.parse_args()
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
S, H, T = 58, (1024, 512, 256, 128), 100
lines = []


def emit(s=""):
    print(s, flush=True)
    lines.append(s)


def make(workers, noise):
    d = pkg.DQN(S, minibatch=32, hidden=H, memory=workers * T + 4096, seed=1, use_graph=True)
    e = pkg.EnvFrontEnd(d, workers, max_steps=T, p_end=0.01, seed=3)
    if noise:
        e.set_noise()
    return d, e


emit("# Exploration noise against the plain env step (scripts/action_noise_ab.py)")
emit()
emit("Hidden %s, S = %d, fp32 acting, max_steps %d, p_end 0.01, epsilon 0.1; one process, %d alternating rounds of dqnhip_env_step(%d) per handle," %
     ("x".join(map(str, H)), S, T, args.rounds, args.steps))
emit("replayed as captured 16-step graphs.  Noise on: the defaults (theta 0.15, sigma_params 0.1, sigma_logits 0, clamp), the literature's")
emit("values, not measured on this workload.")
for workers in [int(w) for w in args.workers.split(",")]:
    pairs = [("off", make(workers, False)), ("on", make(workers, True))]
    for _, (d, e) in pairs:
        e.step(0.1, 64)
        e.stats()
    emit()
    emit("## %d workers" % workers)
    emit()
    emit("launches in the captured (1-step, 16-step) graphs: off %s, on %s" % (pairs[0][1][1].debug_read("graph_nodes"), pairs[1][1][1].debug_read("graph_nodes")))
    emit()
    emit("| round | noise off steps/s | noise on steps/s |")
    emit("|---|---|---|")
    rates = {n: [] for n, _ in pairs}
    for r in range(args.rounds):
        for name, (d, e) in pairs:
            t0 = time.perf_counter()
            e.step(0.1, args.steps)
            e.stats()
            rates[name].append(args.steps / (time.perf_counter() - t0))
        emit("| %d | %.0f | %.0f |" % (r + 1, rates["off"][-1], rates["on"][-1]))
    med = {n: float(np.median(v)) for n, v in rates.items()}
    emit()
    emit("median: off %.0f steps/s (%.2f us per step, min %.0f max %.0f), on %.0f steps/s (%.2f us per step, min %.0f max %.0f): %+.2f us per step, ratio %.3f" %
         (med["off"], 1e6 / med["off"], min(rates["off"]), max(rates["off"]), med["on"], 1e6 / med["on"], min(rates["on"]), max(rates["on"]),
          1e6 / med["on"] - 1e6 / med["off"], med["on"] / med["off"]))
    for _, (d, e) in pairs:
        e.close(); d.close()
# ---- (2) target policy smoothing -------------------------------------------------------------------------------------------------
from synth import synth_replay  # noqa: E402

T = pkg.capi
UB, UH = 256, (1024, 1024, 1024, 1024)
chunk = synth_replay(np.random.default_rng(7), 100000, S)


def make_learner(smooth=False, tuning=0):
    d = pkg.DQN(S, minibatch=UB, hidden=UH, memory=args.fill + 1, seed=1, use_graph=True, tuning=tuning)
    for _ in range(args.fill // 100000):
        d.add_transitions_arrays(*chunk)
    if smooth:
        d.enable_target_smoothing()
    return d


learners = [("default", make_learner()), ("forced", make_learner(tuning=T.TUNE_SEPARATE_CRITIC_FIRST_LAYERS)), ("smoothing", make_learner(smooth=True))]
emit()
emit("# Target policy smoothing against the plain learner")
emit()
emit("B = %d, hidden %s, S = %d, %d transitions filled, fp32, one process, %d alternating rounds of update_async_n(%d) bursts." %
     (UB, "x".join(map(str, UH)), S, learners[0][1].memory_size(), args.rounds, args.updates))
emit("`forced`: a plain learner with TUNE_SEPARATE_CRITIC_FIRST_LAYERS.  Smoothing: the defaults (sigma 0.1, clip 0.25 of the range, clamp), TD3's")
emit("values on a range of 2, not measured on this workload.")
emit()
for name, d in learners:
    p = d.update_plan()
    emit("plan (%s): launches single %d, graph first %d, in graph %d; forms %s" % (name, p["launches_single"], p["launches_graph_first"], p["launches_in_graph"], " ".join(p["forms"])))
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
emit("smoothing against forced: %+.1f us per update (ratio %.3f); against default: %+.1f us (ratio %.3f)" %
     (1e6 / med["smoothing"] - 1e6 / med["forced"], med["smoothing"] / med["forced"], 1e6 / med["smoothing"] - 1e6 / med["default"], med["smoothing"] / med["default"]))
for _, d in learners:
    d.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
