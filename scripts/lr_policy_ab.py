#!/usr/bin/env python3
"""What an lr policy and a weight decay cost, in ONE process on one GPU (the manner of scripts/solvers_ab.py): five alternating rounds
over learners at B = 256, 4 x 1024, S = 58 —

    adam_fixed          the default learner (tuned Adam kernels, first-layer riders)
    adam_exp            the same with lr_policy exp: same kernels, same bytes — expected equal
    adam_l2             Adam with weight_decay on k_sched_soft<Adam>: 36 B/param, no pow chain (the slot), no riders
    adam_fixed_late     the default learner forced onto SEPARATE_FIRST_LAYER | LATE_GATHER: what the riders are worth
    rmsprop_fixed / rmsprop_exp_l2     k_solver_soft<RMSProp> against k_sched_soft<RMSProp>: 28 B/param both

per learner the optimiser launch time (kernel timing mode, family "adam": the mean over the timed launches of eager updates) and the
update_async_n burst rate.  Writes profiles/lr_policy_ab.md; prints one JSON line.  Usage: python scripts/lr_policy_ab.py [--rounds 5] [--out profiles/lr_policy_ab.md]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package  # noqa: E402
from synth import synth_replay  # noqa: E402

B, S, HIDDEN = 256, 58, (1024, 1024, 1024, 1024)
LATE = 32 | 128          # capi.TUNE_SEPARATE_FIRST_LAYER | TUNE_LATE_GATHER
VARIANTS = {
    "adam_fixed": dict(),
    "adam_exp": dict(lr_policy="exp", lr_gamma=0.999999),
    "adam_l2": dict(weight_decay=5e-4),
    "adam_fixed_late": dict(tuning=LATE),
    "rmsprop_fixed": dict(solver="RMSProp", momentum=0.0),
    "rmsprop_exp_l2": dict(solver="RMSProp", momentum=0.0, lr_policy="exp", lr_gamma=0.999999, weight_decay=5e-4),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bursts", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lr_policy_ab.md"))
    a = ap.parse_args()
    pkg = load_package()
    rng = np.random.default_rng(5)
    s, act, r, mc, nx, term = synth_replay(rng, 8192, S, mean_len=50)
    learners = {}
    for name, kw in VARIANTS.items():
        d = pkg.DQN(S, minibatch=B, hidden=HIDDEN, memory=16384, seed=3, use_graph=True, **kw)
        d.add_transitions_arrays(s, act, r, mc, nx, term)
        d.update_async_n(32); d.read_stats()
        learners[name] = d
    rate = {n: [] for n in VARIANTS}
    opt_us = {n: [] for n in VARIANTS}
    for _ in range(a.rounds):
        for name, d in learners.items():
            d.read_stats()
            t0 = time.perf_counter()
            for _ in range(a.bursts):
                d.update_async_n(16)
            d.read_stats()
            rate[name].append(16 * a.bursts / (time.perf_counter() - t0))
            d.set_kernel_timing(True)
            for _ in range(20):
                d.UpdateActorCritic(None)
            ms, n = d.kernel_timing("adam", reset=True)          # the average over the n = 40 timed launches
            d.set_kernel_timing(False)
            assert n == 40, (name, n)
            opt_us[name].append(1e3 * ms)
    plans = {n: d.update_plan() for n, d in learners.items()}
    for d in learners.values():
        d.close()
    med = lambda v: float(np.median(v))
    out = {n: {"updates_per_s": med(rate[n]), "updates_per_s_min_max": [min(rate[n]), max(rate[n])], "optimiser_launch_us": med(opt_us[n]),
               "launches_in_graph": plans[n]["launches_in_graph"], "forms": plans[n]["forms"]} for n in VARIANTS}
    base = out["adam_fixed"]
    lines = ["# lr policy / weight decay A/B", "",
             "B = %d, hidden %s, S = %d; %d alternating rounds in one process, medians (min .. max of the rate)." % (B, "x".join(map(str, HIDDEN)), S, a.rounds), "",
             "| learner | optimiser launch [us] | vs adam_fixed | update_async_n [updates/s] | vs adam_fixed | launches per update in a graph |", "|---|---|---|---|---|---|"]
    for n, o in out.items():
        lines.append("| %s | %.2f | %.3f | %.0f (%.0f .. %.0f) | %.3f | %d |" % (
            n, o["optimiser_launch_us"], o["optimiser_launch_us"] / base["optimiser_launch_us"], o["updates_per_s"], o["updates_per_s_min_max"][0],
            o["updates_per_s_min_max"][1], o["updates_per_s"] / base["updates_per_s"], o["launches_in_graph"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
