#!/usr/bin/env python3
"""Same-process A/B of the three forms a burst of updates can take on the BASELINE configs[1] learner (bench.py's headline shape):

  chained    BenchmarkBlocking(pipelined=2): dqnhip_update_chained, one graph launch and one blocking read-back per update - what
             the drop-in's Update() costs without -deferred_updates
  deferred   BenchmarkBlocking(pipelined=3): dqnhip_update_indexed_n every sixteen updates, dqnhip_collect_stats every 1000 - what
             -deferred_updates costs
  headline   Benchmark: dqnhip_update_async_n, indices sampled on the device - what bench.py times

Six alternating rounds, each leg behind the pre-warm bench.py uses (100 ms of sixteen-update replays), every value printed and
written to --out.  One learner, one process, one GPU.

usage: timeout -k 10 600 python scripts/deferred_timing.py [--out profiles/r07_deferred_update.txt] [--steps 2000]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_deferred_update.txt"))
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--replay", type=int, default=bench.REPLAY)
    args = ap.parse_args()
    pkg = load_package()
    bench.load_built_library(pkg)
    d = pkg.DQN(bench.S, minibatch=bench.B, hidden=bench.HIDDEN, memory=args.replay, seed=1, use_graph=True)
    bench.prefill(d, args.replay - 1, seed=100)

    def prewarm(ms=100.0):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < ms * 1e-3:
            d.update_async_n(16)
        d.read_stats()

    legs = (("chained", lambda: d.BenchmarkBlocking(args.steps, 100, seed=1, pipelined=2)),
            ("deferred", lambda: d.BenchmarkBlocking(args.steps, 100, seed=1, pipelined=3)),
            ("headline", lambda: d.Benchmark(args.steps, 100)))
    lines = ["# scripts/deferred_timing.py: B=%d S=%d hidden=%s replay=%d steps=%d; updates/s per leg and round" % (bench.B, bench.S, bench.HIDDEN, args.replay, args.steps)]
    vals = {k: [] for k, _ in legs}
    for r in range(args.rounds):
        for name, leg in legs:
            prewarm()
            ups = 1e3 / leg()
            vals[name].append(ups)
            lines.append("round %d %-8s %9.1f updates/s" % (r, name, ups))
            print(lines[-1], flush=True)
    for name, _ in legs:
        lines.append("%-8s min %.1f max %.1f" % (name, min(vals[name]), max(vals[name])))
    lines.append("deferred >= chained in every round: %s" % all(b >= a for a, b in zip(vals["chained"], vals["deferred"])))
    lines.append("deferred / headline: %s" % " ".join("%.4f" % (b / h) for b, h in zip(vals["deferred"], vals["headline"])))
    print("\n".join(lines[-5:]), flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    d.close()


if __name__ == "__main__":
    main()
