"""fp16 learner, ms per update by loss-scale mode (A/B inside one process, alternating; the style of scripts/fp16_ab.py):
   python scripts/loss_scale_ab.py [--root TREE] [--modes static,dynamic] [minibatches ...]
--root: load the package from another checkout of this repository (the parent commit, for the static-mode-costs-nothing table);
a tree from before loss_scale_mode existed is driven with --modes static only."""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--modes", default="static,dynamic")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--updates", type=int, default=200)
ap.add_argument("sizes", nargs="*", type=int)
args = ap.parse_args()
root = os.path.abspath(args.root)
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from synth import synth_replay  # noqa: E402

pkg = load_package()
modes = args.modes.split(",")
S, H = 58, (1024, 1024, 1024, 1024)
data = synth_replay(np.random.default_rng(7), 100000, S)
for B in args.sizes or [512, 4096]:
    ds = {}
    for m in modes:
        kw = {} if m == "static" else dict(loss_scale_mode=m)      # (static: also what a tree without the argument builds)
        ds[m] = pkg.DQN(S, minibatch=B, hidden=H, memory=200000, seed=1, use_graph=True, precision="fp16", **kw)
    for d in ds.values():
        d.add_transitions_arrays(*data)
        for _ in range(30):
            d.update_async(None)
        d.read_stats()
    res = {m: [] for m in ds}
    for rep in range(args.reps):
        for m, d in ds.items():
            t0 = time.perf_counter()
            for _ in range(args.updates):
                d.update_async(None)
            d.read_stats()
            res[m].append((time.perf_counter() - t0) / args.updates * 1e3)
    print("B=%d fp16 ms/update" % B, {m: ["%.4f" % x for x in v] for m, v in res.items()}, flush=True)
    for d in ds.values():
        d.close()
