"""fp16 learner, acting precision A/B inside one process (the style of scripts/loss_scale_ab.py): ONE fp16 learner (S = 58, 4x1024)
alternates dqnhip_set_act_precision between fp32 and fp16, `--pairs` times per point:
   env-steps/s of the batched env front-end at 64 / 256 / 1024 / 2048 workers, and dqnhip_select_actions_device at n = 256 / 4096.
   python scripts/act_precision_ab.py [--root TREE] [--modes fp32,fp16] [--pairs 5] [--out FILE.md]
--root: load the package from another checkout of this repository (the parent commit, for the default-is-unchanged table); a tree
from before the switch existed is driven with --modes fp32 only.  Times are host clocks around work that ends in a device
synchronise; every window is preceded by an untimed one in the same mode (the env recaptures its step graphs after a switch)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--modes", default="fp32,fp16")
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--workers", default="64,256,1024,2048")
ap.add_argument("--rows", default="256,4096")
ap.add_argument("--out", default="")
args = ap.parse_args()
root = os.path.abspath(args.root)
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
modes = args.modes.split(",")
S, H = 58, (1024, 1024, 1024, 1024)
rng = np.random.default_rng(7)
dqn = pkg.DQN(S, minibatch=128, hidden=H, memory=300000, seed=1, use_graph=True, precision="fp16")
for net in (0, 1):                                       # random weights (std 0.03: about 1 / sqrt(1024)), targets = copies
    w = dqn.get_params(net)
    dqn.set_params(net, (rng.standard_normal(w.size) * 0.03).astype(np.float32))
    dqn.CloneNet(net)


def set_mode(m):
    if hasattr(dqn, "set_act_precision"):
        dqn.set_act_precision(m)
    elif m != "fp32":
        raise SystemExit("this tree has no act_precision switch: --modes fp32")


hip = C.CDLL("libamdhip64.so")
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]
results = {}                                             # (point, mode) -> [value per pair]


def env_window(env, steps):
    t0 = time.perf_counter()
    env.step(0.1, steps)
    env.stats()                                          # waits for the stream
    return env.N * steps / (time.perf_counter() - t0)


def act_window(ds, do, n, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        dqn._ck(dqn.lib.dqnhip_select_actions_device(dqn.h, ds, n, do))
    assert hip.hipDeviceSynchronize() == 0
    return (time.perf_counter() - t0) / calls * 1e6


for workers in [int(x) for x in args.workers.split(",") if x]:
    env = pkg.EnvFrontEnd(dqn, workers, max_steps=100, seed=3)
    steps = 4800 if workers <= 256 else 1600             # >= 0.1 s per window at either end
    for pair in range(args.pairs):
        for m in modes:
            set_mode(m)
            env_window(env, 160)
            results.setdefault(("env %d workers, env-steps/s" % workers, m), []).append(env_window(env, steps))
    env.close()
for n in [int(x) for x in args.rows.split(",") if x]:
    x = rng.uniform(-1, 1, size=(n, S)).astype(np.float32)
    ds, do = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(ds), x.nbytes) == 0 and hip.hipMalloc(C.byref(do), n * 40) == 0
    assert hip.hipMemcpy(ds, x.ctypes.data_as(C.c_void_p), x.nbytes, 1) == 0
    for pair in range(args.pairs):
        for m in modes:
            set_mode(m)
            act_window(ds, do, n, 50)
            results.setdefault(("select_actions_device n = %d, us/call" % n, m), []).append(act_window(ds, do, n, 1000))
    hip.hipFree(ds); hip.hipFree(do)
set_mode("fp32")
dqn.close()


def cell(v):
    return "%.4g (%.4g .. %.4g)" % (statistics.median(v), min(v), max(v))


points = []
for (p, m) in results:
    if p not in points:
        points.append(p)
lines = ["| point | " + " | ".join("%s: median (min .. max) of %d" % (m, args.pairs) for m in modes) + (" | fp16 / fp32 |" if len(modes) == 2 else " |"),
         "|---|" + "---|" * (len(modes) + (1 if len(modes) == 2 else 0))]
cross = None
for p in points:
    row = "| %s | " % p + " | ".join(cell(results[(p, m)]) for m in modes)
    if len(modes) == 2:
        ratio = statistics.median(results[(p, modes[1])]) / statistics.median(results[(p, modes[0])])
        row += " | %.3f" % ratio
        if p.startswith("env") and ratio > 1.0 and cross is None:
            cross = p.split()[1]
    lines.append(row + " |")
if len(modes) == 2:
    lines.append("")
    lines.append("crossover (smallest measured worker count at which fp16 acting gives more env-steps/s): %s" % (cross or "none measured"))
text = "\n".join(lines)
print(text, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
