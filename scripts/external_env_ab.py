"""The external env handle (dqnhip_env_act_device + dqnhip_env_observe_device) beside the synthetic handle's single step, and the
synthetic step of this tree beside another build's (the parent commit) — the style of scripts/act_precision_ab.py.
   python scripts/external_env_ab.py [--pairs 5] [--workers 64,256,2048] [--parent TREE] [--out profiles/external_env_ab.md]
Part 1, one process: ONE fp16 learner (S = 58, 4x1024) alternates, `--pairs` times per point and acting precision, a window of
dqnhip_env_step(e, eps, 1) calls on a synthetic handle and a window of act_device + observe_device pairs on an external handle of
the same worker count (device buffers prepared beforehand: random rows, 1 % of the workers end an episode per step, as the synthetic
handle's p_end = 0.01).  Reported: us per call / per pair and their ratio — no threshold: the caller's simulator sits between act and
observe anyway.
Part 2 (--parent TREE, a built checkout of the commit to compare with): dqnhip_env_step at 64 workers, S = 68, 4x1024 fp32, one
fresh process per window, this tree and TREE alternating.  The synthetic step's kernels are unchanged text, so this tree's median
must lie inside TREE's own min .. max; anything else means shared device code changed what the compiler made of them.
Times are host clocks around work that ends in a device synchronise; every window follows an untimed one."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=HERE)
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--workers", default="64,256,2048")
ap.add_argument("--parent", default="")
ap.add_argument("--out", default="")
ap.add_argument("--child-step", action="store_true", help="part 2's window: print us per dqnhip_env_step of the tree at --root")
args = ap.parse_args()
root = os.path.abspath(args.root)
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
H = (1024, 1024, 1024, 1024)


def make_learner(S, precision):
    rng = np.random.default_rng(7)
    dqn = pkg.DQN(S, minibatch=128, hidden=H, memory=300000, seed=1, use_graph=True, precision=precision)
    for net in (0, 1):                                   # random weights (std 0.03: about 1 / sqrt(1024)), targets = copies
        w = dqn.get_params(net)
        dqn.set_params(net, (rng.standard_normal(w.size) * 0.03).astype(np.float32))
        dqn.CloneNet(net)
    return dqn


def step_window(env, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        env.step(0.1, 1)
    env.stats()                                          # waits for the stream
    return (time.perf_counter() - t0) / calls * 1e6


if args.child_step:
    dqn = make_learner(68, "fp32")
    env = pkg.EnvFrontEnd(dqn, 64, max_steps=100, seed=3)
    step_window(env, 500)
    print("US_PER_STEP %.3f" % statistics.median(step_window(env, 3000) for _ in range(3)), flush=True)
    env.close(); dqn.close()
    sys.exit(0)

lines = []
# ---- part 1 ----------------------------------------------------------------------------------------------------------------------
S = 58
hip = C.CDLL("libamdhip64.so")
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
hip.hipFree.argtypes = [C.c_void_p]


def to_device(arr):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), arr.nbytes) == 0
    assert hip.hipMemcpy(p, arr.ctypes.data_as(C.c_void_p), arr.nbytes, 1) == 0
    return p


def pair_window(env, bufs, calls):
    t0 = time.perf_counter()
    for i in range(calls):
        nx, st, pob = bufs["obs"][i % len(bufs["obs"])]
        env.act_device(0.1, bufs["action"], bufs["args"], None)
        env.observe_device(nx, st, pob)
    env.stats()
    return (time.perf_counter() - t0) / calls * 1e6


dqn = make_learner(S, "fp16")
rng = np.random.default_rng(3)
results = {}
for workers in [int(x) for x in args.workers.split(",") if x]:
    syn = pkg.EnvFrontEnd(dqn, workers, max_steps=100, seed=3)
    ext = pkg.ExternalEnv(dqn, workers, rng.uniform(-1, 1, size=(workers, S)).astype(np.float32), max_steps=100, seed=3)
    bufs = dict(action=to_device(np.zeros(workers, np.int32)), args=to_device(np.zeros(2 * workers, np.float32)), obs=[])
    for _ in range(8):
        status = (rng.uniform(size=workers) < 0.01).astype(np.int32) * 2
        pob = rng.choice([7, -1], size=workers).astype(np.int32)
        bufs["obs"].append((to_device(rng.uniform(-1, 1, size=(workers, S)).astype(np.float32)), to_device(status), to_device(pob)))
    calls = 2000 if workers <= 256 else 800
    for pair in range(args.pairs):
        for m in ("fp32", "fp16"):
            dqn.set_act_precision(m)
            step_window(syn, 100); pair_window(ext, bufs, 100)
            results.setdefault((workers, m, "step"), []).append(step_window(syn, calls))
            results.setdefault((workers, m, "pair"), []).append(pair_window(ext, bufs, calls))
    syn.close(); ext.close()
    for p in [bufs["action"], bufs["args"]] + [q for t in bufs["obs"] for q in t]:
        hip.hipFree(p)
dqn.set_act_precision("fp32")
dqn.close()


def cell(v):
    return "%.4g (%.4g .. %.4g)" % (statistics.median(v), min(v), max(v))


lines += ["fp16 learner, S = 58, 4x1024, us per call: median (min .. max) of %d alternating windows" % args.pairs, "",
          "| workers | acting | dqnhip_env_step(e, eps, 1) | act_device + observe_device | pair / step |", "|---|---|---|---|---|"]
for (workers, m, kind) in results:
    if kind == "step":
        a, b = results[(workers, m, "step")], results[(workers, m, "pair")]
        lines.append("| %d | %s | %s | %s | %.3f |" % (workers, m, cell(a), cell(b), statistics.median(b) / statistics.median(a)))

# ---- part 2 ----------------------------------------------------------------------------------------------------------------------
if args.parent:
    def child(tree):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-step", "--root", tree], capture_output=True, text=True, timeout=300)
        if out.returncode:
            raise SystemExit("window of %s failed:\n%s" % (tree, out.stderr[-2000:]))
        return float([ln for ln in out.stdout.splitlines() if ln.startswith("US_PER_STEP")][-1].split()[1])
    series = {"parent": [], "this": []}
    for pair in range(args.pairs):
        series["parent"].append(child(os.path.abspath(args.parent)))
        series["this"].append(child(HERE))
    lo, hi = min(series["parent"]), max(series["parent"])
    med = statistics.median(series["this"])
    lines += ["", "dqnhip_env_step at 64 workers, S = 68, 4x1024 fp32, us per step (one process per window, alternating):", "",
              "| build | windows | median (min .. max) |", "|---|---|---|"]
    for k in ("parent", "this"):
        lines.append("| %s | %s | %s |" % (k, ", ".join("%.2f" % v for v in series[k]), cell(series[k])))
    lines += ["", "this tree's median %s the parent's own spread (%.2f .. %.2f)" % ("lies inside" if lo <= med <= hi else "LIES OUTSIDE", lo, hi)]
text = "\n".join(lines)
print(text, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
