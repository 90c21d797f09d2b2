"""What the update diagnostics (dqnhip_diag_collect) cost, at the BASELINE shape: B = 256, 4 x 1024, S = 58, 1 M transitions filled, fp32,
one process, after warm-up.  Writes the tables to profiles/diagnostics_ab.md (--out):
   python scripts/diag_ab.py [--calls 200] [--pairs 5] [--updates 4000] [--every 1000] [--fill 1000000] [--parent DIR] [--bench-pairs 3] [--out FILE]
 (a) one collection: HIP events on the learner's stream around the call (its three launches, the read-back of the report and the
     host's wait are all inside) and the host's wall time, beside the bytes it reads, computed from the shapes;
     --trace-child: only warm up and run `calls` collections, for a `rocprofv3 --kernel-trace --stats` run of its own (the three
     kernels' own durations);
 (b) update_async_n bursts with a collection every `every` updates against never, alternating pairs;
 (c) with --parent DIR (a checkout of the parent commit with its library built): `python bench.py --gpus 1` there and here,
     alternating, the plain learner's rate beside the parent's own run-to-run spread."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--updates", type=int, default=4000)
ap.add_argument("--every", type=int, default=1000)
ap.add_argument("--fill", type=int, default=1000000)
ap.add_argument("--minibatch", type=int, default=256)
ap.add_argument("--parent", default=None)
ap.add_argument("--bench-pairs", type=int, default=3)
ap.add_argument("--bench-steps", type=int, default=2000)
ap.add_argument("--bench-warmup", type=int, default=200)
ap.add_argument("--out", default=None)
ap.add_argument("--trace-child", action="store_true")
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


def make():
    d = pkg.DQN(S, minibatch=B, hidden=H, memory=args.fill + 1, seed=1, use_graph=True)
    for _ in range(args.fill // 100000):
        d.add_transitions_arrays(*chunk)
    return d


hip = C.CDLL("libamdhip64.so")


def bytes_read(d):
    """from the shapes: five arenas of both online nets as stored (pad words included: they are loaded), the 5 x L panels, the rows"""
    pad = lambda x, m: (x + m - 1) // m * m
    arena = 0
    for in_dim, nh in ((S, 10), (S + 10, 1)):
        k = pad(in_dim, 64)
        for n in H:
            arena += n * k + n
            k = n
        arena += nh * k + nh
    panels = 5 * sum(H) * B
    rows = B * (4 + 1 + 16 + 16)
    return 5 * 4 * arena, 4 * panels, 4 * rows


if args.trace_child:
    d = make()
    d.update_async_n(64)
    for _ in range(args.calls):
        d.diag_collect_raw()
    d.close()
    sys.exit(0)

plain, diag = make(), make()
emit("# Update diagnostics: what a collection costs (scripts/diag_ab.py)")
emit()
emit("B = %d, hidden %s, S = %d, %d transitions filled, fp32, one process." % (B, "x".join(map(str, H)), S, plain.memory_size()))
emit("plan (never collects): %s" % plain.update_plan())
emit("plan (collects):       %s" % diag.update_plan())
emit()
for d in (plain, diag):
    d.update_async_n(256)
    d.read_stats()
for _ in range(10):
    diag.diag_collect_raw()

# (a)
stream = C.c_void_p(diag.stream())
ev = [C.c_void_p() for _ in range(2)]
for e in ev:
    assert hip.hipEventCreate(C.byref(e)) == 0
r = pkg.capi.DiagReport()
r.struct_size = C.sizeof(pkg.capi.DiagReport)
walls, evs = [], []
for _ in range(args.calls):
    assert hip.hipEventRecord(ev[0], stream) == 0
    t0 = time.perf_counter()
    assert diag.lib.dqnhip_diag_collect(diag.h, C.byref(r)) == 0
    walls.append(time.perf_counter() - t0)
    assert hip.hipEventRecord(ev[1], stream) == 0 and hip.hipEventSynchronize(ev[1]) == 0
    ms = C.c_float()
    assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
    evs.append(ms.value * 1e-3)
ba, bp, br = bytes_read(diag)
med_ev, med_wall = float(np.median(evs)), float(np.median(walls))
emit("## (a) one collection, %d calls" % args.calls)
emit()
emit("Bytes read, from the shapes: arenas 5 x %.2f M floats = %.1f MB, panels %.1f MB, rows %.3f MB: %.1f MB." %
     (ba / 20e6, ba / 1e6, bp / 1e6, br / 1e6, (ba + bp + br) / 1e6))
emit("Event time brackets the whole call on the learner's stream: three launches, three device-to-host copies (about %d KB) and the host's wait." %
     ((C.sizeof(pkg.capi.DiagReport) + 1023) // 1024))
emit()
emit("| | median us | min us | max us | GB/s at the median |")
emit("|---|---|---|---|---|")
emit("| device events around the call | %.1f | %.1f | %.1f | %.0f |" % (med_ev * 1e6, min(evs) * 1e6, max(evs) * 1e6, (ba + bp + br) / med_ev / 1e9))
emit("| host wall time of the call | %.1f | %.1f | %.1f | %.0f |" % (med_wall * 1e6, min(walls) * 1e6, max(walls) * 1e6, (ba + bp + br) / med_wall / 1e9))
emit()
# the optimiser launches' own time, for the comparison: timing mode, eager launches
timed = pkg.DQN(S, minibatch=B, hidden=H, memory=200001, seed=1, use_graph=False)
timed.add_transitions_arrays(*chunk)
timed.UpdateActorCritic()
timed.set_kernel_timing(True)
for _ in range(50):
    timed.update_async(None)
timed.read_stats()
ms, n = timed.kernel_timing("adam")
emit("The optimiser launches of this learner (timing family `adam`, %d eager launches): %.1f us each, %.1f us for the two of an update." % (n, ms * 1e3, 2 * ms * 1e3))
timed.close()
emit()

# (b)
emit("## (b) update_async_n bursts of %d updates: a collection every %d updates against never, %d alternating pairs" % (args.updates, args.every, args.pairs))
emit()
emit("| pair | never: updates/s | collecting: updates/s | collecting / never |")
emit("|---|---|---|---|")
ratios, rates = [], {"plain": [], "diag": []}
for p in range(args.pairs):
    rate = {}
    for name, d in (("plain", plain), ("diag", diag)):
        t0 = time.perf_counter()
        for _ in range(args.updates // args.every):
            d.update_async_n(args.every)
            if name == "diag":
                d.diag_collect_raw()
        d.read_stats()
        rate[name] = args.updates / (time.perf_counter() - t0)
        rates[name].append(rate[name])
    ratios.append(rate["diag"] / rate["plain"])
    emit("| %d | %.0f | %.0f | %.4f |" % (p + 1, rate["plain"], rate["diag"], ratios[-1]))
emit()
emit("collecting / never: median %.4f (min %.4f, max %.4f); spread of `never` itself: %.4f (max / min)." %
     (float(np.median(ratios)), min(ratios), max(ratios), max(rates["plain"]) / min(rates["plain"])))
plain.close(); diag.close()

# (c)
if args.parent:
    emit()
    emit("## (c) `python bench.py --gpus 1 --steps %d --warmup %d`: the parent commit's tree and this one, alternating" % (args.bench_steps, args.bench_warmup))
    emit()
    emit("| pair | parent updates/s | this tree updates/s |")
    emit("|---|---|---|")
    res = {"parent": [], "here": []}
    for p in range(args.bench_pairs):
        for name, cwd in (("parent", args.parent), ("here", root)):
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)],
                                 cwd=cwd, capture_output=True, text=True, timeout=600)
            rec = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
            assert out.returncode == 0 and rec, (name, out.returncode, out.stderr[-2000:])
            res[name].append(float(rec[-1]["value"]))
        emit("| %d | %.1f | %.1f |" % (p + 1, res["parent"][-1], res["here"][-1]))
    emit()
    for name in ("parent", "here"):
        v = res[name]
        emit("%s: median %.1f, min %.1f, max %.1f (spread %.4f)" % (name, float(np.median(v)), min(v), max(v), max(v) / min(v)))
    med = float(np.median(res["here"]))
    emit("this tree's median lies %s the parent's own run-to-run range." % ("below" if med < min(res["parent"]) else "above" if med > max(res["parent"]) else "inside"))
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
