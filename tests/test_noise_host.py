"""The noise body without a GPU.  tests/cpp/noise_host.cpp is a stand-alone program around the host build of
dqn-hfo_amd/csrc/noise_bodies.hip.h — the text the env kernels evaluate on the device.  It prints normal draws for a fixed key list,
three Ornstein-Uhlenbeck sequences, clipped terms and applied columns as float32 bit patterns.  Against tests/noise_ref.py: a draw is
equal or one float32 ulp away (the host libm's double log / cos against numpy's can land on the other side of a float32 rounding
boundary and can do no more than that); everything derived from a given z is equal bit for bit.  Built and run twice, plain and with
the address + undefined-behaviour sanitizers linked into the stand-alone binary (nothing is preloaded)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noise_ref as NR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "noise_host.cpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
F = np.float32


def _f(bits):
    return np.array([int(bits, 16)], np.uint32).view(F)[0]


def _same(a, b):
    return np.asarray(a, F).view(np.uint32) == np.asarray(b, F).view(np.uint32)


@pytest.mark.parametrize("suffix,extra", [("", ["-O2"]), ("_asan_ubsan", ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                                                                        "-Xarch_host", "-fno-sanitize-recover=undefined"])])
def test_host_build_of_the_noise_body(suffix, extra):
    exe = os.path.join(ROOT, "tests", "cpp", "noise_host" + suffix)
    cmd = [HIPCC, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unused-variable",
           "-I" + os.path.join(ROOT, "dqn-hfo_amd", "csrc"), "-o", exe, SRC] + extra
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "noise host OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    n = {k: 0 for k in "ZEOoCAR"}
    worst, equal = 0, 0
    ou = None
    for line in r.stdout.splitlines():
        t = line.split()
        if not t or t[0] not in n:
            continue
        n[t[0]] += 1
        if t[0] == "Z":
            got, want = _f(t[4]), NR.normal(int(t[1]), int(t[2]), [int(t[3])])[0]
            d = int(NR.ulps32(got, want))
            assert d <= 1 and abs(got) <= NR.Z_MAX, (t, float(got), float(want))
            worst, equal = max(worst, d), equal + (d == 0)
        elif t[0] == "E":
            got, want = _f(t[3]), NR.normal_of([int(t[1])], [int(t[2])])[0]
            assert np.isfinite(got) and abs(got) <= NR.Z_MAX and NR.ulps32(got, want) <= 1, (t, float(got), float(want))
        elif t[0] == "O":
            theta, sig = _f(t[1]), NR.sigmas(_f(t[2]), _f(t[3]))
            ou = dict(theta=theta, sigma=sig, seed=int(t[4]), w=int(t[5]), x=np.zeros(NR.NO, F))
        elif t[0] == "o":
            g, j, z, x = int(t[1]), int(t[2]), _f(t[3]), _f(t[4])
            want_z = NR.normal(ou["seed"], g, [ou["w"] * 32 + 2 * j])[0]
            assert NR.ulps32(z, want_z) <= 1, (t, float(want_z))
            want_x = NR.ou_step(ou["x"][j], ou["theta"], ou["sigma"][j], z)              # from the program's own z: bit for bit
            assert _same(x, want_x), (t, float(want_x))
            if ou["theta"] == 1:
                assert _same(x, ou["sigma"][j] * z)
            ou["x"][j] = x
        elif t[0] == "C":
            assert _same(_f(t[4]), NR.clipped(_f(t[1]), _f(t[2]), float(_f(t[3])))), t
        elif t[0] == "A":
            j, clamp, v, tt = int(t[1]), int(t[2]), _f(t[3]), _f(t[4])
            row, trow = np.zeros(NR.NO, F), np.zeros(NR.NO, F)
            row[j], trow[j] = v, tt
            want = NR.apply(row, trow, clamp)[j]
            assert _same(_f(t[5]), want), (t, float(want))
            if clamp:
                assert NR.MN[j] <= _f(t[5]) <= NR.MX[j]
        elif t[0] == "R":
            assert _f(t[2]) == NR.RANGE[int(t[1])] == (2, 2, 2, 2, 100, 360, 360, 360, 100, 360)[int(t[1])]
    assert n == {"Z": 3 * 4 * 4 * 10, "E": 25, "O": 3, "o": 3 * 20 * 10, "C": 54, "A": 10 * 2 * 7 * 6, "R": 10}, n
    assert equal >= 0.99 * n["Z"], (equal, n["Z"])          # the ulp allowance cannot hide a wrong key
    print("normal draws: worst distance", worst, "ulp,", equal, "of", n["Z"], "bit-equal")
