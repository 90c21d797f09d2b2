"""The host side of the fp16 GEMM launches (dqn-hfo_amd/csrc/hgemm.hip.h), without a GPU: which tile hgemm_plan picks on either
side of the 192-tile thresholds for one problem and for two, tile_end for grouped problems of different shapes, every refusal of
hgemm_plan and of the launchers (all before a launch), hgemm_uses_small_tile, and the two block -> tile maps: hg_tile_of_block is
a bijection for every total up to 600, hg_tile_2d on every grid it accepts up to 32 x 64 tiles and false on the others
(tests/cpp/hgemm_plan_host.cpp).  What the kernels then compute: tests/test_gpu_hgemm_forms.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "hgemm_plan_host")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_hgemm_plan_and_tile_maps():
    src = os.path.join(ROOT, "tests", "cpp", "hgemm_plan_host.cpp")
    cmd = [HIPCC, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-Wno-unused-variable",
           "-I" + os.path.join(ROOT, "dqn-hfo_amd", "csrc"), "-o", EXE, src]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "hgemm plan host OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
