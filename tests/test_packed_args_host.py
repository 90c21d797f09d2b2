"""The host side of the packed GEMM launch arguments (GemmArgs, dqn-hfo_amd/csrc/gemm_common.hip.h), without a GPU: the
branch-free tile map equals the documented one and is a bijection for every tile count up to 48 x 9; pack_args() puts every
field of every problem where the kernels read it; tile accounting that does not hold together is refused before a launch
(tests/cpp/packed_args_host.cpp).  What the kernels then do with it: tests/test_gpu_packed_args.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "packed_args_host")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_tile_map_and_pack_args():
    src = os.path.join(ROOT, "tests", "cpp", "packed_args_host.cpp")
    cmd = [HIPCC, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-Wno-unused-variable",
           "-I" + os.path.join(ROOT, "dqn-hfo_amd", "csrc"), "-o", EXE, src]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "packed args host OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
