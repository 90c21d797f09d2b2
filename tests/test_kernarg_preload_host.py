"""The kernarg preload blocks without a GPU (tests/cpp/kernarg_preload_host.cpp): the 14 words the chain kernels receive in SGPRs at
wave launch, built from a packed GemmArgs and decoded by the functions the kernels call (__host__ __device__ functions of
gemm_bodies.hip.h): preload_decode for the grouped forms of gemm_fwd_lds / gemm_dgrad_lds (one problem, a pair of equal shape),
preload_record_decode for the record form of gemm_wgrad_tail and k_dgrad_qtrain (every block of the tail's grid, the blocks in
front of and behind the record included).  The decode equals the packed fields for every tile — tile counts up to pack_args()'
own limits, leading dimensions up to kMaxLeadingDim; three or four problems, pairs that differ in ldp, ldq, Kred or a tile
count, the tuning bit, and every value a field cannot hold give the all-zero "not valid" block.  Likewise k_dqda_head_bwd's block
(DqdaPreload, head_kernels.hip.h) against the DqdaHeadArgs it is taken from.  The same program once more under
AddressSanitizer + UBSan, stand-alone.  What the kernels then do with it: tests/test_gpu_kernarg_preload.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "kernarg_preload_host.cpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.parametrize("suffix,extra", [("", ["-O2"]), ("_asan_ubsan", ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                                                                        "-Xarch_host", "-fno-sanitize-recover=undefined"])])
def test_preload_block_and_decode(suffix, extra):
    exe = os.path.join(ROOT, "tests", "cpp", "kernarg_preload_host" + suffix)
    cmd = [HIPCC, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unused-variable",
           "-I" + os.path.join(ROOT, "dqn-hfo_amd", "csrc"), "-o", exe, SRC] + extra
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "kernarg preload host OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
