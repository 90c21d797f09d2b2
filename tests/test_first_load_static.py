"""The kernarg preload's static claim, held against compiler updates: in the assembly of learner.hip — compiled as the library's
Makefile compiles it — every converted kernel's descriptor asks for preloaded kernargs, and along its preloaded path no scalar
wait stands between the real entry and the first vector load.  Nothing in the sources pins that order (the bodies' signatures
are fixed, so the argument reads cannot be placed between their loads); the compiler puts the GemmArgs reads behind the first
global_load today, and this test fails when it stops doing so.  scripts/first_load_chain.py does the counting."""
import importlib.util
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# kernel name prefix -> preload length
CONVERTED = {
    "void dqnhip::gemm_fwd_lds<4, 2, true, 1>(": 14, "void dqnhip::gemm_fwd_lds<2, 2, true, 2>(": 14, "void dqnhip::gemm_fwd_lds<1, 1, true, 2>(": 14,
    "void dqnhip::gemm_dgrad_lds<1, 1>(": 14, "void dqnhip::gemm_wgrad_tail<1>(": 14, "void dqnhip::gemm_wgrad_tail<10>(": 14,
    "void dqnhip::k_dgrad_qtrain<0>(": 14, "void dqnhip::k_dqda_head_bwd<false>(": 14, "void dqnhip::k_head_fwd<10, 0, true>(": 11,
}


def test_converted_kernels_reach_their_first_load_without_a_scalar_wait(tmp_path):
    spec = importlib.util.spec_from_file_location("first_load_chain", os.path.join(ROOT, "scripts", "first_load_chain.py"))
    chain = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chain)
    asm = str(tmp_path / "learner.s")
    csrc = os.path.join(ROOT, "dqn-hfo_amd", "csrc")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-mllvm", "-amdgpu-kernarg-preload-count=14",
                        "-o", asm, os.path.join(csrc, "learner.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = chain.listing(asm)
    for prefix, length in CONVERTED.items():
        found = [v for k, v in rows.items() if k.startswith(prefix)]
        assert len(found) == 1, (prefix, sorted(rows))
        _, _, _, _, preload, entry = found[0]
        print(prefix, "preload", preload, "entry path (waits, instructions)", entry)
        assert preload == length, (prefix, preload)
        assert entry is not None and entry[0] == 0, f"{prefix}: {entry[0]} scalar wait(s) before the first vector load on the preloaded path"
