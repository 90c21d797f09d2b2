"""The launch planning of the fp32 GEMM family (dqn-hfo_amd/csrc/gemm_plan.hip.h), without a GPU: the form table, what each form
accepts and the choosers learner.hip asks, compiled for the host and enumerated (tests/cpp/gemm_plan_host.cpp) — every form a chooser
returns accepts the launch it was chosen for, over every layer shape the config validation admits (524 288 forward and 131 072
backward cases), the choices at the measured shapes, and the shapes gemm_form_accepts turns down.  What the launches then compute:
tests/test_gpu_gemm_forms.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "gemm_plan_host")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_gemm_plan():
    src = os.path.join(ROOT, "tests", "cpp", "gemm_plan_host.cpp")
    cmd = [HIPCC, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-Wno-unused-variable",
           "-I" + os.path.join(ROOT, "dqn-hfo_amd", "csrc"), "-o", EXE, src]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "gemm plan host OK: 524288 forward and 131072 backward shapes" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
