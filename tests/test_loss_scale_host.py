"""The decision function of dynamic loss scaling (loss_scale_step, dqn-hfo_amd/csrc/learner_args.hip.h), without a GPU: the code the
optimiser launch runs in one lane, compiled for the host and enumerated (tests/cpp/loss_scale_host.cpp) — halving on a non-finite
norm, the finite-step counter reset on a skip, the report only at the floor with the multiplier staying there, growth exactly at
good == interval and none at interval 0, the cap, and 10 000 random steps against a restatement of the rule.  What the kernels then
do with the multipliers: tests/test_gpu_dynamic_loss_scale.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "loss_scale_host")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_loss_scale_step():
    src = os.path.join(ROOT, "tests", "cpp", "loss_scale_host.cpp")
    cmd = [HIPCC, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-Wno-unused-variable",
           "-I" + os.path.join(ROOT, "dqn-hfo_amd", "csrc"), "-o", EXE, src]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "loss scale host OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
