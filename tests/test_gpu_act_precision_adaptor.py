"""-act_precision fp16 through the adaptor (include/dqn.hpp + dqn_dropin.cpp), driven by tests/cpp/loss_scale_smoke.cpp as
tests/test_gpu_dynamic_loss_scale_adaptor.py drives its flag: the constructor applies dqnhip_set_act_precision after dqnhip_create and
the episode loop — SelectAction, AddTransitions, bursts of Update(), EvaluateAction — runs to its end on the fp16 acting path.  What
that path computes: tests/test_gpu_act_precision.py; the flag's CHECKs: tests/test_act_precision_host.py."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_dropin", "act_precision_smoke")
ARGS = ["-seed", "7", "-memory", "5000", "-memory_threshold", "100", "-loss_display_iter", "7", "-minibatch", "128", "-snapshot_freq", "100000"]


@pytest.mark.gpu
def test_flag_switches_the_adaptor_to_fp16_acting(pkg, gpu, tmp_path):
    lib = pkg.build()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "shim"),
           "-o", EXE, os.path.join(ROOT, "tests", "cpp", "loss_scale_smoke.cpp"), os.path.join(ROOT, "dqn-hfo_amd", "csrc", "dqn_dropin.cpp"),
           lib, "-Wl,-rpath," + os.path.dirname(lib)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    q = {}
    for mode in ("fp32", "fp16"):
        r = subprocess.run([EXE] + ARGS + ["-prefix", str(tmp_path / "agent0"), "-precision", "fp16", "-act_precision", mode],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (mode, r.returncode, r.stdout, r.stderr)
        assert "loss scale smoke OK" in r.stdout and "digest: actor_iter 60 critic_iter 60 memory_size 240" in r.stdout, r.stdout
        q[mode] = [float(v) for v in re.search(r"^q:(.*)$", r.stdout, re.M).group(1).split()]
        assert len(q[mode]) == 4 and all(v == v and abs(v) < 1e6 for v in q[mode]), q[mode]
    # another acting function: the stored actor outputs, hence the training data, hence the probed Q differ in their last digits
    assert q["fp32"] != q["fp16"]
