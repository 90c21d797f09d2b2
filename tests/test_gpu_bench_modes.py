"""bench.py's two modes on one GPU: a plain run measures the headline and nothing else; --full adds every other record
(the one-update-per-launch rate, the roofline, env steps, the CPU baseline, the drop-in's blocking forms, the side records)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "20", "--warmup", "5", "--replay", "20000"]


def run_bench(args, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_measures_the_headline_only(pkg, gpu, tmp_path):
    d = run_bench(SMALL + ["--dump-outputs", str(tmp_path)], timeout=300)
    assert d["metric"].startswith("DQN updates/sec") and d["unit"] == "updates/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == 20 and d["warmup"] == 5 and d["n_gpus"] == 1
    assert d["value"] > 100 and abs(d["value"] * d["ms_per_step"] - 1e3) < 1.0
    assert d["full"] is False
    assert d["roofline"] is None and d["env_steps"] is None and d["cpu_baseline"] is None and d["sub_records"] is None
    assert "ms_per_step_one_update_per_graph_launch" not in d["config"]
    # nothing runs after the timed steps: the line's last update is the one --dump-outputs wrote
    assert np.load(tmp_path / "critic_loss.npy")[0] == np.float32(d["last_critic_loss"])
    assert np.load(tmp_path / "avg_q.npy")[0] == np.float32(d["last_avg_q"])


def test_full_run_keeps_every_record(pkg, gpu):
    d = run_bench(SMALL + ["--full", "--no-live-trace", "--no-live-pmc"], timeout=900)
    assert d["full"] is True and d["value"] > 100
    assert d["config"]["ms_per_step_one_update_per_graph_launch"] > 0
    roof = d["roofline"]
    assert roof["bound"] == "mfma" and 0 < roof["frac"] < 1 and roof["families_us"]
    assert d["env_steps"]["workers_64"]["env_steps_per_s"] > 0 and d["env_steps"]["cpu_port_workers_64"]["env_steps_per_s"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["ref_shape"]["threads_all"]
    sub = d["sub_records"]
    assert "error" not in sub, sub
    for key in ("configs4_1gpu_b4096_fp16", "configs4_1gpu_b4096_fp32", "configs1_shape_b256_fp16", "two_agents_one_gpu_b256_fp32",
                "configs0_ref_defaults_b32", "configs2_64workers_s68", "train_loop", "configs4_rank_shape_b512", "dropin_blocking_b256"):
        assert key in sub, (key, sorted(sub))
    assert sub["dropin_blocking_b256"]["blocking_ms_per_update"] > 0
