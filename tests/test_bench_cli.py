"""bench.py's two forms: a plain run is the headline leg alone (set up, warm up, timed steps, --dump-outputs, the JSON line); --full adds
the legs that take runs of their own (prepass off, low-precision compute, clock probe, latencies, pose-only, CPU baseline) after it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("prepass_off", "lp_compute", "latency_ms_p50", "latency_kitti_size_ms_p50", "latency_one_shot_ms_p50", "pose_only", "cpu_baseline")


def test_full_is_off_by_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert a.full is False and (a.steps, a.warmup) == (3, 1)
    assert bench.parse_args(["--full"]).full is True


def _run(args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_leg_and_full_adds_the_rest(tmp_path):
    """Same small batch twice: plain, then --full without the CPU baseline.  The headline computes the same thing in both (identical dumped
    results, same metric / unit / dtype); only the --full line carries the other legs, and its legs start with the headline's two."""
    base = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--objects-per-gpu", "8"]
    plain = _run(base + ["--dump-outputs", str(tmp_path / "plain")])
    full = _run(base + ["--full", "--no-cpu-baseline", "--latency-runs", "1", "--dump-outputs", str(tmp_path / "full")])

    assert plain["full"] is False and full["full"] is True
    for k in ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup"):
        assert plain[k] == full[k], k
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["config"]["objects_good"] == full["config"]["objects_good"] > 0
    for k in FULL_ONLY:
        assert k not in plain, k
    assert plain["value_lp"] is None
    assert [lg["leg"] for lg in plain["roofline"]["rocprof_check"]["legs"]] == ["headline_warmup", "headline_timed"]

    legs = [lg["leg"] for lg in full["roofline"]["rocprof_check"]["legs"]]
    assert legs[:2] == ["headline_warmup", "headline_timed"] and "lp_compute_timed" in legs and "clock_probe" in legs
    assert full["lp_compute"]["value"] > 0 and full["value_lp"] == full["lp_compute"]["value"]
    assert full["latency_ms_p50"] > 0 and full["latency_kitti_size_ms_p50"] > 0 and "objects_per_s" in full["pose_only"]
    if full["dtype"] != "f32":      # the prepass ran: its fp32-only twin is timed in --full
        assert full["prepass_off"]["value"] > 0 and full["value_fp32_only"] == full["prepass_off"]["value"]
        assert plain["value_fp32_only"] is None
    assert "cpu_baseline" not in full

    names = sorted(os.listdir(str(tmp_path / "plain")))
    assert names == sorted(os.listdir(str(tmp_path / "full"))) and "t_cam_obj.npy" in names
    for f in names:
        assert np.array_equal(np.load(str(tmp_path / "plain" / f)), np.load(str(tmp_path / "full" / f))), f
