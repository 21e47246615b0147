"""`bench.py` with and without --full, each in a fresh process on a small batch: a plain run prints the headline line and
nothing that --full adds; --full (its long legs left out) adds the hipGraph launch-cost fit and the figures quoted from
profiles/."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, STEPS, WARMUP = 4096, 4, 2


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--envs-per-gpu", str(N), "--preroll", "16",
           "--steps", str(STEPS), "--warmup", str(WARMUP)] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone(tmp_path):
    out = _bench("--dump-outputs", str(tmp_path))
    assert out["full"] is False
    assert out["unit"] == "env-steps/s" and out["higher_is_better"] is True and out["dtype"]
    assert out["steps"] == STEPS and out["warmup"] == WARMUP
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert out["value"] * out["ms_per_step"] * 1e-3 == pytest.approx(N, rel=1e-9)
    for key in ("secondary", "cpu_baseline", "cpu_port", "from_profiles", "graph_launch_us"):
        assert key not in out, key
    assert out["sanity"]["graph_launch_fit"] is None
    assert out["roofline"]["pmc_passes"]["skipped"] is True and "valu_issue" not in out["roofline"]
    assert out["sanity"]["launch_mode"] in ("graph", "eager") and out["sanity"]["other_launch_mode"] is not None
    files = out["dump_outputs"]["files"]
    for name in ("quadrotor_obs", "quadrotor_reward", "quadrotor_reward64", "quadrotor_done", "quadrotor_failed"):
        a = np.load(os.path.join(str(tmp_path), name + ".npy"))
        assert list(a.shape) == files[name]["shape"] and a.shape[0] == N


@pytest.mark.gpu
def test_full_run_adds_the_launch_fit_and_the_quoted_figures():
    out = _bench("--full", "--no-pmc", "--no-secondary", "--no-cpu-baseline")
    assert out["full"] is True
    assert out["value"] * out["ms_per_step"] * 1e-3 == pytest.approx(N, rel=1e-9)
    fit = out["sanity"]["graph_launch_fit"]
    assert fit["k"] == [STEPS, 10 * STEPS] and "per_step_us_hip_events" in fit
    assert out["graph_launch_us"] == fit["fixed_us_per_timed_region_host_wall"]
    assert "from_profiles" in out
    assert out["roofline"]["pmc_passes"]["skipped"] is True
    assert "secondary" not in out and "cpu_baseline" not in out
