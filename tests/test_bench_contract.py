"""The driver depends on bench.py's JSON contract: one line from rank 0
with the documented fields. Run a tiny configuration and validate the
shape strictly."""

import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from containerpilot_amd import REPO_ROOT


def test_bench_json_contract(tmp_path):
    dump = tmp_path / "outputs"
    result = subprocess.run(
        [sys.executable, os.path.join(REPO_ROOT, "bench.py"),
         "--steps", "2", "--warmup", "1", "--jobs", "10", "--watches", "2",
         "--dump-outputs", str(dump)],
        capture_output=True, text=True, timeout=300, cwd=REPO_ROOT)
    assert result.returncode == 0, result.stdout + result.stderr
    lines = [ln for ln in result.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, result.stdout
    doc = json.loads(lines[0])

    for field in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                  "ms_per_step", "higher_is_better", "scaling",
                  "vs_baseline", "dtype", "data", "config"):
        assert field in doc, field
    assert doc["metric"] == "events/sec"
    assert doc["n_gpus"] == 1
    assert doc["steps"] == 2
    assert doc["warmup"] == 1
    assert doc["higher_is_better"] is True
    assert doc["scaling"] == "weak"
    assert doc["value"] > 0
    assert doc["vs_baseline"] == round(doc["value"] / 10000.0, 3)
    assert 900 < doc["ms_per_step"] < 1500  # a step is one second
    assert "p99_dispatch_ms" in doc["config"]
    assert doc["config"]["jobs"] == 10

    # --dump-outputs: which event series published in the last timed
    # step, as float64 .npy; determined by the config, not by timing
    arrays = {p.stem: np.load(p) for p in dump.glob("*.npy")}
    assert sorted(arrays) == [
        "job_series_active_last_step", "other_series_active_last_step",
        "watch_series_active_last_step"]
    assert all(a.dtype == np.float64 for a in arrays.values())
    # every job's 100 ms check exits 0 and reports healthy each step
    assert np.array_equal(arrays["job_series_active_last_step"],
                          np.ones((10, 2)))
    # the upstream set is stable, so the watches publish nothing
    assert np.array_equal(arrays["watch_series_active_last_step"],
                          np.zeros((2, 2)))
    assert np.array_equal(arrays["other_series_active_last_step"], [0.0])


def test_bench_setup_validates_config_natively():
    """Set-up runs the generated config through the native library's
    validator before any daemon starts: a zero check interval is
    rejected with the daemon's own message."""
    sys.path.insert(0, REPO_ROOT)
    import bench
    args = argparse.Namespace(jobs=2, watches=1, check_ms=0)
    with pytest.raises(RuntimeError, match="health.interval must be > 0"):
        bench.run_rank(args, 0)
