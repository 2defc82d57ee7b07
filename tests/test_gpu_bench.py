"""bench.py as it is run for every change: a plain run times the headline and measures nothing beside it, and
``--dump-outputs`` writes what the last timed step returned (the extra figures of ``--full``: tests/test_gpu_dp.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_the_last_step(tmp_path):
    dump = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "tiny", "--steps", "3", "--warmup", "2",
           "--dump-outputs", str(dump)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 2 and line["unit"] == "images/sec" and line["higher_is_better"] is True
    b = line["config"]["global_batch"]
    assert abs(line["value"] - b / (line["ms_per_step"] * 1e-3)) <= 1e-2 * line["value"]
    assert line["roofline"] is None and line["host_enqueue_ms_per_step"] is None
    assert "gd_only" not in line and "cpu_baseline" not in line
    files = {f[:-len(".npy")]: np.load(dump / f) for f in os.listdir(dump)}
    assert {"g_params", "d_params", "g_adam_m", "d_adam_v", "g_batch_stats", "d_spectral_norm_stats"} <= set(files)
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in files.values())
    assert sum(v.nbytes for v in files.values()) <= 64 << 20
    for k, v in line["losses"].items():
        assert round(float(files[k]), 4) == v, (k, float(files[k]), v)
