"""bench.py's command line on a GPU: a plain run times exactly --steps steps and prints the headline
fields alone; --dump-outputs writes the last timed step's output; --full adds the roofline pass,
the CPU baseline and the parity.  Short runs of the flagship gen64 workload (B = 256).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "fft_roofline", "cpu_baseline", "parity", "kernels")


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *argv], capture_output=True,
                       text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_outputs(tmp_path):
    line = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY)
    assert line["steps"] == 3 and line["unit"] == "images/s" and line["dtype"] == "f32" and line["higher_is_better"]
    # value is the global batch over the wall time of the timed steps, ms_per_step that time per step
    assert line["value"] == pytest.approx(256 / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert os.listdir(tmp_path) == ["images.npy"]
    img = np.load(tmp_path / "images.npy")
    assert img.dtype == np.float32 and img.shape == (256, 3, 64, 64)
    assert np.isfinite(img).all() and np.abs(img).max() <= 1.0 and img.std() > 0   # tanh head


def test_full_run_carries_roofline_baseline_and_parity():
    line = _bench("--full", "--global-batch", "32", "--steps", "3", "--warmup", "1", "--cpu-seconds", "0.1",
                  "--profile-steps", "1")
    assert all(k in line for k in HEADLINE + FULL_ONLY)
    assert line["parity"]["normwise_err_vs_cpu_ref"] <= line["parity"]["tolerance"]
    assert line["cpu_baseline"]["value"] > 0 and line["roofline"]["frac"] > 0 and line["kernels"]
