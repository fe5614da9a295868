"""bench.py's two kinds of run on a small DEM: a plain run does the headline only (set-up, warm-up, the timed steps,
--dump-outputs, the result line); --full adds what the headline does not need, after the timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--ny", "1024", "--nx", "1024", "--steps", "3", "--warmup", "2"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("cpu_baseline", "cpu_baseline_all_cores", "parity_spot", "descriptors", "descriptors_at_config_sizes",
             "end_to_end")


def bench(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *args], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_plain_run_is_the_headline_only(tmp_path):
    line = bench("--dump-outputs", str(tmp_path))
    for key in HEADLINE:
        assert key in line, key
    assert line["unit"] == "Mpixels/s" and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 3 and line["warmup"] == 2
    assert not set(FULL_ONLY) & set(line), set(FULL_ONLY) & set(line)
    assert "hbm_copy_live" not in line["roofline"]
    tpi, rows = np.load(tmp_path / "tpi.npy"), np.load(tmp_path / "tpi_rows.npy")
    assert tpi.shape == (1024, 1024) and tpi.dtype == np.float32 and np.array_equal(rows, np.arange(1024))


def test_full_run_adds_the_side_tables():
    # (--no-cpu: the CPU baselines and parity spots cut 16384- and 4096-row windows out of the bench DEM)
    line = bench("--full", "--no-cpu", "--no-end-to-end")
    for key in HEADLINE:
        assert key in line, key
    assert "ms" in line["roofline"]["hbm_copy_live"]
    assert line["descriptors"]["tpi_s67"]["ms"] > 0
    assert line["descriptors_at_config_sizes"]["config2_8192_tpi_s7"]["ms"] > 0
    assert "cpu_baseline" not in line and "end_to_end" not in line
