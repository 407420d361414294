"""bench.py's two kinds of run: a plain run reports the headline figure and nothing else; --full (off by default) adds the
per-kernel roofline, the other rates and configurations and the CPU baseline."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "roofline_hbm", "roofline_overall", "kernel_breakdown", "forward_only", "alt_dtype", "config4", "config5",
             "cpu_baseline")


def test_full_is_an_option():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout


@pytest.mark.gpu
def test_plain_run_reports_the_headline_only():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(k in line for k in HEADLINE), line
    assert line["unit"] == "images/sec" and line["higher_is_better"] is True and line["dtype"] == "f16"
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 2 and line["warmup"] == 1
    assert not set(FULL_ONLY) & set(line), sorted(set(FULL_ONLY) & set(line))
