"""GPU: a plain `bench.py` run prints the headline line and writes --dump-outputs, nothing more; the other legs
(training step, kernel table, rooflines, other precisions, CPU baselines, other configurations) wait for --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = {"train", "kernels", "roofline", "parity_mode", "fp32_mode", "cpu_baseline", "speedup_vs_cpu",
             "max_rel_err_vs_cpu_fp32", "anomaly_eval", "scorer", "eval_1024px_tile", "drn_forward", "drn_train"}


def test_plain_bench_prints_the_headline_line_alone(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["metric"] == "HR Mpixels/sec DRCT-L x4 @128px HR (SR forward)" and line["unit"] == "HR Mpixels/s"
    assert line["higher_is_better"] is True and line["dtype"] == "bf16" and line["steps"] == 3 and line["warmup"] == 1
    assert line["value"] > 0 and line["value"] == pytest.approx(4 * 128 * 128 / (line["ms_per_step"] * 1e3), rel=1e-3)
    assert not FULL_ONLY & set(line), sorted(FULL_ONLY & set(line))
    sr = np.load(tmp_path / "sr.npy")
    assert line["dump_outputs"]["arrays"] == {"sr": [4, 1, 128, 128]} and sr.shape == (4, 1, 128, 128) and np.isfinite(sr).all()
