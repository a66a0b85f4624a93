"""A plain `bench.py --gpus 1 --steps K --warmup W` run: the headline line only (the passes behind --full are not
taken), K timed steps, and with --dump-outputs the last step's arrays as float32 .npy files."""

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FULL_ONLY = ("roofline", "hbm", "without_optimizer", "graphed_step", "fp32_operands", "cpu_baseline")


def test_plain_bench_line_and_dump(tmp_path):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--batch", "1", "--size", "128", "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["unit"] == "img/s" and line["higher_is_better"] is True
    assert line["dtype"] == "bf16" and line["value"] > 0 and line["ms_per_step"] > 0
    # value and ms_per_step describe the same 3 timed steps of 1 image
    assert line["value"] == pytest.approx(1 / (line["ms_per_step"] * 1e-3), rel=1e-2)
    assert not [k for k in FULL_ONLY if k in line], line
    got = {p.stem: np.load(p) for p in (tmp_path / "out").glob("*.npy")}
    assert set(got) == {"loss", "logits", "params", "buffers"}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert got["logits"].shape == (1, 2, 128, 128)
    assert float(got["loss"][0]) == pytest.approx(line["final_loss"], abs=1e-5)
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
