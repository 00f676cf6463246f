"""bench.py's plain run and its --dump-outputs (GPU): the headline line alone, and the last timed step's outputs on disk."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_last_step_outputs(tmp_path):
    """A plain run prints the headline without the --full measurements, and --dump-outputs writes the loss, logits and
    targets of both directions and the gradient sample / norms of the step it timed last: float32 / float64, < 64 MB,
    the loss equal to the one the line reports."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4",
           "--coin-patterns", "2", "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["roofline"] is None and not {"cpu_baseline", "f32_exact"} & set(d) and "per_pattern" not in d["config"]
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == {"loss", "pred_l2r", "gold_l2r", "pred_r2l", "gold_r2l", "grad_sample", "grad_norm"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) < 64 << 20
    assert abs(float(got["loss"]) - d["config"]["loss"]) < 1e-4
    assert got["pred_l2r"].shape == got["pred_r2l"].shape and got["pred_l2r"].shape[-1] == 58
    assert np.isfinite(got["grad_sample"]).all() and np.isfinite(got["grad_norm"]).all() and got["grad_norm"].max() > 0
