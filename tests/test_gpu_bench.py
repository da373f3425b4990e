"""`bench.py` on one GPU (tiny config): a plain run carries the headline alone, `--full` adds the untimed figures, and both
time the same steps on the same inputs, so the outputs they dump are identical."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "kernel_breakdown", "mfma_stages", "ranks", "collective", "secondary", "tolerance_mode",
             "cpu_baseline", "parity")


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--config", "tiny",
           "--dump-outputs", str(out_dir), *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-3000:]
    return json.loads(lines[0])


def test_bench_plain_run_is_the_headline_alone_and_full_adds_the_rest(tmp_path):
    plain = _bench(tmp_path / "plain")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain, k
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["value"] > 0 and plain["higher_is_better"] is True
    assert not [k for k in FULL_ONLY if k in plain]

    full = _bench(tmp_path / "full", "--full")
    assert {k: full[k] for k in ("metric", "unit", "dtype", "steps", "warmup", "config")} == \
           {k: plain[k] for k in ("metric", "unit", "dtype", "steps", "warmup", "config")}
    assert "roofline" in full and full["kernel_breakdown"]

    names = sorted(os.listdir(tmp_path / "plain"))
    assert "output_ids.npy" in names and names == sorted(os.listdir(tmp_path / "full"))
    for n in names:
        assert np.array_equal(np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)), n
