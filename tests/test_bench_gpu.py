"""bench.py's two kinds of run, on 4M-Ti at batch 8: a plain run prints the headline record and measures nothing else; ``--full`` adds the
per-kernel breakdown, the roofline and the parity record (its CPU baseline and rocprofv3 PMC passes switched off here to keep it to seconds)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "kernel_breakdown_ms_per_step", "kernel_tflops", "parity", "cpu_baseline", "extra")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--model", "fm_tiny_6e_6d_swiglu_nobias", "--batch", "8", *args], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_bench_py_plain_run_and_full(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    assert all(k in plain for k in HEADLINE) and plain["value"] > 0 and plain["steps"] == 2 and plain["warmup"] == 1
    assert not [k for k in FULL_ONLY if k in plain]
    full = _bench("--full", "--no-cpu-baseline", "--no-traffic", "--dump-outputs", str(tmp_path / "full"))
    assert {k: full[k] for k in ("metric", "unit", "higher_is_better", "dtype")} == {k: plain[k] for k in ("metric", "unit", "higher_is_better", "dtype")}
    assert full["roofline"]["achieved"] > 0 and full["kernel_breakdown_ms_per_step"]["sum_of_families"] > 0 and "parity" in full
    assert "cpu_baseline" not in full and full["roofline"]["traffic"] is None
    # --full adds work after the timed steps only: the two runs time and dump the same steps
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(os.listdir(tmp_path / "full"))
    for name in sorted(os.listdir(tmp_path / "plain")):
        if name != "params_sample.npy":      # (loss, per-modality losses, gradient norm: the dW reductions may add in either order)
            assert np.allclose(np.load(tmp_path / "plain" / name), np.load(tmp_path / "full" / name), rtol=1e-3), name
