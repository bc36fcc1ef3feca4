"""bench.py on the device: a plain run carries the headline line only and `--dump-outputs` writes the last timed step; `--full` adds the
CPU baseline and the parity check against the oracle.  Config c1 (n = 64, m = 128): seconds per run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c1"] + args, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_and_dumped_outputs(gpu, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    out = _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", str(a)])
    assert out["metric"] == "ADMM iterations/sec" and out["unit"] == "iterations/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["steps"] == 3 and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(out["config"]["admm_iterations_per_step"] / (out["ms_per_step"] / 1e3), rel=1e-3)
    assert out["config"]["full"] is False and out["cpu_baseline"] is None and out["parity"] is None
    dumped = {k: np.load(a / f"{k}.npy") for k in ("x", "z", "y")}
    assert {k: (v.dtype, v.shape) for k, v in dumped.items()} == {"x": (np.float64, (64,)), "z": (np.float64, (128,)), "y": (np.float64, (128,))}
    assert all(np.isfinite(v).all() for v in dumped.values()) and np.abs(dumped["x"]).max() > 0
    # every step starts from x = 0 on the same seeded problem: another run with another step count ends on the same iterate
    _bench(["--steps", "2", "--warmup", "0", "--dump-outputs", str(b)])
    for k, v in dumped.items():
        np.testing.assert_allclose(np.load(b / f"{k}.npy"), v, rtol=1e-12, atol=1e-12 * max(1.0, np.abs(v).max()))


def test_full_run_adds_the_cpu_baseline_and_parity(gpu):
    out = _bench(["--steps", "2", "--warmup", "1", "--full"])
    assert out["config"]["full"] is True and out["steps"] == 2 and out["ms_per_step"] > 0
    assert out["cpu_baseline"]["value"] > 0 and out["parity"]["ok"] is True, out["parity"]
