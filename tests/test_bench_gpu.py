"""bench.py's plain run (no --full): the headline line alone, --steps timed steps, and --dump-outputs writing what the
last timed step computed - the same inputs and the same arithmetic, hence the same files, from run to run of one
build."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, tmp_path):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=str(tmp_path), env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_reports_the_headline_and_dumps_the_last_step(dev, tmp_path):
    small = ["--gpus", "1", "--warmup", "1", "--batch", "8", "--t-out", "200", "--t-in", "40"]
    d1, d2, d3 = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "c")
    r1 = _bench(small + ["--steps", "3", "--dump-outputs", d1], tmp_path)
    assert r1["steps"] == 3 and r1["warmup"] == 1 and r1["n_gpus"] == 1
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in r1, k
    assert r1["higher_is_better"] is True and r1["unit"] == "mel-frames/s" and r1["dtype"] == "bf16"
    assert abs(r1["value"] - 8 * 200 / (r1["ms_per_step"] * 1e-3)) < 1e-6 * r1["value"]
    # the plain run measures the headline only: what takes runs of its own is behind --full
    for k in ("roofline", "roofline_gemm_family", "phases_ms", "real_dynamics", "griffin_lim", "cpu_baseline"):
        assert k not in r1, k
    names = sorted(f for f in os.listdir(d1))
    assert names == sorted(n + ".npy" for n in ("losses", "mel_outputs", "decoder_outputs", "linear_outputs",
                                                 "alignments", "gradients", "parameters")), names
    total = 0
    for f in names:
        a = np.load(os.path.join(d1, f))
        assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all(), f
        total += a.nbytes
    assert total <= 64 << 20, total
    assert np.load(os.path.join(d1, "mel_outputs.npy")).shape == (8, 200, 80)
    losses = np.load(os.path.join(d1, "losses.npy"))
    assert abs(losses[0] - r1["config"]["loss"]) < 1e-9 * abs(losses[0]), (losses, r1["config"]["loss"])
    # the same arguments give the same inputs, the same model and - the split-K slices added in a fixed order - the
    # same arithmetic: two runs dump the same numbers (to rounding: the loss scalars are fp32 atomic sums)
    r2 = _bench(small + ["--steps", "3", "--warmup", "1", "--dump-outputs", d2], tmp_path)
    r3 = _bench(small + ["--steps", "3", "--warmup", "1", "--dump-outputs", d3], tmp_path)
    assert r2["steps"] == 3 and r2["config"]["deterministic_gradients"] is True
    for f in names:
        a, b = np.load(os.path.join(d2, f)), np.load(os.path.join(d3, f))
        assert a.shape == b.shape, f
        assert np.abs(a.astype(np.float64) - b).max() <= 1e-6 * np.abs(a).max(), f
