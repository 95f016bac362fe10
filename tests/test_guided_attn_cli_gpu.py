"""train.py with --hparams guided_attention_weight=..., on the tiny synthetic corpus of tests/test_cli_gpu.py (built the
same way): the feeder's frame counts reach the model through both loops (the pipelined one and the synchronous summary
steps), events.jsonl carries the two alignment scores, and the logged loss is the total."""
import json
import os
import re
import subprocess
import sys
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ("embedding_dim=32,encoder_conv_channels=64,encoder_lstm_units=32,attention_dim=64,decoder_lstm_units=64,"
         "postnet_conv_channels=64,expand_conv_channels=64,expand_lstm_units=32,batch_size=2,batch_group_size=2,max_iters=60")


def _corpus(tmp):
    os.makedirs(os.path.join(tmp, "wavs"))
    rng = np.random.default_rng(0)
    lines = []
    for i, text in enumerate(["Hello world.", "Dr. Smith met Mr. Jones!", "A short one.", "The quick brown fox jumps."]):
        L = int(20000 * rng.uniform(0.5, 0.9))
        t = np.arange(L) / 20000.0
        y = 0.5 * np.sin(2 * np.pi * 180 * t) * (0.5 + 0.5 * np.sin(2 * np.pi * 3 * t)) + rng.normal(0, 0.01, L)
        with wave.open(os.path.join(tmp, "wavs", "utt%d.wav" % i), "wb") as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(20000)
            f.writeframes((np.clip(y, -1, 1) * 32767).astype("<i2").tobytes())
        lines.append("utt%d|%s|%s" % (i, text, text))
    with open(os.path.join(tmp, "metadata.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")


def _train(tmp_path, model, hparams, precision, steps, summary_interval):
    data = str(tmp_path / "lj")
    os.makedirs(data)
    _corpus(data)
    logs = str(tmp_path / "logs")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--ljspeech", data, "--model", model, "--log_dir", logs,
                        "--hparams", hparams, "--checkpoint_interval", "1000", "--precision", precision,
                        "--summary-interval", str(summary_interval), "--max_steps", str(steps)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    ev = [json.loads(l) for l in open(os.path.join(logs, "logs-%s" % model, "events.jsonl"))]
    logged = {int(m.group(1)): float(m.group(2)) for m in re.finditer(r"Step (\d+)\s+\[[^\]]*?loss=([0-9.]+),", r.stdout)}
    return r, ev, logged


def _check_events(ev, logged, weight):
    for e in ev:
        att, focus = e["loss_attention"], e["attention_focus"]
        assert np.isfinite(att) and 0.0 <= att < 1.0, e
        assert np.isfinite(focus) and 0.0 < focus <= 1.0, e
        # the loss of the summary and of the step's log line is the total: the reference's two terms plus the weighted one
        assert abs(e["loss"] - (e["loss_mel"] + e["loss_linear"] + weight * att)) < 1e-9, e
        assert att > 0.0 and e["loss"] > e["loss_mel"] + e["loss_linear"]
        assert abs(logged[e["step"]] - e["loss"]) < 1e-5 + 1e-9, (logged, e["loss"])       # the line prints five decimals


def test_taco2_trains_with_the_guided_term(tmp_path):
    # summaries at steps 2 and 4 (synchronous steps), steps 1 and 3 through the pipelined loop
    r, ev, logged = _train(tmp_path, "taco2", SMALL + ",guided_attention_weight=1.0,guided_attention_sigma=0.2", "fp32", 4, 2)
    assert "guided_attention_weight: 1.0" in r.stdout and "guided_attention_sigma: 0.2" in r.stdout
    assert [e["step"] for e in ev] == [2, 4] and sorted(logged) == [1, 2, 3, 4]
    _check_events(ev, logged, 1.0)


def test_taco1_trains_with_the_guided_term_at_the_shipped_widths(tmp_path):
    hps = "batch_size=2,batch_group_size=2,outputs_per_step=5,max_iters=12,guided_attention_weight=1.0,guided_attention_sigma=0.2"
    r, ev, logged = _train(tmp_path, "taco1", hps, "mixed", 2, 1)
    assert "attn:bwd=cluster" in r.stdout, r.stdout[-3000:]
    assert [e["step"] for e in ev] == [1, 2]
    _check_events(ev, logged, 1.0)
