"""train.py --hparams stop_token=true on the tiny synthetic corpus of tests/test_cli_gpu.py (built the same way):
events.jsonl carries loss_stop and stop_step_error, the logged loss is the total, a checkpoint is written with the stop
variables in it, and eval.py synthesises from it with the same switch."""
import glob
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
STOP_HP = ",stop_token=true,stop_token_weight=2.0,stop_token_pos_weight=3.0,stop_threshold=0.4"


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


def test_train_then_eval_with_the_stop_token(tmp_path):
    import torch
    data = str(tmp_path / "lj")
    os.makedirs(data)
    _corpus(data)
    logs = str(tmp_path / "logs")
    # summaries at steps 2 and 4 (synchronous steps), steps 1 and 3 through the pipelined loop; a checkpoint at step 4
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--ljspeech", data, "--model", "taco2", "--log_dir", logs,
                        "--hparams", SMALL + STOP_HP, "--checkpoint_interval", "4", "--precision", "fp32",
                        "--summary-interval", "2", "--max_steps", "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "stop_token: True" in r.stdout and "stop_threshold: 0.4" in r.stdout
    out_dir = os.path.join(logs, "logs-taco2")
    ev = [json.loads(l) for l in open(os.path.join(out_dir, "events.jsonl"))]
    logged = {int(m.group(1)): float(m.group(2)) for m in re.finditer(r"Step (\d+)\s+\[[^\]]*?loss=([0-9.]+),", r.stdout)}
    assert [e["step"] for e in ev] == [2, 4] and sorted(logged) == [1, 2, 3, 4]
    for e in ev:
        ls, err = e["loss_stop"], e["stop_step_error"]
        assert np.isfinite(ls) and ls > 0.0 and np.isfinite(err) and err >= 0.0, e
        assert abs(e["loss"] - (e["loss_mel"] + e["loss_linear"] + 2.0 * ls)) < 1e-9, e
        assert abs(logged[e["step"]] - e["loss"]) < 1e-5 + 1e-9, (logged, e["loss"])       # the line prints five decimals
        assert "decoder/stop_projection/kernel" in e["gradient_norm"]
    ckpt = os.path.join(out_dir, "model.ckpt-4")
    assert os.path.exists(ckpt), os.listdir(out_dir)
    sd = torch.load(ckpt, map_location="cpu", weights_only=True)
    assert tuple(sd["model/inference/decoder/stop_projection/kernel"].shape) == (64, 1)
    assert tuple(sd["model/inference/decoder/stop_projection/bias"].shape) == (1,)
    # eval.py needs no flag of its own: the hparams carry the switch and the threshold
    r = subprocess.run([sys.executable, os.path.join(ROOT, "eval.py"), "--checkpoint", ckpt, "--model", "taco2",
                        "--hparams", SMALL + STOP_HP + ",max_iters=12", "--precision", "fp32"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    wavs = sorted(glob.glob(os.path.join(out_dir, "eval-4-*.wav")))
    assert len(wavs) == 6
    with wave.open(wavs[0], "rb") as f:
        assert f.getframerate() == 20000 and f.getnframes() > 0


def test_taco1_refuses_the_switch_on_the_command_line(tmp_path):
    data = str(tmp_path / "lj")
    os.makedirs(data)
    _corpus(data)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--ljspeech", data, "--model", "taco1", "--log_dir",
                        str(tmp_path / "logs"), "--hparams", "batch_size=2,batch_group_size=2,stop_token=true",
                        "--max_steps", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert "only the Tacotron-2 model" in r.stdout + r.stderr
