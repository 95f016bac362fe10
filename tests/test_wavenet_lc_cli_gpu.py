"""train_wavenet.py --hparams lc_channels=80 on a corpus the test writes itself - every piece conditioned on its own
waveform's mel at frame rate - then generate_wavenet.py from the checkpoint on the mel spectrogram of one corpus wav."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _corpus(tmp, n=12):
    os.makedirs(os.path.join(tmp, "wavs"))
    rng = np.random.default_rng(0)
    lines = []
    for i in range(n):
        L = int(20000 * rng.uniform(0.15, 0.3))
        t = np.arange(L) / 20000.0
        y = 0.5 * np.sin(2 * np.pi * rng.uniform(120, 400) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 5 * t)) + rng.normal(0, 0.01, L)
        with wave.open(os.path.join(tmp, "wavs", "utt%d.wav" % i), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(20000)
            f.writeframes((np.clip(y, -1, 1) * 32767).astype("<i2").tobytes())
        lines.append("utt%d|text %d|text %d" % (i, i, i))
    with open(os.path.join(tmp, "metadata.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")


def test_mel_conditioned_wavenet_train_then_generate(dev, tmp_path):
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.utils import audio
    data = str(tmp_path / "lj")
    os.makedirs(data)
    _corpus(data)
    logs = str(tmp_path / "logs")
    small = "dilations_length=4,dilations_depth=2,skip_channels=64,sample_size=400,batch_size=4,queue_size=16"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_wavenet.py"), "--ljspeech", data, "--log-dir", logs,
                        "--hparams", small + ",lc_channels=80,use_biases=true", "--max-steps", "3", "--checkpoint-interval", "3"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    ckpt = os.path.join(logs, "wavenet", "model.ckpt-3")
    assert os.path.exists(ckpt) and "Step 3 " in r.stdout
    hp = hparams_mod.load("wavenet")
    hop = int(hp.frame_shift_ms / 1000 * hp.sample_rate)
    mel = audio.melspectrogram(audio.load_wav(os.path.join(data, "wavs", "utt0.wav"))).T
    assert mel.shape[1] == 80 and mel.shape[0] * hop >= 300
    cond, out = str(tmp_path / "mel.npy"), str(tmp_path / "gen.wav")
    np.save(cond, mel.astype(np.float32))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate_wavenet.py"), ckpt, "--samples", "300", "--hparams",
                        small + ",use_biases=true", "--lc_channels", "80", "--local_condition", cond, "--lc_hold", str(hop),
                        "--wav_out_path", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with wave.open(out, "rb") as f:
        assert f.getnframes() >= 300
    # any other local condition is still refused by name, as is simple_wavenet
    for extra in (["--hparams", small + ",lc_channels=4"], ["--hparams", small + ",lc_channels=80", "--model", "simple_wavenet"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "train_wavenet.py"), "--ljspeech", data, "--log-dir", logs,
                            "--max-steps", "1"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "lc_channels" in (r.stdout + r.stderr)
