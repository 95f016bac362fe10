"""What a mel local condition costs the WaveNet training step: ms per step at the shipped wavenet.yaml widths (50 layers,
R = Dc = 32, S = 512, Q = 256), bf16, 8 clips of 13 117 samples (bench.py's step), lc_channels = 80, one mel row per 250
samples (53 rows per clip).

    python profiles/tools/wavenet_lc_train_bench.py [--steps 5] [--reps 3]

  (i)   the unconditioned step (--model wavenet with every option off = simple_wavenet)
  (ii)  lc_channels=80 in the per-sample form, [N, T - 1, 80]: the mel repeated on the host inside the timed step, as a
        caller who holds a mel has to do for that form
  (iii) lc_channels=80 in the held form, step(audio, None, mel, hold=250): the condition's 1x1 convolutions at frame rate,
        its term added inside the gate kernel, its weight gradient from ns_wavenet_hold_sum

Two warm-up steps per variant, then the variants alternate --reps times inside this process; a repetition is --steps
steps between two device synchronisations, host work included.  Acceptance: (iii) faster than (ii) by more than the
largest spread between repeats of one variant."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.models import create_model
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()

    def model(**over):
        hp = hparams_mod.load("wavenet")
        for k, v in over.items():
            setattr(hp, k, v)
        m = create_model("wavenet", hp, device="cuda:0", dtype="bf16", seed=1234)
        m.add_optimizer(0)
        return m
    plain, per_sample, held = model(), model(lc_channels=80), model(lc_channels=80)
    rf = plain.rf
    rng = np.random.default_rng(1234)
    N, T, hold = 8, rf + 8000, 250
    t = np.arange(T) / 16000.0
    audio = (0.5 * np.sin(2 * np.pi * 220 * t)[None] + 0.02 * rng.standard_normal((N, T))).astype(np.float32)
    T0 = T - 1
    mel = rng.standard_normal((N, (T0 - 1) // hold + 1, 80)).astype(np.float32)
    variants = [
        ("(i)   unconditioned", lambda: plain.step(audio)),
        ("(ii)  lc 80, per sample (host repeat)", lambda: per_sample.step(audio, None, np.repeat(mel, hold, axis=1)[:, :T0])),
        ("(iii) lc 80, held, hold 250", lambda: held.step(audio, None, mel, hold=hold)),
    ]
    loss = {}
    for name, fn in variants:                # warm-up (buffers, first launches)
        for _ in range(2):
            loss[name] = fn()
    ms = {name: [] for name, _ in variants}
    for _ in range(a.reps):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    print("device: %s; %d clips of %d samples (receptive field %d), %d mel rows of %d channels per clip, bf16; %d repetitions of "
          "%d steps, variants alternated" % (torch.cuda.get_device_name(0), N, T, rf, mel.shape[1], mel.shape[2], a.reps, a.steps))
    print("%-42s %12s %10s %10s %10s %12s" % ("variant", "ms / step", "min", "max", "spread", "first loss"))
    med = {}
    for name, _ in variants:
        v = np.asarray(ms[name])
        med[name] = float(np.median(v))
        print("%-42s %12.3f %10.3f %10.3f %10.3f %12.4f" % (name, med[name], v.min(), v.max(), v.max() - v.min(), loss[name]))
    spread = max(float(np.max(v) - np.min(v)) for v in ms.values())
    k = [name for name, _ in variants]
    print("largest spread between repeats of one variant: %.3f ms" % spread)
    print("(iii) - (i): %+.3f ms per step (what the held condition costs)" % (med[k[2]] - med[k[0]]))
    print("(ii) - (i): %+.3f ms per step (what the per-sample form costs)" % (med[k[1]] - med[k[0]]))
    ok = med[k[1]] - med[k[2]] > spread
    print("(ii) / (iii) = %.2fx; acceptance ((iii) faster than (ii) by more than the spread): %s"
          % (med[k[1]] / med[k[2]], "met" if ok else "NOT met"))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
