"""What a condition costs the WaveNet generator: us per drawn sample at the shipped wavenet.yaml widths (50 layers,
R = Dc = 32, S = 512, Q = 256), batch 1, 2000 drawn samples behind a receptive-field seed, bf16 weights.

    python profiles/tools/wavenet_cond_bench.py [--samples 2000] [--reps 3]

  (i)   simple_wavenet on the MFMA chain (engine 2)
  (ii)  gc_channels=32, use_biases=true on the per-layer kernel (fast=False) - where such a model ran before the chain
        took conditions
  (iii) the same model on the MFMA chain's conditioned instantiation
  (iv)  (iii) + lc_channels=80 at hold=250: one mel row per hop of audio.yaml

One warm-up call per variant, then the variants alternate --reps times inside this process.  A call is timed between
device events; the seed walk (rf steps without a draw) is timed by a one-draw call of its own in the same repetition and
subtracted, as bench.py does.  Acceptance: (iii) and (iv) faster than (ii) by more than the spread between repeats."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.models import create_model
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    n = a.samples

    def model(kind, **over):
        hp = hparams_mod.load("wavenet")
        for k, v in over.items():
            setattr(hp, k, v)
        return create_model(kind, hp, device="cuda:0", dtype="bf16", seed=1234)
    spk = dict(gc_channels=32, gc_category_cardinality=109, use_biases=True)
    simple, cond, local = model("simple_wavenet"), model("wavenet", **spk), model("wavenet", lc_channels=80, **spk)
    for m in (cond, local):                  # biases start at zero: give them values (the kernels do not look, the reader might)
        p = m.numpy_params()
        rng = np.random.RandomState(1)
        for k in p:
            if k.endswith("_bias"):
                p[k] = (rng.randn(*p[k].shape) * 0.1).astype(np.float32)
        m.load_numpy_params(p)
    rf = simple.rf
    rng = np.random.default_rng(0)
    seed = rng.integers(0, 256, size=(1, rf)).astype(np.int32)
    hold = 250
    mel = rng.standard_normal((1, (n - 1) // hold + 1, 80)).astype(np.float32)
    gc = np.array([7])
    variants = [
        ("(i)   simple_wavenet, engine 2", simple, dict(engine=2), 2),
        ("(ii)  gc 32 + biases, per-layer kernel", cond, dict(fast=False, global_conditions=gc), 0),
        ("(iii) gc 32 + biases, engine 2", cond, dict(global_conditions=gc), 2),
        ("(iv)  (iii) + lc 80, hold 250, engine 2", local, dict(global_conditions=gc, local_conditions=mel, hold=hold, t0=-rf), 2),
    ]

    def timed(m, k, kw):
        un = rng.random((1, k))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m.generate(seed, k, uniforms=un, **kw)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    for name, m, kw, eng in variants:        # warm-up
        timed(m, 64, kw)
        assert m.last_engine == eng, (name, m.last_engine)
    us = {name: [] for name, _, _, _ in variants}
    walk = {name: [] for name, _, _, _ in variants}
    for _ in range(a.reps):
        for name, m, kw, _ in variants:
            full, one = timed(m, n, kw), timed(m, 1, kw)
            us[name].append((full - one) / (n - 1) * 1e6)
            walk[name].append(one * 1e3)
    print("device: %s; %d drawn samples behind a seed of %d, batch 1, %d repetitions, variants alternated" %
          (torch.cuda.get_device_name(0), n, rf, a.reps))
    print("%-44s %12s %10s %10s %14s" % ("variant", "us / sample", "min", "max", "seed walk ms"))
    med = {}
    for name, _, _, _ in variants:
        v = np.asarray(us[name])
        med[name] = float(np.median(v))
        print("%-44s %12.2f %10.2f %10.2f %14.1f" % (name, med[name], v.min(), v.max(), np.median(walk[name])))
    spread = max(float(np.max(v) - np.min(v)) for v in us.values())
    k = [name for name, _, _, _ in variants]
    print("largest spread between repeats of one variant: %.2f us" % spread)
    print("(iii) against (i): %+.2f us per drawn sample (what the condition terms cost the chain)" % (med[k[2]] - med[k[0]]))
    print("(iv) against (iii): %+.2f us" % (med[k[3]] - med[k[2]]))
    ok = all(med[k[1]] - med[x] > spread for x in (k[2], k[3]))
    print("(ii) / (iii) = %.1fx, (ii) / (iv) = %.1fx; acceptance ((iii), (iv) faster than (ii) by more than the spread): %s" %
          (med[k[1]] / med[k[2]], med[k[1]] / med[k[3]], "met" if ok else "NOT met"))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
