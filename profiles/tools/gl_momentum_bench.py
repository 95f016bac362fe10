"""Griffin-Lim with and without the momentum update, timed side by side in ONE process: the 797-frame clip (10 s) and the
batch of 32 that bench.py's griffin_lim leg times, at (momentum, iterations) = (0, 60), (0.99, 60), (0.99, 30).

Every shape and setting is warmed, the settings alternate inside each round, and a timing is a host clock around
CALLS calls that end in a device synchronise (a window of a few tenths of a second).  Printed per setting: minimum /
median / maximum ms per call over the rounds - the spread of (0, 60) is the yardstick for any difference claimed - and
the spectral convergence SC = || g |STFT(y)| - S || / || S || (least-squares gain g, float64 on the host) of the three
single-clip results, against the magnitudes S the kernel itself starts from (the normalised spectrogram through the
shipped `power`: inconsistent, both updates stall at one floor) and, as a second input, against consistent raw
magnitudes |STFT(y)| of the same signal (raw_magnitude=True).  One JSON line at the end.

  python3 profiles/tools/gl_momentum_bench.py [--rounds 7]
  rocprofv3 --kernel-trace --stats -d <dir> -- python3 profiles/tools/gl_momentum_bench.py --rounds 2   (a run of its own)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from nspeech_amd import hparams as hparams_mod  # noqa: E402
from nspeech_amd.utils import audio as A  # noqa: E402
from oracle import audio_oracle as AO  # noqa: E402

SETTINGS = [(0.0, 60), (0.99, 60), (0.99, 30)]
CALLS = {"clip": 400, "batch_32": 40}


def signal_and_spectrogram(hp):
    """bench.py's griffin_lim leg, restated: the seeded speech-like 10 s signal and its 797 normalised frames."""
    rng = np.random.default_rng(1234)
    L = 200000
    t = np.arange(L) / hp.sample_rate
    f0 = rng.uniform(90, 250)
    y = sum(np.sin(2 * np.pi * f0 * (h + 1) * t) / (h + 1) for h in range(5)) * (0.5 + 0.5 * np.sin(2 * np.pi * 4 * t))
    y = (0.8 * y / np.abs(y).max() + rng.normal(0, 0.01, L)).astype(np.float32)
    return y, AO.spectrogram(y, dict(hp.values(), min_level_db=-100)).T[:797].copy()


def spectral_convergence(y, S):
    m = np.abs(AO.tf_stft(np.asarray(y, np.float64), 2048, 250, 1000))
    g = (m * S).sum() / (m * m).sum()
    return float(np.linalg.norm(g * m - S) / np.linalg.norm(S))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    hp = hparams_mod.load("taco2")
    assert A._stft_parameters() == (2048, 250, 1000)
    y, spec = signal_and_spectrogram(hp)
    inputs = {"clip": torch.tensor(spec, device="cuda")}
    inputs["batch_32"] = inputs["clip"].unsqueeze(0).repeat(32, 1, 1).contiguous()
    for st in inputs.values():                                     # warm every shape at every setting
        for a, it in SETTINGS:
            A.griffin_lim_gpu(st, iters=it, momentum=a)
    torch.cuda.synchronize()
    ms = {(k, s): [] for k in inputs for s in SETTINGS}
    for _ in range(args.rounds):
        for k, st in inputs.items():
            for a, it in SETTINGS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(CALLS[k]):
                    A.griffin_lim_gpu(st, iters=it, momentum=a)
                torch.cuda.synchronize()
                ms[(k, (a, it))].append((time.perf_counter() - t0) * 1e3 / CALLS[k])
    res = {"rounds": args.rounds, "calls_per_window": CALLS, "ms_min_median_max": {}, "sc_shipped_power": {}, "sc_consistent": {}}
    for (k, (a, it)), v in ms.items():
        v = sorted(v)
        res["ms_min_median_max"]["%s momentum %g iters %d" % (k, a, it)] = [round(v[0], 4), round(v[len(v) // 2], 4), round(v[-1], 4)]
        print("%-9s momentum %-4g iters %2d: %8.4f / %8.4f / %8.4f ms per call (min / median / max of %d windows of %d calls)"
              % (k, a, it, v[0], v[len(v) // 2], v[-1], len(v), CALLS[k]))
    # what the iterations are for: |STFT(result)| against the magnitudes they were given
    x = np.clip(spec.astype(np.float64), 0, 1)
    S_shipped = np.power(np.power(10.0, (x * -hp.min_level_db + hp.min_level_db + hp.ref_level_db) * 0.05), hp.power)
    S_cons = np.abs(AO.tf_stft(y[:796 * 250 + 1000], 2048, 250, 1000)).astype(np.float32)
    for a, it in SETTINGS:
        key = "momentum %g iters %d" % (a, it)
        res["sc_shipped_power"][key] = spectral_convergence(A.griffin_lim_gpu(inputs["clip"], iters=it, momentum=a).cpu().numpy(), S_shipped)
        res["sc_consistent"][key] = spectral_convergence(
            A.griffin_lim_gpu(S_cons, iters=it, raw_magnitude=True, momentum=a).cpu().numpy(), S_cons.astype(np.float64))
        print("SC %-22s: %.4f on the spectrogram through power %.1f, %.4f on consistent raw magnitudes"
              % (key, res["sc_shipped_power"][key], hp.power, res["sc_consistent"][key]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
