"""Batched synthesis against the loop it replaces, and the finishing stage on its own (ns_wave_finish, csrc/audio.hip).

    python profiles/tools/synth_batch_bench.py [--pairs 8] [--reps 10]

1. Text -> waveforms for eval.py's six sentences: Tacotron-2 at the shipped widths, `mixed`, no checkpoint, Griffin-Lim.
   (a) the parent's form, a loop of Synthesizer.synthesize; (b) one Synthesizer.synthesize_batch.  Host clock around
   work that ends in the device-to-host copies of the results (they wait for the stream) and a synchronise.  Both forms
   are warmed up first - the six sentences have six lengths, so every call of (a) meets a new signature and runs
   eagerly, as it does in eval.py - then --pairs alternated pairs in one process.
2. The finishing stage alone for 32 clips of 10 s that lie on the device, results wanted on the host: (a) 32 x
   (copy to the host, audio.inv_preemphasis, audio.find_endpoint) as synthesize does it, (b) one audio.finish_waves and
   the copies of y and ends; and the launch of (b) by itself between device events."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def line(name, v):
    v = np.asarray(v) * 1e3
    return "    %-58s: median %9.3f ms  (min %9.3f, max %9.3f, spread %5.1f %%)" % (
        name, np.median(v), v.min(), v.max(), 100.0 * (v.max() - v.min()) / np.median(v))


def sentences(pairs):
    import eval as eval_cli
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.synthesizer import Synthesizer
    hp = hparams_mod.load("taco2")
    synth = Synthesizer(hp, dtype="mixed").load(None, "taco2")
    texts = list(eval_cli.TEST_SENTENCES)

    def loop():
        return [synth.synthesize(t) for t in texts]

    def batch():
        return synth.synthesize_batch(texts)

    paths = {}
    for _ in range(2):
        a = loop()
        paths["a"] = synth.model.last_paths.get("decode")
        b = batch()
        paths["b"] = synth.model.last_paths.get("decode")
    print("# 1. six sentences -> (wav, mel, lin), %d alternated pairs after 2 warm-up rounds of each form" % pairs)
    print("    decode path: (a) %s, (b) %s; frames per sentence %d; samples kept (a) %s (b) %s"
          % (paths["a"], paths["b"], a[0][1].shape[0], [len(w) for w, _, _ in a], [len(w) for w, _, _ in b]))
    ta, tb = [], []
    for r in range(pairs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        batch()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ta.append(t1 - t0), tb.append(t2 - t1)
        print("    pair %2d: (a) loop of synthesize %9.3f ms   (b) synthesize_batch %9.3f ms   a / b = %.2f"
              % (r, ta[-1] * 1e3, tb[-1] * 1e3, ta[-1] / tb[-1]))
    print(line("(a) loop of six synthesize calls", ta))
    print(line("(b) one synthesize_batch call", tb))
    print("    ratio of the medians a / b = %.2f" % (np.median(ta) / np.median(tb)))


def finishing(reps):
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.utils import audio as A
    hp = hparams_mod.load("taco2")
    N, L = 32, 10 * hp.sample_rate
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((N, L)) * 0.05).astype(np.float32)
    for i in range(N):                           # 5 .. 9 s of signal, silence behind it
        x[i, int((5 + 4 * i / (N - 1)) * hp.sample_rate):] = 0
    xd = torch.from_numpy(x).cuda()

    def parent():
        out = []
        for i in range(N):
            w = A.inv_preemphasis(xd[i].cpu().numpy())
            out.append(w[:A.find_endpoint(w)])
        return out

    def change():
        y, ends = A.finish_waves(xd)
        y, ends = y.cpu().numpy(), ends.cpu().numpy()
        return [y[i, :ends[i]] for i in range(N)]

    for _ in range(2):
        a, b = parent(), change()
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    print("# 2. finishing stage alone, %d clips of %d samples on the device -> cut clips on the host, %d alternated pairs "
          "after 2 warm-up; both forms return the same bits; ends %d .. %d" % (N, L, reps, min(map(len, b)), max(map(len, b))))
    ta, tb, tk = [], [], []
    for r in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        parent()
        t1 = time.perf_counter()
        change()
        t2 = time.perf_counter()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        A.finish_waves(xd)
        e1.record()
        e1.synchronize()
        ta.append(t1 - t0), tb.append(t2 - t1), tk.append(e0.elapsed_time(e1) * 1e-3)
        print("    pair %2d: (a) %9.3f ms   (b) %9.3f ms   a / b = %.1f   launch alone %.3f ms"
              % (r, ta[-1] * 1e3, tb[-1] * 1e3, ta[-1] / tb[-1], tk[-1] * 1e3))
    print(line("(a) 32 x (copy, inv_preemphasis, find_endpoint)", ta))
    print(line("(b) one finish_waves + the copies of y and ends", tb))
    print(line("(b) finish_waves alone, device events (with its allocations)", tk))
    print("    ratio of the medians a / b = %.1f" % (np.median(ta) / np.median(tb)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    assert a.pairs >= 6, "at least six alternated pairs"
    print("device: %s" % torch.cuda.get_device_name(0))
    finishing(a.reps)
    sentences(a.pairs)


if __name__ == "__main__":
    main()
