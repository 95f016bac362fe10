"""The utterance front end: what a file costs on its way to cached features, before and after ns_resample /
ns_frame_power (csrc/frontend.hip).  The parent's resampler is still in the tree as audio._resample_reference, so one
checkout measures both sides; they alternate inside every repetition.

    python profiles/tools/frontend_bench.py [--reps 20] [--files 64] [--budget-ms-per-step X]
    python profiles/tools/frontend_bench.py --profile-only      (a few kernel launches, for rocprofv3 --kernel-trace --stats)

1. `resample` alone on a 10 s clip at 16 000, 22 050 and 48 000 Hz -> 20 000 Hz, NumPy in / NumPy out as load_wav calls
   it (host clock; both sides end in the device-to-host copy of the result, which waits for the stream), plus the
   kernel by itself between device events.
2. file -> cached features per utterance through DataFeeder's first pass (cold cache) over a corpus of --files files
   (half 22 050 Hz WAV, a quarter 16 000 Hz FLAC, a quarter 48 000 Hz WAV; 3 - 8 s each): the parent's chain (host
   chain with the reference resampler), the host chain with the kernel resampler, the device chain; and the host-only
   part (file read + decode + mix-down) on its own.  Host clock, ending in a synchronise of the feeder's stream."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def speech(rng, seconds, sr):
    import bench
    return bench.synthetic_speech(rng, seconds, sr)


def stats(v):
    v = np.asarray(v) * 1e3
    return "median %8.3f ms  (min %8.3f, max %8.3f)" % (np.median(v), v.min(), v.max())


def resample_alone(reps):
    from nspeech_amd.utils import audio as A
    print("# 1. resample alone, 10 s clip -> 20 000 Hz, %d repetitions after 2 warm-up, parent and change alternated" % reps)
    ok = True
    for sr in (16000, 22050, 48000):
        x = speech(np.random.default_rng(sr), 10, sr)
        xt = torch.from_numpy(x).cuda()
        ref, new, dev = [], [], []
        for r in range(reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a = A._resample_reference(x, sr, 20000)
            t1 = time.perf_counter()
            b = A.resample(x, sr, 20000)
            t2 = time.perf_counter()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            A.resample_device(xt, sr, 20000)
            e1.record()
            e1.synchronize()
            if r >= 2:
                ref.append(t1 - t0), new.append(t2 - t1), dev.append(e0.elapsed_time(e1) * 1e-3)
        assert np.array_equal(a, b)
        ratio = np.median(ref) / np.median(new)
        ok = ok and ratio >= 10.0
        taps = 2 * int(32769 // int(min(1.0, 20000.0 / sr) * 512))
        print("%6d Hz (%7d -> %7d samples, <= %3d taps)" % (sr, x.size, b.size, taps))
        print("    parent  _resample_reference on the GPU : %s" % stats(ref))
        print("    change  resample (ns_resample)          : %s   %.1fx" % (stats(new), ratio))
        print("    change  kernel alone, device events     : %s" % stats(dev))
    print("acceptance (>= 10x at each rate): %s" % ("met" if ok else "NOT met"))
    return ok


def write_corpus(root, files):
    import flac_writer as FW
    os.makedirs(os.path.join(root, "wavs"))
    rng = np.random.default_rng(0)
    lines, seconds = [], 0.0
    for i in range(files):
        kind = ("wav22", "flac16", "wav22", "wav48")[i % 4]
        sr = {"wav22": 22050, "flac16": 16000, "wav48": 48000}[kind]
        dur = float(rng.uniform(3.0, 8.0))
        body = speech(rng, dur, sr)
        x = np.concatenate([rng.normal(0, 0.002, int(0.3 * sr)), body, rng.normal(0, 0.002, int(0.3 * sr))])
        seconds += x.size / sr
        pcm = np.round(np.clip(x, -1, 1) * 32767).astype(np.int64)
        path = os.path.join(root, "wavs", "utt%03d.wav" % i)       # load_wav tells FLAC from RIFF by the magic, not the name
        if kind == "flac16":
            frames, pos = [], 0
            while pos < len(pcm):
                size = min(4096, len(pcm) - pos)
                frames.append(dict(size=size, subframes=[dict(type="fixed", order=2, porder=3 if size == 4096 else 0)]))
                pos += size
            with open(path, "wb") as f:
                f.write(FW.encode(pcm[:, None], 16, sr, frames))
        else:
            with wave.open(path, "wb") as f:
                f.setnchannels(1)
                f.setsampwidth(2)
                f.setframerate(sr)
                f.writeframes(pcm.astype("<i2").tobytes())
        lines.append("utt%03d|some text|some text" % i)
    with open(os.path.join(root, "metadata.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return seconds / files


def first_pass(reps, files, budget):
    from nspeech_amd import hparams
    from nspeech_amd.datasets.datafeeder import DataFeeder
    from nspeech_amd.utils import audio as A
    hp = hparams.load("taco2")
    tmp = tempfile.mkdtemp(prefix="nspeech_frontend_")
    try:
        mean_s = write_corpus(tmp, files)

        def parent_loader(path):          # load_wav as it was: the torch resampler on the GPU, result back on the host
            x, sr = A._load_native(path)
            return A._resample_reference(x, sr, hp.sample_rate) if sr != hp.sample_rate else x

        chains = (("parent  host chain, reference resampler", dict(loader=parent_loader)),
                  ("change  host chain, ns_resample", dict(loader=A.load_wav)),
                  ("change  device chain", dict()))
        times = {name: [] for name, _ in chains}
        decode = []
        kept = {}
        for r in range(reps + 1):
            for name, kw in chains:
                fd = DataFeeder(hp, ljspeech=tmp, prefetch=False, device_cache=True, **kw)
                assert fd.front_end == ("device" if not kw else "host")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(files):
                    fd._get_next_example()
                fd._feeder_stream().synchronize()
                dt = (time.perf_counter() - t0) / files
                if r >= 1:
                    times[name].append(dt)
                kept[name] = fd.cache
            t0 = time.perf_counter()
            for path in sorted(kept[chains[0][0]]):
                A._load_native(path)
            if r >= 1:
                decode.append((time.perf_counter() - t0) / files)
        base = kept[chains[0][0]]
        for name, _ in chains[1:]:
            for path, (mel, lin) in kept[name].items():
                assert torch.equal(mel, base[path][0]) and torch.equal(lin, base[path][1]), (name, path)
        print("# 2. file -> cached features per utterance, DataFeeder(device_cache=True) first pass over %d files "
              "(mean %.1f s of audio), %d repetitions after 1 warm-up, chains alternated; every chain caches the same bits" % (files, mean_s, reps))
        for name, _ in chains:
            print("    %-42s: %s" % (name, stats(times[name])))
        print("    %-42s: %s" % ("host only: file read + decode + mix-down", stats(decode)))
        d = np.median(times[chains[2][0]]) * 1e3
        h = np.median(decode) * 1e3
        print("    split of the device chain: %.3f ms host decode + %.3f ms upload, kernels and the trim read-back" % (h, d - h))
        if budget:
            print("    budget: bench.py ms_per_step %.3f / 32 utterances = %.3f ms per utterance" % (budget, budget / 32.0))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def profile_only():
    from nspeech_amd.datasets import process as P
    from nspeech_amd.utils import audio as A
    for sr in (16000, 22050, 48000):
        xt = torch.from_numpy(speech(np.random.default_rng(sr), 10, sr)).cuda()
        for _ in range(5):
            y = A.resample_device(xt, sr, 20000)
        P.frame_power_device(y, 1024, 512)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--budget-ms-per-step", type=float, default=0.0)
    ap.add_argument("--bench-json", default=None, help="file holding bench.py's JSON line: its ms_per_step is the budget")
    ap.add_argument("--profile-only", action="store_true")
    a = ap.parse_args()
    if a.profile_only:
        return profile_only()
    budget = a.budget_ms_per_step
    if a.bench_json:
        for line in open(a.bench_json):
            if line.startswith("{"):
                budget = float(json.loads(line)["ms_per_step"])
    print("device: %s" % torch.cuda.get_device_name(0))
    ok = resample_alone(a.reps)
    first_pass(a.reps, a.files, budget)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
