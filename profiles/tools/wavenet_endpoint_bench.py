"""The WaveNet generator's own end point (ns_wavenet_generate_until, generate(endpoint=)): what the armed rule costs a drawn
sample, and what stopping at the end point buys a synthesize() call.

  --what cost   us per drawn sample at the shipped wavenet.yaml widths (50 layers, R = Dc = 32, S = 512, Q = 256), bf16
                weights, 2000 drawn samples behind a receptive-field seed, engine 2 without conditions and with them
                (use_biases + lc_channels=80 at hold=250), batch 1 and 32, as
                    parent | parent again | stop = NULL | armed, below = 0
                "parent" is the library of the commit before the entry point, loaded beside this one in the same process
                (ns_wavenet_generate_params is unchanged, so it reads the same block); the second parent column is the
                same library once more - the distance between the two is what a repeat of the SAME code moves by.
                "armed, below = 0" is generate(endpoint=(16000, 4000, -2.0)): the rule runs on every drawn sample and
                never fires.  One warm-up call per mode, then the modes alternate --reps times, rotating which goes
                first; a call is timed between device events, the seed walk by a one-draw call of its own in the same
                repetition and subtracted, as bench.py does.  Accepted when the medians of the last two columns lie
                within the parent's spread (the range of all its timings, both columns) of the parent's median.

                    git worktree add ../parent HEAD~1 && bash ../parent/nspeech_amd/csrc/build.sh
                    python profiles/tools/wavenet_endpoint_bench.py --what cost --parent-lib ../parent/nspeech_amd/csrc/libnspeech_hip.so

  --what buys   Synthesizer.synthesize(text, vocoder="wavenet") at the shipped Tacotron-2 and WaveNet widths, max_iters =
                300 (1500 frames, 375000 samples), initial weights, the vocoder's postprocess2 bias raised at the code of
                zero amplitude and temperature = 0: every sample is silent, the end point is at 8000 and the rule stops
                the draw at 20000 samples.  stop_at_endpoint False against True, one warm-up and three timed calls each:
                seconds per call (host clock around the call) and samples drawn.  This is the best case by construction -
                a real utterance saves its own silent tail (the samples behind end - hop + window), not this ratio.

The register and scratch report of the kernels: profiles/tools/wavenet_temperature_bench.py --resources DIR."""
import argparse
import contextlib
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

NEVER = (16000, 4000, -2.0)          # endpoint_code(Q, -2.0) == 0: no code is silent
MODES = [("parent", True, {}), ("parent again", True, {}), ("stop = NULL", False, {}), ("armed, below = 0", False, dict(endpoint=NEVER))]


def cost(a):
    import torch
    from nspeech_amd import _lib
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.models import create_model
    n = a.samples
    this = _lib.lib()
    parent = None
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        parent.ns_last_error.restype = ctypes.c_char_p
        assert parent.ns_version() < this.ns_version(), "--parent-lib is not older than this library"

    @contextlib.contextmanager
    def library(handle):
        _lib._lib = handle
        try:
            yield
        finally:
            _lib._lib = this

    def model(kind, **over):
        hp = hparams_mod.load("wavenet")
        for k, v in over.items():
            setattr(hp, k, v)
        return create_model(kind, hp, device="cuda:0", dtype="bf16", seed=1234)
    simple, local = model("simple_wavenet"), model("wavenet", use_biases=True, lc_channels=80)
    p = local.numpy_params()
    rs = np.random.RandomState(1)
    for k in p:                              # biases start at zero: give them values
        if k.endswith("_bias"):
            p[k] = (rs.randn(*p[k].shape) * 0.1).astype(np.float32)
    local.load_numpy_params(p)
    rf, hold = simple.rf, 250
    rng = np.random.default_rng(0)
    rows = []
    for B in (1, 32):
        seed = rng.integers(0, 256, size=(B, rf)).astype(np.int32)
        mel = rng.standard_normal((B, (n - 1) // hold + 1, 80)).astype(np.float32)
        rows += [("engine 2, batch %d" % B, simple, seed, dict(engine=2)),
                 ("engine 2 conditioned, batch %d" % B, local, seed, dict(local_conditions=mel, hold=hold, t0=-rf))]
    modes = [m for m in MODES if parent is not None or not m[1]]

    def timed(m, seed, k, kw, old):
        un = rng.random((len(seed), k))
        with library(parent if old else this):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            m.generate(seed, k, uniforms=un, **kw)
            e1.record()
            e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def same_bits(m, seed, kw):
        """64 draws at the same uniforms on the parent's library, on this one, and on this one armed: ids and last_probs."""
        un, out = rng.random((len(seed), 64)), []
        for handle, more in ((parent, {}), (this, {}), (this, dict(endpoint=NEVER))):
            with library(handle):
                ids = m.generate(seed, 64, uniforms=un, **dict(kw, **more))
                out.append((ids.clone(), m.last_probs.clone()))
        return all(torch.equal(out[0][0], o[0]) and torch.equal(out[0][1], o[1]) for o in out[1:])

    print("device: %s; %d drawn samples behind a seed of %d, %d repetitions, the modes of a row alternated" %
          (torch.cuda.get_device_name(0), n, rf, a.reps))
    print("us per drawn sample: median [min .. max]")
    print("%-32s" % "variant" + "".join("%26s" % name for name, _, _ in modes))
    worst, identical = 0.0, True
    for name, m, seed, kw in rows:
        for _, old, more in modes:           # warm-up
            timed(m, seed, 64, dict(kw, **more), old)
            assert m.last_engine == 2, (name, m.last_engine)
        if parent is not None:
            identical = same_bits(m, seed, kw) and identical
        us = {mode: [] for mode, _, _ in modes}
        for r in range(a.reps):
            for mode, old, more in modes[r % len(modes):] + modes[:r % len(modes)]:      # every mode takes every place in turn
                k = dict(kw, **more)
                full, one = timed(m, seed, n, k, old), timed(m, seed, 1, k, old)
                us[mode].append((full - one) / (n - 1) * 1e6)
        v = {mode: np.asarray(x) for mode, x in us.items()}
        print("%-32s" % name + "".join("%10.2f [%5.2f ..%6.2f]" % (np.median(v[mode]), v[mode].min(), v[mode].max()) for mode, _, _ in modes))
        if parent is not None:
            base = np.concatenate([v["parent"], v["parent again"]])
            spread, mid = float(base.max() - base.min()), float(np.median(base))
            print("    parent: median of both columns %.2f us, spread (range of all its timings) %.2f us, column against column %+.2f us"
                  % (mid, spread, float(np.median(v["parent again"]) - np.median(v["parent"]))))
        else:
            base = v["stop = NULL"]
            spread, mid = float(base.max() - base.min()), float(np.median(base))
        for mode in ("stop = NULL", "armed, below = 0"):
            if parent is None and mode == "stop = NULL":
                continue
            over = float(np.median(v[mode])) - mid
            print("    %-18s %+6.2f us against %s%s" % (mode, over, "the parent" if parent is not None else "stop = NULL",
                                                       "" if over <= spread else "   <-- more than the spread (%.2f us)" % spread))
            worst = max(worst, over - spread)
    if parent is not None:
        print("64 draws and last_probs, parent against this library with stop = NULL and armed at below = 0, every row: %s"
              % ("bit-identical" if identical else "DIFFERENT"))
    print("expectation (stop = NULL and the armed rule within the parent's spread): %s" % ("met" if worst <= 0 else "NOT met, see the flags"))


def buys(a):
    import torch
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.models.wavenet import mu_law_encode
    from nspeech_amd.synthesizer import Synthesizer
    from nspeech_amd.utils import audio
    whp = hparams_mod.load("wavenet")
    whp.use_biases, whp.lc_channels = True, 80
    hp = hparams_mod.load("taco2")
    hp.max_iters = 300
    hparams_mod.set_hparams(hp)
    synth = Synthesizer(hp).load(None, "taco2")
    synth.load_vocoder(None, whp)
    v = synth.vocoder
    p = v.numpy_params()
    bias = p["wavenet/postprocessing/postprocess2_bias"].copy()
    bias[int(mu_law_encode(np.zeros(1, np.float32), v.Q)[0])] = 30.0
    p["wavenet/postprocessing/postprocess2_bias"] = bias
    v.load_numpy_params(p)
    total = hp.max_iters * hp.outputs_per_step * synth._vocoder_hop
    print("device: %s; synthesize(vocoder='wavenet', temperature=0), %d frames = %d samples, a vocoder that draws silence only"
          % (torch.cuda.get_device_name(0), hp.max_iters * hp.outputs_per_step, total))
    print("%-24s %28s %14s %14s %10s" % ("stop_at_endpoint", "seconds per call (%d calls)" % a.calls, "samples drawn", "samples kept", "engine"))
    out = {}
    for flag in (False, True):
        secs = []
        for i in range(1 + a.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            wav = synth.synthesize("Hello, World.", vocoder="wavenet", temperature=0, stop_at_endpoint=flag)[0]
            secs.append(time.perf_counter() - t0)
        end = int(v.last_ends[0].item())
        window, hop, _ = audio.endpoint_rule()
        drawn = end - hop + window if end < total else total
        out[flag] = (wav, np.median(secs[1:]))
        print("%-24s %28s %14d %14d %10d" % (flag, "  ".join("%.3f" % s for s in secs[1:]), drawn, len(wav), v.last_engine))
    same = np.array_equal(out[False][0], out[True][0])
    print("the two waveforms: %s; median %.3f s against %.3f s per call" % ("bit-identical" if same else "DIFFERENT", out[False][1], out[True][1]))
    print("(the best case by construction: a real utterance saves its own silent tail - the samples behind end - hop + window - "
          "not this ratio)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["cost", "buys", "both"], default="both")
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if a.what in ("cost", "both"):
        cost(a)
    if a.what in ("buys", "both"):
        buys(a)


if __name__ == "__main__":
    main()
