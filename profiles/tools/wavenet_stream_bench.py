"""The resumable WaveNet generator (ns_wavenet_generate_span, generate_stream, synthesize_stream, generate_wavenet.py
--stream_chunk): what passing a span to the kernels costs the one-call generate, what a stream of spans costs against
the one call, and how much earlier the first samples are out.  Shipped wavenet.yaml widths (50 layers, R = Dc = 32,
S = 512, Q = 256), bf16 weights, engine 2 without conditions and with them (use_biases + lc_channels=80 at hold=250),
batch 1, --samples drawn samples (40000) behind a receptive-field seed.

  --what cost    us per drawn sample of generate(), as   parent | parent again | this library.  "parent" is the library of
                 the commit before the entry point, loaded beside this one in the same process (the structs are unchanged,
                 so it reads the same blocks); the second parent column is the same library once more - the distance
                 between the two is what a repeat of the SAME code moves by.  One warm-up call per mode, then the modes
                 alternate --reps times, rotating which goes first; a call is timed between device events, the seed walk
                 by a one-draw call of its own in the same repetition and subtracted, as bench.py does.  Expected: this
                 library's median within the parent's spread (the range of all its timings) of the parent's median.

                     git worktree add ../parent HEAD~1 && bash ../parent/nspeech_amd/csrc/build.sh
                     python profiles/tools/wavenet_stream_bench.py --what cost --parent-lib ../parent/nspeech_amd/csrc/libnspeech_hip.so

  --what stream  generate() against generate_stream(chunk = --chunk, 5000), host clock from the call to the last sample on
                 the host, the two alternated --reps times: the totals, the difference per span, and the time to the first
                 chunk on the host against the time of the whole one call.
  --what cli     generate_wavenet.py --save_every CHUNK against --stream_chunk CHUNK for the same --samples, in this process
                 (main() on a checkpoint of the unconditioned model written to a temporary directory, no --wav_out_path):
                 seconds per run.  --save_every restarts the generator per chunk - zero queues and the last receptive
                 field walked again - which --stream_chunk does not.
  --what synth   Synthesizer.synthesize(text, vocoder="wavenet") against synthesize_stream(text) at the shipped Tacotron-2
                 and WaveNet widths, max_iters = 60 (300 frames, 75000 samples), initial weights (a vocoder that never
                 falls silent: every sample is drawn): seconds to the returned waveform against seconds to the first
                 piece and to the last.

The register and scratch report of the kernels: profiles/tools/wavenet_temperature_bench.py --resources DIR."""
import argparse
import contextlib
import ctypes
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

MODES = [("parent", True), ("parent again", True), ("this library", False)]


def _models():
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.models import create_model

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
    return simple, local


def _rows(a, simple, local, rng):
    rf, hold, n = simple.rf, 250, a.samples
    seed = rng.integers(0, 256, size=(1, rf)).astype(np.int32)
    mel = rng.standard_normal((1, (n - 1) // hold + 1, 80)).astype(np.float32)
    return [("engine 2", simple, seed, dict(engine=2)),
            ("engine 2 conditioned", local, seed, dict(local_conditions=mel, hold=hold, t0=-rf))]


def cost(a):
    import torch
    from nspeech_amd import _lib
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
    simple, local = _models()
    rng = np.random.default_rng(0)
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
        un, out = rng.random((len(seed), 64)), []
        for handle in (parent, this):
            with library(handle):
                ids = m.generate(seed, 64, uniforms=un, **kw)
                out.append((ids.clone(), m.last_probs.clone()))
        return torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])

    print("device: %s; batch 1, %d drawn samples behind a seed of %d, %d repetitions, the modes of a row alternated" %
          (torch.cuda.get_device_name(0), n, simple.rf, a.reps))
    print("generate(), us per drawn sample: median [min .. max]")
    print("%-24s" % "variant" + "".join("%26s" % name for name, _ in modes))
    worst, identical = 0.0, True
    for name, m, seed, kw in _rows(a, simple, local, rng):
        for _, old in modes:                 # warm-up
            timed(m, seed, 64, kw, old)
            assert m.last_engine == 2, (name, m.last_engine)
        if parent is not None:
            identical = same_bits(m, seed, kw) and identical
        us = {mode: [] for mode, _ in modes}
        for r in range(a.reps):
            for mode, old in modes[r % len(modes):] + modes[:r % len(modes)]:      # every mode takes every place in turn
                full, one = timed(m, seed, n, kw, old), timed(m, seed, 1, kw, old)
                us[mode].append((full - one) / (n - 1) * 1e6)
        v = {mode: np.asarray(x) for mode, x in us.items()}
        print("%-24s" % name + "".join("%10.2f [%5.2f ..%6.2f]" % (np.median(v[mode]), v[mode].min(), v[mode].max()) for mode, _ in modes))
        if parent is not None:
            base = np.concatenate([v["parent"], v["parent again"]])
            spread, mid = float(base.max() - base.min()), float(np.median(base))
            over = float(np.median(v["this library"])) - mid
            print("    parent: median of both columns %.2f us, spread (range of all its timings) %.2f us; this library %+.2f us%s"
                  % (mid, spread, over, "" if abs(over) <= spread else "   <-- more than the spread"))
            worst = max(worst, abs(over) - spread)
    if parent is not None:
        print("64 draws and last_probs, parent against this library at the same uniforms, every row: %s"
              % ("bit-identical" if identical else "DIFFERENT"))
        print("expectation (this library within the parent's spread): %s" % ("met" if worst <= 0 else "NOT met, see the flags"))


def stream(a):
    import torch
    simple, local = _models()
    rng = np.random.default_rng(0)
    n, chunk = a.samples, a.chunk
    spans = -(-n // chunk)
    print("device: %s; batch 1, %d drawn samples, generate() against generate_stream(chunk=%d): %d spans; host clock, %d repetitions"
          % (torch.cuda.get_device_name(0), n, chunk, spans, a.reps))
    print("%-24s %22s %22s %16s %22s" % ("variant", "one call, s", "stream, s", "us per span", "first chunk, s"))
    for name, m, seed, kw in _rows(a, simple, local, rng):
        un = rng.random((1, n))

        def one():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids = m.generate(seed, n, uniforms=un, **kw).cpu().numpy()
            return time.perf_counter() - t0, None, ids[:, m.rf:]

        def streamed():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            first, pieces = None, []
            for piece in m.generate_stream(seed, n, chunk, uniforms=un, **kw):
                first = first or time.perf_counter() - t0
                pieces.append(piece)
            return time.perf_counter() - t0, first, np.concatenate(pieces, axis=1)
        m.generate(seed, 64, uniforms=un[:, :64], **kw)
        list(m.generate_stream(seed, 64, 32, uniforms=un[:, :64], **kw))
        t = {"one": [], "stream": [], "first": []}
        same = True
        for r in range(a.reps):
            order = (one, streamed) if r % 2 == 0 else (streamed, one)
            got = {}
            for fn in order:
                secs, first, ids = fn()
                got[fn.__name__] = ids
                t["one" if fn is one else "stream"].append(secs)
                if first is not None:
                    t["first"].append(first)
            same = same and np.array_equal(got["one"], got["streamed"])
        med = {k: float(np.median(v)) for k, v in t.items()}
        rng_ = lambda v: "%.4f [%.4f .. %.4f]" % (np.median(v), min(v), max(v))
        print("%-24s %22s %22s %16.1f %22s" % (name, rng_(t["one"]), rng_(t["stream"]), (med["stream"] - med["one"]) / spans * 1e6,
                                               rng_(t["first"])))
        print("    the first chunk is on the host after %.1f %% of the one call's time; the samples: %s"
              % (100 * med["first"] / med["one"], "bit-identical" if same else "DIFFERENT"))


def cli(a):
    import torch
    import generate_wavenet
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.models import create_model
    m = create_model("simple_wavenet", hparams_mod.load("wavenet"), device="cuda:0", dtype="bf16", seed=1234)
    print("device: %s; generate_wavenet.py main(), %d samples, seed walk of %d per restart, %d runs after a warm-up each"
          % (torch.cuda.get_device_name(0), a.samples, m.rf, a.calls))
    with tempfile.TemporaryDirectory() as tmp:
        ckpt = os.path.join(tmp, "model.ckpt-0")
        torch.save(m.state_dict(), ckpt)
        base = dict(checkpoint=ckpt, hparams="", gc_channels=None, lc_channels=None, local_condition=None, lc_hold=1, samples=a.samples,
                    fast_generation=True, temperature=1.0, precision="bf16", seed=0, wav_seed=None, save_every=None, wav_out_path=None)
        out = {}
        with open(os.devnull, "w") as null:
            for flag in ("save_every", "stream_chunk", None):
                secs = []
                for i in range(1 + a.calls):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    with contextlib.redirect_stdout(null):
                        wav = generate_wavenet.main(argparse.Namespace(**dict(base, **({flag: a.chunk} if flag else {}))))
                    secs.append(time.perf_counter() - t0)
                out[flag] = (wav, secs[1:])
        for flag in ("save_every", "stream_chunk", None):
            print("%-24s %s" % ("--%s %d" % (flag, a.chunk) if flag else "one call", "  ".join("%.3f" % s for s in out[flag][1])))
        print("--stream_chunk writes the samples of the one call: %s (--save_every draws other ones: a block of uniforms per "
              "chunk and a re-seeded generator)" % ("yes" if out["stream_chunk"][0] == out[None][0] else "NO"))
        print("medians: --save_every %.3f s, --stream_chunk %.3f s, one call %.3f s"
              % tuple(float(np.median(out[f][1])) for f in ("save_every", "stream_chunk", None)))


def synth(a):
    import torch
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.synthesizer import Synthesizer
    whp = hparams_mod.load("wavenet")
    whp.use_biases, whp.lc_channels = True, 80
    hp = hparams_mod.load("taco2")
    hp.max_iters = 60
    hparams_mod.set_hparams(hp)
    s = Synthesizer(hp).load(None, "taco2")
    s.load_vocoder(None, whp)
    total = hp.max_iters * hp.outputs_per_step * s._vocoder_hop
    print("device: %s; %d frames = %d samples = %.2f s of audio at %d Hz, initial weights; chunks of 20 hops = %d samples"
          % (torch.cuda.get_device_name(0), hp.max_iters * hp.outputs_per_step, total, total / hp.sample_rate, hp.sample_rate,
             20 * s._vocoder_hop))
    print("%-44s %s" % ("", "seconds, %d calls after a warm-up" % a.calls))
    whole, first, last, same = [], [], [], True
    for i in range(1 + a.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wav = s.synthesize("Hello, World.", vocoder="wavenet", seed=i)[0]
        whole.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pieces, t1 = [], None
        for piece in s.synthesize_stream("Hello, World.", seed=i):
            t1 = t1 or time.perf_counter() - t0
            pieces.append(piece)
        last.append(time.perf_counter() - t0)
        first.append(t1)
        same = same and np.array_equal(np.concatenate(pieces), wav) and len(wav) == total
    for name, v in (("synthesize: the waveform returned", whole), ("synthesize_stream: the first piece", first),
                    ("synthesize_stream: the last piece", last)):
        print("%-44s %s" % (name, "  ".join("%.3f" % x for x in v[1:])))
    print("the pieces side by side are synthesize's waveform, all %d samples drawn: %s" % (total, "yes" if same else "NO"))
    print("medians: first piece after %.3f s, the whole call %.3f s" % (float(np.median(first[1:])), float(np.median(whole[1:]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["cost", "stream", "cli", "synth", "all"], default="all")
    ap.add_argument("--samples", type=int, default=40000)
    ap.add_argument("--chunk", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    for what, fn in (("cost", cost), ("stream", stream), ("cli", cli), ("synth", synth)):
        if a.what in (what, "all"):
            fn(a)
            print(flush=True)


if __name__ == "__main__":
    main()
