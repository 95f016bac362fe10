"""What the sampling temperature and argmax cost the WaveNet generator's draw: us per drawn sample at the shipped
wavenet.yaml widths (50 layers, R = Dc = 32, S = 512, Q = 256), 2000 drawn samples behind a receptive-field seed, bf16
weights, batch 1 and 32, on

  engine 3              simple_wavenet, MFMA chain + helper workgroups
  engine 2              simple_wavenet, MFMA chain
  engine 2 conditioned  use_biases + lc_channels=80 at hold=250: one mel row per hop of audio.yaml

each as  parent T=1 | T=1 | T=0.7 | argmax.  "parent" is the library of the commit before the two fields, loaded beside
this one in the same process (the two fields lie in what that library's struct has as padding, so it reads the same block):

    git worktree add ../parent HEAD~1 && bash ../parent/nspeech_amd/csrc/build.sh
    python profiles/tools/wavenet_temperature_bench.py --parent-lib ../parent/nspeech_amd/csrc/libnspeech_hip.so

Without --parent-lib the parent column is left out.  One warm-up call per variant, then the modes alternate --reps times,
rotating which of them goes first (a mode's place in the order alone moved the median by up to 0.4 us);
a call is timed between device events, the seed walk by a one-draw call of its own in the same repetition and subtracted,
as bench.py does.  Expectation: T=1 within the parent's run-to-run spread, T=0.7 and argmax within that spread of T=1.

    python profiles/tools/wavenet_temperature_bench.py --resources DIR [--resources DIR2 ...]

prints instead the compiler's register and scratch report of the generation kernels in DIR/wavenet.hip (a csrc
directory), with the flags of DIR/build.sh; no device needed."""
import argparse
import contextlib
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

MODES = [("parent T=1", True, {}), ("T=1", False, {}), ("T=0.7", False, dict(temperature=0.7)), ("argmax", False, dict(temperature=0))]


def resources(csrc):
    sh = open(os.path.join(csrc, "build.sh")).read()
    flags = re.search(r'^FLAGS="([^"]*)"', sh, re.M).group(1).split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "wavenet.hip", "-o",
                        os.devnull], cwd=csrc, capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr[-2000:])
    print("%s/wavenet.hip" % csrc)
    print("  %-34s %6s %6s %14s %12s" % ("kernel", "VGPRs", "SGPRs", "scratch B/lane", "VGPR spills"))
    for b in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        name = b.split()[0]
        m = re.match(r"_Z\d+(wn_generate\w*kernel)(?:I(\w+?)E+v|\d)", name)       # a template's instantiation, or a plain kernel
        if not m:
            continue
        arg = {"Lb1": "<true>", "Lb0": "<false>", "Li32": "<32>", "Li16": "<16>", "DF16b": "<bf16>", "f": "<float>", None: ""}.get(m.group(2), m.group(2))

        def num(key):
            return int(re.search(re.escape(key) + r": (\d+)", b).group(1))
        print("  %-34s %6d %6d %14d %12d" % (m.group(1) + arg, num(" VGPRs"), num("TotalSGPRs"), num("ScratchSize [bytes/lane]"),
                                             num("VGPRs Spill")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--resources", action="append", default=None)
    a = ap.parse_args()
    if a.resources:
        for d in a.resources:
            resources(d)
        return
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
        assert parent.ns_version() <= this.ns_version(), "--parent-lib is newer than this library"

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
        rows += [("engine 3, batch %d" % B, simple, seed, {}, 3),
                 ("engine 2, batch %d" % B, simple, seed, dict(engine=2), 2),
                 ("engine 2 conditioned, batch %d" % B, local, seed, dict(local_conditions=mel, hold=hold, t0=-rf), 2)]
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
        """T = 1 on the parent's library and on this one at the same uniforms: the draws and last_probs, bit for bit."""
        un, out = rng.random((len(seed), 64)), []
        for handle in (parent, this):
            with library(handle):
                ids = m.generate(seed, 64, uniforms=un, **kw)
                out.append((ids.clone(), m.last_probs.clone()))
        return torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])

    print("device: %s; %d drawn samples behind a seed of %d, %d repetitions, the modes of a row alternated" %
          (torch.cuda.get_device_name(0), n, rf, a.reps))
    print("us per drawn sample: median [min .. max]")
    print("%-32s" % "variant" + "".join("%26s" % name for name, _, _ in modes))
    worst, identical = 0.0, True
    for name, m, seed, kw, eng in rows:
        for _, old, more in modes:           # warm-up
            timed(m, seed, 64, dict(kw, **more), old)
            assert m.last_engine == eng, (name, m.last_engine)
        if parent is not None:
            same = same_bits(m, seed, kw)
            identical = identical and same
        us = {mode: [] for mode, _, _ in modes}
        for r in range(a.reps):
            for mode, old, more in modes[r % len(modes):] + modes[:r % len(modes)]:      # every mode takes every place in turn
                k = dict(kw, **more)
                full, one = timed(m, seed, n, k, old), timed(m, seed, 1, k, old)
                us[mode].append((full - one) / (n - 1) * 1e6)
        v = {mode: np.asarray(x) for mode, x in us.items()}
        print("%-32s" % name + "".join("%10.2f [%5.2f ..%6.2f]" % (np.median(v[mode]), v[mode].min(), v[mode].max()) for mode, _, _ in modes))
        base = "parent T=1" if parent is not None else "T=1"
        spread = float(v[base].max() - v[base].min())
        for mode, _, _ in modes:
            if mode != base:
                over = float(np.median(v[mode]) - np.median(v["T=1" if mode in ("T=0.7", "argmax") else base]))
                flag = "" if over <= spread else "   <-- more than the spread"
                print("    %-10s against %-10s %+6.2f us (spread of %s: %.2f us)%s" %
                      (mode, "T=1" if mode in ("T=0.7", "argmax") else base, over, base, spread, flag))
                worst = max(worst, over - spread)
    if parent is not None:
        print("64 draws and last_probs at T=1, parent against this library at the same uniforms, every row: %s"
              % ("bit-identical" if identical else "DIFFERENT"))
    print("expectation (every difference within the spread between repeats): %s" % ("met" if worst <= 0 else "NOT met, see the flags"))


if __name__ == "__main__":
    main()
