"""Tacotron-1 synthesis: the persistent decoder loop (ns_taco1_decode) against the launch-per-step loop, alternating in
one process.  Times Tacotron.initialize() (encoder, decoder loop, post-CBHG, linear head) and, inside it, the decoder
section alone (from the end of the encoder CBHG to the start of the post CBHG: memory keys, the loop on either path, the
output projection) with device events after a warm-up, at max_iters = 300, T_in = 160, N = 1, 2, 4, 16 and 32, mode
`mixed`; reads the status words after every timed call; prints one JSON line.

    python profiles/tools/taco1_decode_bench.py [--reps 5] [--steps 300] [--ti 160] [--ns 1,2,4,16,32] [--only persistent|step]

"launches" counts the C-ABI entry points one call makes (each enqueues one kernel, a few two: the persistent kernels
clear their exchange buffers first; ns_taco1_decode above its rows per launch: one kernel per launch).  "spread" is
(max - min) / median of the timed calls.  --only runs one path (for a rocprofv3 trace of it)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--ti", type=int, default=160)
    ap.add_argument("--ns", default="1,2,4,16,32")
    ap.add_argument("--only", choices=("persistent", "step"), default=None)
    a = ap.parse_args()
    from nspeech_amd import _lib
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.models import create_model
    from util import make_batch

    calls = [0]
    check = _lib.check

    def counting_check(rc, what):
        calls[0] += 1
        return check(rc, what)
    _lib.check = counting_check

    hp = hparams_mod.load("taco1")
    hp.max_iters = a.steps
    m = create_model("taco1", hp, device="cuda:0", dtype="mixed", seed=1)
    paths = [a.only] if a.only else ["persistent", "step"]
    # the decoder section of initialize(): events behind the encoder CBHG and ahead of the post CBHG
    marks = [None, None]
    cbhg = m._cbhg

    def marked_cbhg(name, *args, **kw):
        if name == "post" and marks[1] is not None:
            marks[1].record()
        out = cbhg(name, *args, **kw)
        if name == "enc" and marks[0] is not None:
            marks[0].record()
        return out
    m._cbhg = marked_cbhg
    res = dict(metric="taco1_synthesis", mode="mixed", max_iters=a.steps, T_in=a.ti, reps=a.reps, device=torch.cuda.get_device_name(0))
    for N in [int(x) for x in a.ns.split(",")]:
        inputs, lengths, _, _ = make_batch(hp, N, a.ti, 10, seed=N)
        lengths = np.full(N, a.ti, np.int32)
        times = {p: [] for p in paths}
        loops = {p: [] for p in paths}
        outs, launches = {}, {}
        for p in paths:                     # warm-up (buffers, shadows, code objects)
            m.use_decode_kernel = p == "persistent"
            m.initialize(inputs, lengths)
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for p in paths:
                m.use_decode_kernel = p == "persistent"
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                marks[0], marks[1] = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                calls[0] = 0
                e0.record()
                m.initialize(inputs, lengths)
                e1.record()
                launches[p] = calls[0]
                torch.cuda.synchronize()
                m.check_status()
                assert m.last_paths["decode"] == p, m.last_paths
                times[p].append(e0.elapsed_time(e1))
                loops[p].append(marks[0].elapsed_time(marks[1]))
                outs[p] = m.mel_outputs.float().cpu().numpy().copy()
        for p in paths:
            ms = float(np.median(times[p]))
            res["%s_n%d_ms" % (p, N)] = round(ms, 3)
            res["%s_n%d_spread" % (p, N)] = round((max(times[p]) - min(times[p])) / ms, 3)
            lp = float(np.median(loops[p]))
            res["%s_n%d_decode_ms" % (p, N)] = round(lp, 3)
            res["%s_n%d_decode_us_per_step" % (p, N)] = round(1e3 * lp / a.steps, 2)
            res["%s_n%d_decode_spread" % (p, N)] = round((max(loops[p]) - min(loops[p])) / lp, 3)
            res["%s_n%d_launches" % (p, N)] = launches[p]
        if len(paths) == 2:
            d = float(np.abs(outs["persistent"] - outs["step"]).max() / np.abs(outs["step"]).max())
            res["n%d_speedup" % N] = round(res["step_n%d_ms" % N] / res["persistent_n%d_ms" % N], 2)
            res["n%d_decode_speedup" % N] = round(res["step_n%d_decode_ms" % N] / res["persistent_n%d_decode_ms" % N], 2)
            res["n%d_max_rel_diff" % N] = float("%.3e" % d)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
