#!/usr/bin/env python3
"""Cost of the stop token (hparam stop_token): (1) the Tacotron-2 `mixed` training step at the benchmark shape (N 32,
T_in 160, T_out 1000) with the term off and on, timed side by side in one process on ONE model and one device-resident
synthetic batch (bench.synthetic_batch) - the model is built with stop_token=true and its `stop_token` attribute is
switched between windows, so both forms run on the same buffers (two model instances differ by up to 0.1 ms per step in
phases this change does not touch); off is then a model that carries the two variables (1032 floats of 28 M) but issues
no launch - alternated round by round, each round a window of steps between two device synchronisations; (2) the
ns_stop_token launch alone on an otherwise idle chip (device events around the calls), in training form on fp32 and on
bf16 h and in synthesis form, with the bytes each form moves and the achieved GB/s against the 6.3 TB/s a float4 copy
reaches on this chip (8 TB/s spec); (3) 300-step batch-1 synthesis (graph replay) with the switch off and on, two models,
alternated windows.
Usage: python profiles/tools/stop_token_bench.py [rounds] [steps per window]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from nspeech_amd import hparams as hparams_mod  # noqa: E402
from nspeech_amd import ops  # noqa: E402
from nspeech_amd.models import create_model  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
N, TI, TO = 32, 160, 1000
HBM_COPY = 6.3e12


def model(batch):
    hp = hparams_mod.load("taco2")
    hp.stop_token = True
    m = create_model("taco2", hp, device="cuda:0", dtype="mixed", seed=1234)
    m.add_loss().add_optimizer(global_step=0)
    m.initialize(batch[0], batch[1], None, batch[2], batch[3])       # uploads the batch once; the steps re-run it from HBM
    for on in (False, True):
        m.stop_token = on
        for _ in range(3):
            m.step(read_loss=False)
    torch.cuda.synchronize()
    m.check_status()
    return m


def window(m, on):
    m.stop_token = on
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        m.step(read_loss=False)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / STEPS * 1e3


def timed(fn, reps=50):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def launch_alone(S, D):
    dev = torch.device("cuda:0")
    S1 = S + 1
    g = torch.Generator(device=dev).manual_seed(1)
    h32 = torch.randn(N, S1, D, device=dev, generator=g) * 0.1
    h16 = h32.to(torch.bfloat16)
    w = torch.randn(D, device=dev, generator=g) * 0.05
    b = torch.zeros(8, device=dev)
    dh = torch.zeros(N, S1, D, device=dev)
    dw, db = torch.zeros(D, device=dev), torch.zeros(8, device=dev)
    acc = torch.zeros(8, device=dev)
    logits = torch.zeros(N * S, device=dev)
    steps = torch.zeros(N, dtype=torch.int32, device=dev)
    work = torch.zeros(ops.stop_token_work_floats(N, S, D), device=dev)
    rows = N * S
    part = (work.numel() - rows - N) * 4 * 2            # the partials: written by the first kernel, read by the second
    for name, h in (("fp32", h32), ("bf16", h16)):
        ms = timed(lambda: ops.stop_token(N, S, D, h, S1 * D, D, w, b, work, h_off=D, grad_scale=1.0, dh=dh, dh_off=D,
                                          dh_sn=S1 * D, dh_ss=D, dw=dw, db=db, acc=acc))
        moved = rows * D * (h.element_size() + 8) + part
        print("ns_stop_token alone, training form, %s h: %.4f ms per call (two kernels); h %.1f MB read, dh %.1f MB read and "
              "%.1f MB written, partials %.1f MB -> %.0f GB/s = %.0f %% of the 6.3 TB/s copy rate"
              % (name, ms, rows * D * h.element_size() / 1e6, rows * D * 4 / 1e6, rows * D * 4 / 1e6, part / 1e6,
                 moved / (ms * 1e-3) / 1e9, 100.0 * moved / (ms * 1e-3) / HBM_COPY))
    ms = timed(lambda: ops.stop_token(N, S, D, h32, S1 * D, D, w, b, work, h_off=D, logits=logits, threshold=0.5,
                                      stop_steps=steps))
    moved = rows * D * 4
    print("ns_stop_token alone, synthesis form, fp32 h at this shape: %.4f ms per call; h %.1f MB read -> %.0f GB/s = %.0f %%"
          % (ms, moved / 1e6, moved / (ms * 1e-3) / 1e9, 100.0 * moved / (ms * 1e-3) / HBM_COPY))
    h1 = torch.randn(1, 301, D, device=dev, generator=g) * 0.1
    ms = timed(lambda: ops.stop_token(1, 300, D, h1, 301 * D, D, w, b, work, h_off=D, logits=logits, threshold=0.5,
                                      stop_steps=steps))
    print("ns_stop_token alone, synthesis form, N 1, S 300 (1.2 MB): %.4f ms per call (launch-bound)" % ms)


def synthesis(rounds, reps=20):
    from nspeech_amd.utils.text import text_to_sequence
    seq = text_to_sequence("The first measurement took twelve milliseconds; the second one took longer.", ["english_cleaners"])
    inputs, lengths = np.asarray([seq], np.int32), np.asarray([len(seq)], np.int32)
    ms = {}
    models = {}
    for on in (False, True):
        hp = hparams_mod.load("taco2")
        hp.max_iters = 300
        hp.stop_token = on
        m = create_model("taco2", hp, device="cuda:0", dtype="mixed", seed=1234)
        for _ in range(4):              # eager, capture + replay, replays
            m.initialize(inputs, lengths)
        torch.cuda.synchronize()
        m.check_status()
        models[on], ms[on] = m, []
    for rnd in range(rounds):
        for on in ((False, True) if rnd % 2 == 0 else (True, False)):
            m = models[on]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                m.initialize(inputs, lengths)
            torch.cuda.synchronize()
            ms[on].append((time.perf_counter() - t0) / reps * 1e3)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print("synthesis, batch 1, 300 steps (%d symbols, graph replay, path %s), median ms per pass: switch off %.3f (%.3f .. %.3f)"
          " | on %.3f (%.3f .. %.3f) | difference %+.3f ms = %+.2f %%; stop step of the untrained model: %d"
          % (len(seq), models[True].last_paths.get("decode"), med[False], min(ms[False]), max(ms[False]), med[True],
             min(ms[True]), max(ms[True]), med[True] - med[False], 100.0 * (med[True] - med[False]) / med[False],
             int(models[True].stop_steps[0])))


def main():
    dev = torch.device("cuda:0")
    print("# stop token: Tacotron-2 mixed, N %d, T_in %d, T_out %d; %s; %d rounds of %d steps per form"
          % (N, TI, TO, torch.cuda.get_device_name(dev), ROUNDS, STEPS))
    hp = hparams_mod.load("taco2")
    batch = bench.synthetic_batch(hp, N, TI, TO, 1234)
    m1 = model(batch)
    times = {False: [], True: []}
    for rnd in range(ROUNDS):
        for on in ((False, True) if rnd % 2 == 0 else (True, False)):         # alternate which one goes first
            times[on].append(window(m1, on))
        print("round %d: off %.3f ms/step | on %.3f ms/step" % (rnd, times[False][-1], times[True][-1]), flush=True)
    m1.check_status()
    med = {k: float(np.median(v)) for k, v in times.items()}
    print("median ms/step: off %.3f (%.3f .. %.3f) | on %.3f (%.3f .. %.3f) | difference %+.3f ms = %+.2f %%"
          % (med[False], min(times[False]), max(times[False]), med[True], min(times[True]), max(times[True]),
             med[True] - med[False], 100.0 * (med[True] - med[False]) / med[False]))
    m1.stop_token = True
    m1.step(read_loss=False)
    m1.read_losses()
    print("after the run: loss %.5f, stop_loss %.6f, stop_step_error %.3f; the kernel read %s h"
          % (m1.loss, m1.stop_loss, m1.stop_step_error, m1.stop_h_dtype))
    S, D = m1.dims["S"], hp.decoder_lstm_units
    del m1
    torch.cuda.empty_cache()
    launch_alone(S, D)
    synthesis(ROUNDS)


if __name__ == "__main__":
    main()
