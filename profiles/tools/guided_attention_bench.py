#!/usr/bin/env python3
"""Cost of the guided attention loss in the Tacotron-2 training step: `mixed` at the benchmark shape (N 32, T_in 160,
T_out 1000), guided_attention_weight 0 and 1 timed side by side in one process on ONE model and one device-resident
synthetic batch (bench.synthetic_batch) - the weight is switched between windows, so both forms run on the same
buffers (two model instances differ by up to 0.1 ms per step in phases this change does not touch) - alternated round by
round, each round a window of steps between two device synchronisations; the main-stream phases of both forms; and the
ns_guided_attention launch alone (device events around the call, on an otherwise idle chip).  The byte count of the pass
(read align, read-modify-write da0: 4 MB each at this shape) is computed from the shape.
Usage: python profiles/tools/guided_attention_bench.py [rounds] [steps per window]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from nspeech_amd import hparams as hparams_mod  # noqa: E402
from nspeech_amd.models import create_model  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
N, TI, TO = 32, 160, 1000


def model(batch):
    hp = hparams_mod.load("taco2")
    m = create_model("taco2", hp, device="cuda:0", dtype="mixed", seed=1234)
    m.add_loss().add_optimizer(global_step=0)
    m.initialize(batch[0], batch[1], None, batch[2], batch[3])       # uploads the batch once; the steps re-run it from HBM
    for w in (0.0, 1.0):
        m.guided_weight = w         # what hparams.guided_attention_weight sets
        for _ in range(3):
            m.step(read_loss=False)
    torch.cuda.synchronize()
    m.check_status()
    return m


def window(m, weight):
    m.guided_weight = weight
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        m.step(read_loss=False)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / STEPS * 1e3


def phases(m, weight, steps=10):
    """Mean main-stream time between the model's phase ticks (Tacotron2._tick) over `steps` steps as they are timed above,
    weight gradients on the second stream: {label: ms}.  The guided launch sits in the phase that ends at attn_rnn_bwd."""
    sums = {}
    m.guided_weight = weight
    for _ in range(steps):
        m.timing = []
        m.step(read_loss=False)
        torch.cuda.synchronize()
        tm, m.timing = m.timing, None
        for i in range(1, len(tm)):
            sums[tm[i][0]] = sums.get(tm[i][0], 0.0) + tm[i - 1][1].elapsed_time(tm[i][1])
    return {k: v / steps for k, v in sums.items()}


def launch_alone(m, reps=50):
    """ns_guided_attention as backward() issues it, alone on the chip: ms per call (two kernels: rows, then the means)."""
    da0 = m._bufs["d_a0"]
    keep = da0.clone()
    for _ in range(5):
        m._guided_attention(da0, m.scal, 4)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        m._guided_attention(da0, m.scal, 4)
    e1.record()
    torch.cuda.synchronize()
    da0.copy_(keep)
    return e0.elapsed_time(e1) / reps


def main():
    dev = torch.device("cuda:0")
    print("# guided attention loss: Tacotron-2 mixed, N %d, T_in %d, T_out %d; %s; %d rounds of %d steps per weight"
          % (N, TI, TO, torch.cuda.get_device_name(dev), ROUNDS, STEPS))
    hp = hparams_mod.load("taco2")
    batch = bench.synthetic_batch(hp, N, TI, TO, 1234)
    m1 = model(batch)
    times = {0.0: [], 1.0: []}
    for rnd in range(ROUNDS):
        for w in ((0.0, 1.0) if rnd % 2 == 0 else (1.0, 0.0)):         # alternate which one goes first
            times[w].append(window(m1, w))
        print("round %d: weight 0 %.3f ms/step | weight 1 %.3f ms/step" % (rnd, times[0.0][-1], times[1.0][-1]), flush=True)
    m1.check_status()
    med = {w: float(np.median(v)) for w, v in times.items()}
    spread = {w: (min(v), max(v)) for w, v in times.items()}
    print("median ms/step: weight 0 %.3f (%.3f .. %.3f) | weight 1 %.3f (%.3f .. %.3f) | difference %+.3f ms = %+.2f %%"
          % (med[0.0], spread[0.0][0], spread[0.0][1], med[1.0], spread[1.0][0], spread[1.0][1], med[1.0] - med[0.0],
             100.0 * (med[1.0] - med[0.0]) / med[0.0]))
    ph = {w: phases(m1, w) for w in (0.0, 1.0)}
    print("main-stream phases, ms (mean of 10 steps; weight 0 | weight 1 | difference), those that differ by 0.01 ms or more:")
    for k in ph[0.0]:
        d01 = ph[1.0][k] - ph[0.0][k]
        if abs(d01) >= 0.01:
            print("  %-20s %8.3f | %8.3f | %+.3f" % (k, ph[0.0][k], ph[1.0][k], d01))
    print("  %-20s %8.3f | %8.3f | %+.3f" % ("all phases", sum(ph[0.0].values()), sum(ph[1.0].values()),
                                             sum(ph[1.0].values()) - sum(ph[0.0].values())))
    d = m1.dims
    S, Tia = d["S"], (d["Ti"] + 7) // 8 * 8
    ms = launch_alone(m1)
    valid = float(sum(int(t) for t in batch[1])) * S                    # S_n = S on a synthetic batch
    moved = 3 * 4 * valid                                               # read align; read and write da0
    print("ns_guided_attention alone: %.4f ms per call (two kernels); align / da0 are [%d, %d, %d] fp32 = %.2f MB each, the "
          "valid region moves %.2f MB -> %.0f GB/s" % (ms, N, S + 1, Tia, N * (S + 1) * Tia * 4 / 1e6, moved / 1e6,
                                                         moved / (ms * 1e-3) / 1e9))
    m1.read_losses()
    print("after the run (last steps at weight 1): loss %.5f, attention_loss %.6f, attention_focus %.5f; paths attn:bwd = %s"
          % (m1.loss, m1.attention_loss, m1.attention_focus, m1.last_paths.get("attn:bwd")))


if __name__ == "__main__":
    main()
