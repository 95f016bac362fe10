#!/usr/bin/env python3
"""Cost of prenet dropout (hparam prenet_dropout) in the training step of both Tacotron models: `mixed` at the benchmark
shape (N 32, T_in 160, T_out 1000), the option off and on (drop_rate 0.5) timed side by side in one process on ONE model
per kind and one device-resident synthetic batch (bench.synthetic_batch) - the switch is flipped between windows, so both
forms run on the same buffers (profiles/guided_attention.txt, section 2: two instances of a model differ by 0.1 ms per
step in phases a change does not touch) - alternated round by round, each round a window of steps between two device
synchronisations; and the main-stream phases that hold the attention recurrences.
On a tree without the option the switch does nothing: both columns then time the same step (the "off" figure of a parent
commit, for the default-off comparison).
Usage: python profiles/tools/prenet_dropout_bench.py [rounds] [steps per window] [taco2,taco1]"""
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
KINDS = sys.argv[3].split(",") if len(sys.argv) > 3 else ["taco2", "taco1"]
N, TI, TO = 32, 160, 1000


def model(kind, batch):
    hp = hparams_mod.load(kind)
    hp.drop_rate = 0.5
    m = create_model(kind, hp, device="cuda:0", dtype="mixed", seed=1234)
    m.drop_rate = 0.5
    m.add_optimizer(global_step=0)
    m.initialize(batch[0], batch[1], None, batch[2], batch[3])       # uploads the batch once; the steps re-run it from HBM
    for on in (False, True):
        m.prenet_dropout = on       # what hparams.prenet_dropout sets
        for _ in range(3):
            m.step(read_loss=False)
    torch.cuda.synchronize()
    m.check_status()
    return m


def window(m, on):
    m.prenet_dropout = on
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        m.step(read_loss=False)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / STEPS * 1e3


def phases(m, on, steps=10):
    """Mean main-stream time between the model's phase ticks (Tacotron2._tick) over `steps` steps: {label: ms}."""
    sums = {}
    m.prenet_dropout = on
    for _ in range(steps):
        m.timing = []
        m.step(read_loss=False)
        torch.cuda.synchronize()
        tm, m.timing = m.timing, None
        for i in range(1, len(tm)):
            sums[tm[i][0]] = sums.get(tm[i][0], 0.0) + tm[i - 1][1].elapsed_time(tm[i][1])
    return {k: v / steps for k, v in sums.items()}


def main():
    dev = torch.device("cuda:0")
    from nspeech_amd.models.tacotron2 import Tacotron2
    has = hasattr(Tacotron2, "prenet_dropout_args")
    print("# prenet dropout: mixed, N %d, T_in %d, T_out %d; %s; %d rounds of %d steps per form; the tree %s the option"
          % (N, TI, TO, torch.cuda.get_device_name(dev), ROUNDS, STEPS, "has" if has else "does NOT have"))
    for kind in KINDS:
        hp = hparams_mod.load(kind)
        batch = bench.synthetic_batch(hp, N, TI, TO, 1234)
        m = model(kind, batch)
        times = {False: [], True: []}
        for rnd in range(ROUNDS):
            for on in ((False, True) if rnd % 2 == 0 else (True, False)):         # alternate which one goes first
                times[on].append(window(m, on))
            print("%s round %d: off %.3f ms/step | on %.3f ms/step" % (kind, rnd, times[False][-1], times[True][-1]), flush=True)
        m.check_status()
        med = {k: float(np.median(v)) for k, v in times.items()}
        print("%s median ms/step: off %.3f (%.3f .. %.3f) | on %.3f (%.3f .. %.3f) | difference %+.3f ms = %+.2f %%"
              % (kind, med[False], min(times[False]), max(times[False]), med[True], min(times[True]), max(times[True]),
                 med[True] - med[False], 100.0 * (med[True] - med[False]) / med[False]))
        if kind == "taco2":
            ph = {on: phases(m, on) for on in (False, True)}
            print("taco2 main-stream phases, ms (mean of 10 steps; off | on | difference), those that differ by 0.01 ms or more:")
            for k in ph[False]:
                d = ph[True][k] - ph[False][k]
                if abs(d) >= 0.01 or k in ("attn_rnn", "attn_rnn_bwd"):
                    print("  %-20s %8.3f | %8.3f | %+.3f" % (k, ph[False][k], ph[True][k], d))
            S = m.dims["S"]
            for k in ("attn_rnn", "attn_rnn_bwd"):
                if k in ph[False]:
                    print("  %s per decoder step: off %.2f us | on %.2f us" % (k, ph[False][k] * 1e3 / S, ph[True][k] * 1e3 / S))
        m.prenet_dropout = True
        m.step(read_loss=False)
        m.read_losses()
        args = m.prenet_dropout_args() if has else None
        print("%s after the run (last step with the option on): loss %.5f; paths attn:fwd = %s, attn:bwd = %s; dropout block %s"
              % (kind, m.loss, m.last_paths.get("attn:fwd"), m.last_paths.get("attn:bwd"), "set" if args else "none"))
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
