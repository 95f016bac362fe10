#!/usr/bin/env python
"""Two-stream phase table of the Tacotron-2 training step at the benchmark shape (Tacotron2.timing: one event per
phase on the main stream, the weight gradients on the second stream as in the timed steps), median of --steps steps,
for each setting of NS_WGRAD_GROUP given; the settings are interleaved step by step in one process.

    python profiles/tools/wgrad_group_phases.py [--steps 10] [--root DIR] default none decoder postnet,head all

--root: the tree to import bench.py and nspeech_amd from (a checkout of the parent commit ignores the settings)."""
import argparse
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("settings", nargs="*", default=["default", "none"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    import bench
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.models import create_model
    hp = hparams_mod.load("taco2")
    m = create_model("taco2", hp, device="cuda:0", dtype="mixed", seed=1234)
    m.deterministic = True
    inputs, lengths, mel, lin = bench.synthetic_batch(hp, 32, 160, 1000, 1234)
    m.add_optimizer(global_step=0)
    m.initialize(inputs, lengths, None, mel, lin)

    def step(setting):
        if setting == "default":
            os.environ.pop("NS_WGRAD_GROUP", None)
        else:
            os.environ["NS_WGRAD_GROUP"] = {"none": "", "all": "decoder,postnet,head"}.get(setting, setting)
        m.forward_train()
        m.backward()
        m.apply_gradients()

    for s in a.settings * 3:
        step(s)
    torch.cuda.synchronize()
    rows = {s: {} for s in a.settings}
    order = []
    for _ in range(a.steps):
        for s in a.settings:
            m.timing = []
            step(s)
            torch.cuda.synchronize()
            tm, m.timing = m.timing, None
            for i in range(1, len(tm)):
                if tm[i][0] not in order:
                    order.append(tm[i][0])
                rows[s].setdefault(tm[i][0], []).append(tm[i - 1][1].elapsed_time(tm[i][1]))
            rows[s].setdefault("step", []).append(tm[0][1].elapsed_time(tm[-1][1]))
    print("%-22s" % "phase (ms, median of %d)" % a.steps + "".join("%14s" % s for s in a.settings))
    for name in order + ["step"]:
        print("%-22s" % name + "".join("%14.3f" % statistics.median(rows[s].get(name, [float("nan")])) for s in a.settings))
    print("wgrad_group (queues, items per launch):", getattr(m, "wgrad_group", None))


if __name__ == "__main__":
    main()
