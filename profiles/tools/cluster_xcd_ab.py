#!/usr/bin/env python3
"""Placement of the persistent kernels' clusters (NS_CLUSTER_XCD = 0 linear / 1 one XCD per cluster), alternated in one
process at the benchmark's shapes:
  1. the probe's XCD ids (ns_cluster_probe), linear and placed;
  2. the BiLSTM cluster kernels alone through the C ABI (the harness of cluster_rows_trace.py): launch time and the
     in-kernel hop of workgroup 0 (NS_CLUSTER_DBG=16 stamps);
  3. every persistent launch of a Tacotron-2 and of a Tacotron-1 training pass (32 x 160 -> 1000, `mixed`, one stream),
     with device events around the call: ns_lstm_cluster_*, ns_taco2_attn_cluster_*, ns_gru_seq_*,
     ns_taco1_attn_cluster_*, and ns_lstm_wide_* (which the switch does not reach: a control; it did while the remap of
     profiles/cluster_xcd.txt section 4 was tried); with NS_ATTN_TRACE=1 in the environment also workgroup 0's step and
     wait times inside the Tacotron-2 attention kernels.
Usage: python profiles/tools/cluster_xcd_ab.py [rounds]"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import cluster_rows_trace as crt  # noqa: E402
from nspeech_amd import _lib, hparams as hparams_mod, ops  # noqa: E402
from nspeech_amd.models import create_model  # noqa: E402

dev = torch.device("cuda:0")
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
MODES = (("0", "linear"), ("1", "placed"))


def probe(clusters, members, placed):
    xcc = torch.full((clusters * members,), -1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().ns_cluster_probe(clusters, members, placed, ctypes.c_void_p(xcc.data_ptr()),
                                           ctypes.c_void_p(ops.stream())), "ns_cluster_probe")
    torch.cuda.synchronize()
    return xcc.view(clusters, members).cpu().tolist()


def bilstm_alone():
    print("\n## 2. BiLSTM cluster kernels alone, H 256, N 32, default rows per chain; ms per launch | hop of workgroup 0, us")
    for T, fp32 in ((1000, False), (160, True), (160, False)):
        _, fp, bp, w = crt.setup(32, T, 256, fp32)
        for rnd in range(ROUNDS):
            for value, name in MODES:
                os.environ["NS_CLUSTER_XCD"] = value
                tf, ff = crt.timed("fwd", fp, w)
                line = "T %4d %s round %d %-6s forward %.4f ms (%d rows)" % (T, "fp32 state" if fp32 else "bf16", rnd, name, tf, ff)
                if not fp32:
                    c = crt.stamps("fwd", fp, w, 32, 256, 100, min(500, T - 1))
                    line += " hop %.3f" % (c[5][1:] - c[2][:-1]).mean()
                    tb, fb = crt.timed("bwd", bp, w)
                    c = crt.stamps("bwd", bp, w, 32, 256, 100, min(500, T - 1))
                    line += " | backward %.4f ms (%d rows) hop %.3f" % (tb, fb, (c[4][1:] - c[7][:-1]).mean())
                print(line, flush=True)


def key_of(name, args):
    direction = args[0]
    p = args[1] if len(args) > 1 else None
    shape = ""
    if isinstance(p, ctypes.Structure):
        shape = " T %d H %d%s" % (p.T, p.H, " fp32" if p.dtype == ops.NS_F32 else "")
    return "%s %s%s" % (name, direction, shape)


def attn_stamps(work, S, waits):
    tr = work[-(256 * 16 * 2):].view(torch.int64).view(256, 16).cpu().numpy().astype(np.float64)
    rows, nxt = tr[4:min(S, 256) - 1], tr[5:min(S, 256)]
    step = (nxt[:, 0] - rows[:, 0]).mean() * 1e-2
    return step, [(rows[:, k + 1] - rows[:, k]).mean() * 1e-2 for k in waits]


def model_pass(kind):
    print("\n## 3. %s training pass, 32 x 160 -> 1000, mixed, one stream: ms per launch (mean of 3 passes)" % kind)
    hp = hparams_mod.load(kind)
    m = create_model(kind, hp, device="cuda:0", dtype="mixed", seed=1234)
    inputs, lengths, mel, lin = bench.synthetic_batch(hp, 32, 160, 1000, 1234)
    m.add_optimizer(0)
    m.overlap_wgrads = False
    names = ("lstm_cluster", "taco2_attn_cluster", "lstm_wide", "gru_seq", "taco1_attn_cluster")
    orig = {n: getattr(ops, n) for n in names}
    ev = []

    def wrap(n):
        def f(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            orig[n](*args, **kw)
            e1.record()
            ev.append((key_of(n, args), e0, e1))
        return f
    for n in names:
        setattr(ops, n, wrap(n))
    table = {}
    try:
        for rnd in range(ROUNDS):
            for value, name in MODES:
                os.environ["NS_CLUSTER_XCD"] = value
                m.initialize(inputs, lengths, None, mel, lin)
                m.backward()
                torch.cuda.synchronize()
                del ev[:]
                for _ in range(3):
                    m.initialize(inputs, lengths, None, mel, lin)
                    m.backward()
                torch.cuda.synchronize()
                m.check_status()
                sums = {}
                for k, e0, e1 in ev:
                    sums.setdefault(k, []).append(e0.elapsed_time(e1))
                for k, v in sums.items():           # (a key that occurs several times per pass: the sum per pass)
                    table.setdefault(k, {}).setdefault(name, []).append(sum(v) / 3)
                if kind == "taco2" and os.environ.get("NS_ATTN_TRACE"):
                    fs, fw = attn_stamps(m._status_words[("attn", "fwd")], 200, (3, 8))
                    bs, bw = attn_stamps(m._status_words[("attn", "bwd")], 200, (4, 7))
                    print("round %d %-6s attention stamps, us per step: forward %.3f (X2 wait %.3f, X3 wait %.3f) | backward %.3f "
                          "(E2 wait %.3f, E3 wait %.3f)" % (rnd, name, fs, fw[0], fw[1], bs, bw[0], bw[1]), flush=True)
    finally:
        for n in names:
            setattr(ops, n, orig[n])
    for k in sorted(table):
        lin_, pla = table[k]["linear"], table[k]["placed"]
        verdict = "placed wins every run" if max(pla) < min(lin_) else ("linear wins every run" if max(lin_) < min(pla) else "overlap")
        print("%-40s linear %s | placed %s | %s" % (k, " ".join("%.4f" % x for x in lin_), " ".join("%.4f" % x for x in pla), verdict))


def main():
    print("# cluster placement A/B; %s, %d CUs, %d rounds" % (torch.cuda.get_device_name(dev),
                                                             torch.cuda.get_device_properties(dev).multi_processor_count, ROUNDS))
    print("\n## 1. XCD id of every (cluster, member), members = 4")
    for clusters in (16, 5):
        for placed, name in ((0, "linear"), (1, "placed")):
            print("clusters %2d %-6s %s" % (clusters, name, probe(clusters, 4, placed)))
    bilstm_alone()
    model_pass("taco2")
    model_pass("taco1")


if __name__ == "__main__":
    main()
