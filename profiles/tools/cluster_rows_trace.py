#!/usr/bin/env python3
"""Rows per chain of the BiLSTM cluster kernels (NS_CLUSTER_ROWS = 16 / 8 / 4), the kernels alone through the C ABI:
launch time (device events, no stamps) and the in-kernel slot split (NS_CLUSTER_DBG=16: 100 MHz stamps of workgroup 0)
at the benchmark's expand shape (T 1000, H 256, N 32), at N 1 (synthesis), and the launch time of the fp32-state
forward at the encoder shape (T 160, H 256, N 32), which takes no stamps.
Forward stamps per slot: [0] compute start behind the slot barrier, [1] product + cell update done, [2] h published;
poller: [4] starts waiting for the slot's h, [5] has it, [6] poll passes beyond the first / 100.
Backward stamps per slot: [0] slot start, [4] the peers' sums are in ([6] extra poll passes / 100), [1] cell update done
+ operand image written, [2] behind the barrier, [3] MFMAs done, [7] partial sums published."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nspeech_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
bf = torch.bfloat16


def setup(N, T, H, fp32):
    g = torch.Generator().manual_seed(N + T)
    P, padl = T + 4, 2
    rows = N * P
    out = dict(h=torch.zeros(rows * 2 * H, dtype=torch.float32 if fp32 else bf, device=dev),
               hb=torch.zeros(rows * 2 * H, dtype=bf, device=dev))
    dh = (torch.randn(rows, 2 * H, generator=g) * 0.1).to(dev)
    fp, bp = [], []
    if fp32:
        ops.F32_PASSES = 3
    for di, d in enumerate(("fw", "bw")):
        xg = torch.randn(rows, 4 * H, generator=g).to(dev)
        w = torch.randn(H, 4 * H, generator=g) / H ** 0.5
        c = torch.zeros(rows * H, device=dev)
        gates = torch.zeros(rows * 4 * H, dtype=bf, device=dev)
        dg = torch.zeros(rows * 4 * H, dtype=bf, device=dev)
        out[d] = (xg, c, gates, dg)
        if fp32:
            whT = w.t().contiguous().to(dev)
            hi = whT.to(bf)
            lo = (whT - hi.float()).to(bf)
            out["w" + d] = (whT, hi, lo)
            fp.append(ops.lstm_seq_params(N, T, H, P, padl, xg, 4 * H, whT, None, None, d == "bw", out["h"], 2 * H, c, gates,
                                          h_off=di * H, whT_hi=hi, whT_lo=lo, h_bf16=out["hb"], h_bf16_off=di * H,
                                          ld_h_bf16=2 * H))
            continue
        whT = w.t().contiguous().to(bf).to(dev)
        wh = w.to(bf).to(dev).contiguous()
        work = torch.zeros(N * H + 64, device=dev)
        out["w" + d] = (whT, wh, work)
        fp.append(ops.lstm_seq_params(N, T, H, P, padl, xg, 4 * H, whT, None, None, d == "bw", out["h"], 2 * H, c, gates,
                                      h_off=di * H))
        bp.append(ops.lstm_seq_params(N, T, H, P, padl, xg, 4 * H, None, wh, None, d == "bw", out["h"], 2 * H, c, gates,
                                      dh=dh, ld_dh=2 * H, dgates=dg, work=work, dh_off=di * H, h_off=di * H))
    ops.F32_PASSES = 0
    out["dh"] = dh
    w = torch.zeros(ops.lstm_cluster_work_floats(fp[0]), device=dev)
    return out, fp, bp, w


def timed(direction, pair, w, reps=5):
    for _ in range(2):
        ops.lstm_cluster(direction, pair[0], pair[1], w)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ops.lstm_cluster(direction, pair[0], pair[1], w)
    e1.record()
    torch.cuda.synchronize()
    assert int(w[:1].view(torch.int32).item()) == 0, "status word"
    return e0.elapsed_time(e1) / reps, int(w[1:2].view(torch.int32).item()) or 16


def stamps(direction, pair, w, N, H, q0, q1):
    os.environ["NS_CLUSTER_DBG"] = "16"
    ops.lstm_cluster(direction, pair[0], pair[1], w)
    torch.cuda.synchronize()
    del os.environ["NS_CLUSTER_DBG"]
    off = 256 + 4096 + 2 * ((N + 15) // 16 + 1) * 2 * 16 * (4 * H // 2) * 8
    tr = w.view(torch.uint8)[off:off + 512 * 8 * 8].view(torch.int64).view(512, 8).cpu().numpy().astype(np.float64) * 0.01
    return [tr[q0:q1, i] for i in range(8)]


def main():
    T, H = 1000, 256
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    print("# rows per chain of the BiLSTM cluster kernels; %s, %d CUs" % (torch.cuda.get_device_name(dev), cus))
    os.environ.pop("NS_CLUSTER_ROWS", None)
    for N in (32, 1):
        _, fp, bp, w = setup(N, T, H, False)
        print("\n## bf16 forward + partial-sum backward, T %d, H %d, N %d" % (T, H, N))
        _, dflt_f = timed("fwd", fp, w, 1)
        _, dflt_b = timed("bwd", bp, w, 1)
        print("default form (no override): forward %d rows, backward %d rows" % (dflt_f, dflt_b))
        for rows in (16, 8, 4):
            os.environ["NS_CLUSTER_ROWS"] = str(rows)
            tf, ff = timed("fwd", fp, w)
            c = stamps("fwd", fp, w, N, H, 100, 500)
            grid = 2 * ((N + ff - 1) // ff) * (H // 64)
            print("rows %2d (ran %2d, grid %3d) forward  %.3f ms per launch | slot %.2f us = product + cell update %.2f | publish "
                  "%.2f | publish -> next slot start %.2f ; hop: publish(q-1) -> peers' h in(q) %.2f us, poller waits %.2f us "
                  "(%.1f extra passes), h in -> compute start %.2f"
                  % (rows, ff, grid, tf, (c[0][-1] - c[0][0]) / (len(c[0]) - 1), (c[1] - c[0]).mean(), (c[2] - c[1]).mean(),
                     (c[0][1:] - c[2][:-1]).mean(), (c[5][1:] - c[2][:-1]).mean(), (c[5] - c[4]).mean(), (c[6] * 100).mean(),
                     (c[0] - c[5]).mean()))
            tb, fb = timed("bwd", bp, w)
            c = stamps("bwd", bp, w, N, H, 100, 500)
            print("rows %2d (ran %2d, grid %3d) backward %.3f ms per launch | slot %.2f us = wait for the peers' sums %.2f (%.1f extra "
                  "passes) | cell update + image %.2f | barrier %.2f | MFMA %.2f | publish %.2f | -> next slot start %.2f ; hop: "
                  "publish(q-1) -> sums in(q) %.2f us"
                  % (rows, fb, grid, tb, (c[0][-1] - c[0][0]) / (len(c[0]) - 1), (c[4] - c[0]).mean(), (c[6] * 100).mean(),
                     (c[1] - c[4]).mean(), (c[2] - c[1]).mean(), (c[3] - c[2]).mean(), (c[7] - c[3]).mean(),
                     (c[0][1:] - c[7][:-1]).mean(), (c[4][1:] - c[7][:-1]).mean()))
            del os.environ["NS_CLUSTER_ROWS"]
    T = 160
    for N in (32, 1):
        _, fp, _, w = setup(N, T, H, True)
        print("\n## fp32-state forward (three split-bf16 passes), T %d, H %d, N %d" % (T, H, N))
        _, dflt = timed("fwd", fp, w, 1)
        print("default form (no override): %d rows" % dflt)
        for rows in (16, 8, 4):
            os.environ["NS_CLUSTER_ROWS"] = str(rows)
            tf, ff = timed("fwd", fp, w)
            print("rows %2d (ran %2d, grid %3d) forward %.3f ms per launch = %.2f us per step"
                  % (rows, ff, 2 * ((N + ff - 1) // ff) * (H // 32), tf, tf * 1e3 / T))
            del os.environ["NS_CLUSTER_ROWS"]


if __name__ == "__main__":
    main()
