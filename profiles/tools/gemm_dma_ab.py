#!/usr/bin/env python3
"""The k-slow x k-slow weight-gradient product alone, register-staged loop against the direct-to-LDS loop, at the
step's shapes (the method of profiles/tools/gemm_shapes.py: random operands, 30 launches back to back between two HIP
events; here the two loops alternate through NS_GEMM_DMA in one process, ROUNDS times, and the minimum and the median of
the rounds are printed).  Both split-K forms: atomic, and fixed-order with the deterministic scratch.
Usage: python profiles/tools/gemm_dma_ab.py [value ...]       values of NS_GEMM_DMA to alternate: 0 (staged), 1 (direct); default "0 1"
       NS_GEMM_BK32 = 0 / 1 in the environment forces the tile depth for every row.
       NS_AB_SPLITS = "8,16": the first shape only, at these splits (640 and 1280 workgroups: the BK = 32 threshold)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from nspeech_amd import _lib as L  # noqa: E402
from nspeech_amd import ops, profiling  # noqa: E402

# (label, M, N, K, split_k): the splits are the models' (tacotron2.py: about 512 workgroups)
SHAPES = [
    ("postnet conv weight gradient", 2560, 512, 32124, 6),
    ("decoder lstm weight gradient", 1024, 4096, 6432, 2),
    ("decoder lstm 1 input weight gradient", 768, 4096, 6432, 2),
    ("encoder conv weight gradient", 2560, 512, 5244, 6),
    ("head (output projection) weight gradient", 1024, 400, 6432, 12),
]
ROUNDS, REPS = 5, 30


def main():
    variants = sys.argv[1:] or ["0", "1"]
    dev = "cuda:0"
    g = torch.Generator().manual_seed(1)
    lib = L.lib()
    lib.ns_gemm_last_loop.restype = L.C.c_char_p
    shapes = SHAPES
    if os.environ.get("NS_AB_SPLITS"):
        shapes = [SHAPES[0][:4] + (int(x),) for x in os.environ["NS_AB_SPLITS"].split(",")]
    for label, M, N, K, sk in shapes:
        Ad = (torch.randn(K, M, generator=g) * 0.5).to(torch.bfloat16).to(dev)
        Bd = (torch.randn(K, N, generator=g) * 0.5).to(torch.bfloat16).to(dev)
        for det in (False, True):
            ops.DETERMINISTIC_SPLITK = det
            times = {v: [] for v in variants}
            names, outs = {}, {}
            for r in range(ROUNDS):
                for v in variants:
                    os.environ["NS_GEMM_DMA"] = v
                    C = torch.zeros(M, N, device=dev)
                    ops.gemm(Ad, Bd, C, M, N, K, M, N, N, a_mode=1, b_mode=1, split_k=sk, accumulate=2)
                    torch.cuda.synchronize()
                    names[v] = "%s %s" % (profiling._last_kernel()[-9:-1], lib.ns_gemm_last_loop().decode())
                    outs[v] = C.clone()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(REPS):
                        ops.gemm(Ad, Bd, C, M, N, K, M, N, N, a_mode=1, b_mode=1, split_k=sk, accumulate=2)
                    e1.record()
                    torch.cuda.synchronize()
                    times[v].append(e0.elapsed_time(e1) * 1e3 / REPS)
            same = all(torch.equal(outs[v], outs[variants[0]]) for v in variants) if det else None
            row = "  ".join("[%s: %s] min %6.1f med %6.1f us" % (v, names[v], min(times[v]), statistics.median(times[v]))
                            for v in variants)
            print("%-40s %5d x %5d x %6d sk %2d %-6s %s%s" % (label, M, N, K, sk, "fixed" if det else "atomic", row,
                  "  bit-equal" if same else ("  DIFFERENT" if same is False else "")), flush=True)


if __name__ == "__main__":
    main()
