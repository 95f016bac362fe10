"""The direct-to-LDS K loop of the k-slow x k-slow 128-tile bf16 product (gemm_mfma_dma_body) against the register-staged
loop it replaces, through the per-call switch NS_GEMM_DMA = 0.

Both loops put the same operand tiles into the same LDS images and issue the same MFMAs in the same order, so with a
fixed summation order - one K slice, or the deterministic split-K scratch - C must be bit-equal (torch.equal), guard
bands included.  Cases: the smallest shapes at which the loop takes another path - one tile with one K-tile; a ragged
last K-tile (K = 63, 65, 64 * 3 + 8) and a K shorter than anything (K = 1); ragged tile edges in M and N; an empty K
slice (split 3 over two K-tiles) and a split with a short last slice (6 over 13 K-tiles); B one row down with K = rows - 1
(the LSTM pairing); an overlapping 5-tap im2col view (lda = 64, M = 320), where a linear range cannot tell row K from
row K - 1; both tile depths, forced.  K-tile counts are given for BK = 64; at BK = 32 the same shapes have twice the
K-tiles and the same edges.

Atomic split-K adds the slices in arrival order: each loop is held to the float64 contract of tests/gemm_ref.py under
the bound tests/test_gemm_epilogue_gpu.py uses for this kernel (u = 2^-24): 2 (K + 4) u mag + 2^-23 |ref|.

A leading dimension that is no multiple of 8 elements allows no 16-byte chunks: ns_gemm sends it where it sent it before
(ns_gemm_last_kernel and ns_gemm_last_loop say so).  A grouped launch of two items runs the same body.
"""
import ctypes
import os

import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu

bf, f32 = torch.bfloat16, torch.float32
U = 2.0 ** -24
GUARD = 64

# name: (M, N, K, lda, ldb, a_off, b_off, split_k)
CASES = {
    "one_tile": (128, 128, 64, 128, 128, 0, 0, 1),
    "k1": (128, 128, 1, 128, 128, 0, 0, 1),
    "k63": (128, 128, 63, 128, 128, 0, 0, 1),
    "k65": (128, 128, 65, 128, 128, 0, 0, 1),
    "k200": (128, 128, 64 * 3 + 8, 128, 128, 0, 0, 1),
    "ragged_mn": (136, 264, 200, 136, 264, 0, 0, 1),
    "empty_slice": (136, 264, 128, 136, 264, 0, 0, 3),
    "split6_13": (136, 264, 64 * 12 + 40, 144, 272, 8, 16, 6),
    "lstm_pair": (136, 264, 199, 136, 264, 0, 264, 2),          # B one row down, K = rows - 1
    "im2col": (320, 136, 100, 64, 136, 0, 0, 2),                # cin 64, width 5: ~100 padded rows
}
_DATA = {}


def _uniform(n, seed):
    return (torch.rand(n, generator=torch.Generator().manual_seed(seed)) * 2.0 - 1.0).to(bf)


def _data(dev, name):
    if name not in _DATA:
        M, N, K, lda, ldb, a_off, b_off, sk = CASES[name]
        i = list(CASES).index(name)
        A = _uniform(a_off + (K - 1) * lda + M + 8, 100 + i)
        B = _uniform(b_off + (K - 1) * ldb + N + 8, 200 + i)
        prior = _uniform(M * (N + 3) + 2 * GUARD, 300 + i).to(f32)
        _DATA[name] = (A, B, prior, A.to(dev), B.to(dev))
    return _DATA[name]


def _lib():
    from nspeech_amd import _lib
    lib = _lib.lib()
    lib.ns_gemm_last_kernel.restype = lib.ns_gemm_last_loop.restype = ctypes.c_char_p
    lib.ns_gemm_splitk_work_bytes.restype = lib.ns_gemm_splitk_counters.restype = ctypes.c_size_t
    return _lib, lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _params(dev, name, flat, det, scratch):
    L, lib = _lib()
    M, N, K, lda, ldb, a_off, b_off, sk = CASES[name]
    _, _, _, dA, dB = _data(dev, name)
    p = L.struct("ns_gemm_params")
    p.dtype, p.M, p.N, p.K = L.NS_BF16, M, N, K
    p.A, p.lda, p.a_mode = dA.data_ptr() + 2 * a_off, lda, 1
    p.B, p.ldb, p.b_mode = dB.data_ptr() + 2 * b_off, ldb, 1
    p.C, p.ldc, p.c_dtype = flat.data_ptr() + 4 * GUARD, N + 3, L.NS_F32      # c_off = GUARD, an odd leading dimension
    p.accumulate, p.split_k, p.alpha, p.f32_passes = 2, sk, 1.0, 1
    if det and sk > 1:
        work, count = scratch
        assert lib.ns_gemm_splitk_work_bytes(M, N, sk) <= work.numel() * 4 and lib.ns_gemm_splitk_counters(M, N) <= count.numel()
        p.splitk_work, p.splitk_count = work.data_ptr(), count.data_ptr()
    return p


def _scratch(dev):
    return torch.empty(2 << 20, dtype=f32, device=dev), torch.zeros(256, dtype=torch.int32, device=dev)


def _run(dev, monkeypatch, name, loop, det, bk32):
    """C (guards included) of one ns_gemm call on the given loop and tile depth; asserts that this loop ran."""
    L, lib = _lib()
    if loop == "staged":
        monkeypatch.setenv("NS_GEMM_DMA", "0")
    else:
        monkeypatch.delenv("NS_GEMM_DMA", raising=False)
    monkeypatch.setenv("NS_GEMM_BK32", "1" if bk32 else "0")
    flat = _data(dev, name)[2].to(dev)
    scratch = _scratch(dev)
    p = _params(dev, name, flat, det, scratch)
    L.check(lib.ns_gemm(ctypes.byref(p), _stream()), "ns_gemm")
    torch.cuda.synchronize()
    assert lib.ns_gemm_last_kernel() == (b"gemm_mfma_kernel<1, 1, false, 32, 128>" if bk32 else b"gemm_mfma_kernel<1, 1, false, 64, 128>")
    assert lib.ns_gemm_last_loop() == loop.encode()
    if det and CASES[name][7] > 1:
        assert int(scratch[1].abs().sum().item()) == 0          # every arrival counter left clean
    return flat.cpu()


@pytest.mark.parametrize("bk32", [False, True], ids=["bk64", "bk32"])
@pytest.mark.parametrize("name", list(CASES))
def test_fixed_order_is_bit_equal_to_the_staged_loop(dev, monkeypatch, name, bk32):
    want = _run(dev, monkeypatch, name, "staged", True, bk32)
    got = _run(dev, monkeypatch, name, "dma", True, bk32)
    assert torch.equal(got, want), (got - want).abs().max().item()
    prior = _data(dev, name)[2]
    assert torch.equal(got[:GUARD], prior[:GUARD]) and torch.equal(got[-GUARD:], prior[-GUARD:])
    assert not torch.equal(got, prior)


@pytest.mark.parametrize("bk32", [False, True], ids=["bk64", "bk32"])
@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][7] > 1])
def test_atomic_split_k_meets_the_float64_contract(dev, monkeypatch, name, bk32):
    M, N, K, lda, ldb, a_off, b_off, sk = CASES[name]
    A, B, prior, _, _ = _data(dev, name)
    ref = R.gemm_ref(A, B, prior, M, N, K, lda, ldb, N + 3, a_mode=1, b_mode=1, a_off=a_off, b_off=b_off, c_off=GUARD,
                     accumulate=2)
    exact, mag = ref.exact[0], ref.mag[0]
    bound = 2.0 * (K + 4) * U * mag + 2.0 ** -23 * exact.abs()
    idx = GUARD + torch.arange(M)[:, None] * (N + 3) + torch.arange(N)[None, :]
    for loop in ("staged", "dma"):
        got = _run(dev, monkeypatch, name, loop, False, bk32)
        err = (got.double()[idx] - exact).abs()
        worst = (err / bound).max().item()
        print(name, "bk32" if bk32 else "bk64", loop, "worst err / bound %.3f" % worst)
        assert worst <= 1.0, (loop, worst)
        rest = torch.ones(got.numel(), dtype=torch.bool)
        rest[idx.reshape(-1)] = False
        assert torch.equal(got[rest], prior[rest])              # nothing outside the M x N region moves


def test_unaligned_leading_dimension_keeps_its_kernel(dev, monkeypatch):
    """lda = 132 + 2: rows start at 4-byte boundaries, no 16-byte chunks; the same kernel and loop with and without the switch."""
    from nspeech_amd import ops
    L, lib = _lib()
    M, N, K, lda = 136, 264, 200, 138
    A, B = _uniform(K * lda, 1).to(dev), _uniform(K * N, 2).to(dev)
    out = {}
    for loop in ("staged", "dma"):
        if loop == "staged":
            monkeypatch.setenv("NS_GEMM_DMA", "0")
        else:
            monkeypatch.delenv("NS_GEMM_DMA", raising=False)
        Cm = torch.zeros(M, N, dtype=f32, device=dev)
        ops.gemm(A, B, Cm, M, N, K, lda, N, N, a_mode=1, b_mode=1)
        torch.cuda.synchronize()
        assert lib.ns_gemm_last_kernel() == b"gemm_generic_kernel"
        assert lib.ns_gemm_last_loop() == b"staged"
        out[loop] = Cm.cpu()
    assert torch.equal(out["dma"], out["staged"])
    ref = A.double().cpu().reshape(K, lda)[:, :M].t() @ B.double().cpu().reshape(K, N)
    assert (out["dma"].double() - ref).abs().max().item() <= 2.0 * (K + 4) * U * K + 2.0 ** -23 * ref.abs().max().item()


def test_grouped_launch_of_two_items_is_bit_equal(dev, monkeypatch):
    L, lib = _lib()
    names = ("split6_13", "im2col")
    out = {}
    for loop in ("staged", "dma"):
        if loop == "staged":
            monkeypatch.setenv("NS_GEMM_DMA", "0")
        else:
            monkeypatch.delenv("NS_GEMM_DMA", raising=False)
        monkeypatch.setenv("NS_GEMM_BK32", "0")
        flats = [_data(dev, n)[2].to(dev) for n in names]
        scratch = [_scratch(dev) for _ in names]
        ps = [_params(dev, n, f, True, s) for n, f, s in zip(names, flats, scratch)]
        arr = (L.STRUCTS["ns_gemm_params"] * len(ps))(*ps)
        L.check(lib.ns_gemm_group(arr, len(ps), None, 0, _stream()), "ns_gemm_group")
        torch.cuda.synchronize()
        assert lib.ns_gemm_last_kernel() == b"gemm_group_kernel"
        assert lib.ns_gemm_last_loop() == loop.encode()
        out[loop] = [f.cpu() for f in flats]
    for n, a, b in zip(names, out["dma"], out["staged"]):
        assert torch.equal(a, b), n
        assert torch.equal(a, _run(dev, monkeypatch, n, "dma", True, False)), n     # and to the item launched alone


# (form of tests/test_gemm_epilogue_gpu.py at its smallest shape: dtype, M, N, K, a_mode, b_mode, f32_passes, element offset of A)
PLANNED = {
    "skinny": (bf, 17, 72, 104, 0, 0, 0, 0),
    "generic": (bf, 70, 67, 45, 0, 0, 0, 3),
    "half_tiles": (bf, 130, 136, 72, 0, 0, 0, 0),
    "dma": (bf, 136, 136, 100, 1, 1, 0, 0),
    "three_passes": (f32, 136, 136, 100, 1, 0, 3, 0),
}


@pytest.mark.parametrize("name", list(PLANNED))
def test_the_launch_is_what_the_plan_said(dev, monkeypatch, name):
    """ns_gemm_plan and ns_gemm on one block: the query names the kernel and the loop that the launch then reports"""
    L, lib = _lib()
    monkeypatch.delenv("NS_GEMM_DMA", raising=False)
    monkeypatch.delenv("NS_GEMM_BK32", raising=False)
    dtype, M, N, K, a_mode, b_mode, passes, a_off = PLANNED[name]
    g = torch.Generator().manual_seed(7)
    A = (torch.rand(a_off + M * K, generator=g) - 0.5).to(dtype).to(dev)
    B = (torch.rand(K * N, generator=g) - 0.5).to(dtype).to(dev)
    Cm = torch.zeros(M * N, dtype=f32, device=dev)
    p = L.struct("ns_gemm_params")
    p.dtype, p.M, p.N, p.K = (L.NS_BF16 if dtype == bf else L.NS_F32), M, N, K
    p.A, p.lda, p.a_mode = A.data_ptr() + a_off * A.element_size(), (K if a_mode == 0 else M), a_mode
    p.B, p.ldb, p.b_mode = B.data_ptr(), (K if b_mode == 0 else N), b_mode
    p.C, p.ldc, p.c_dtype = Cm.data_ptr(), N, L.NS_F32
    p.alpha, p.f32_passes = 1.0, passes
    info = L.struct("ns_gemm_plan_info")
    L.check(lib.ns_gemm_plan(ctypes.byref(p), ctypes.byref(info)), "ns_gemm_plan")
    said = (ctypes.cast(info.kernel, ctypes.c_char_p).value, ctypes.cast(info.loop, ctypes.c_char_p).value)
    L.check(lib.ns_gemm(ctypes.byref(p), _stream()), "ns_gemm")
    torch.cuda.synchronize()
    assert (lib.ns_gemm_last_kernel(), lib.ns_gemm_last_loop()) == said
    want = {"skinny": b"gemm_skinny_kernel<1>", "generic": b"gemm_generic_kernel", "half_tiles": b"gemm_mfma_kernel<0, 0, true, 64, 64>",
            "dma": b"gemm_mfma_kernel<1, 1, true, 64, 128>", "three_passes": b"gemm_mfma_f32_kernel<1, 0, 3, true, 128>"}[name]
    assert said == (want, b"dma" if name == "dma" else b"staged")
    a = A[a_off:].double().cpu().reshape((M, K) if a_mode == 0 else (K, M))
    b = B.double().cpu().reshape((N, K) if b_mode == 0 else (K, N))
    ref = (a if a_mode == 0 else a.t()) @ (b.t() if b_mode == 0 else b)
    # the bounds of tests/test_gemm_epilogue_gpu.py: exact products 2 (K + 4) u mag, three passes 3e-5 max|A| max|B| sqrt(K)
    acc = 3e-5 * a.abs().max() * b.abs().max() * K ** 0.5 if passes == 3 else 2.0 * (K + 4) * U * (
        (a.abs() if a_mode == 0 else a.abs().t()) @ (b.abs().t() if b_mode == 0 else b.abs()))
    assert bool(((Cm.double().cpu().reshape(M, N) - ref).abs() <= acc + 2.0 ** -23 * ref.abs()).all())
