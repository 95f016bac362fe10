"""ns_gemm_group against the same items launched one by one through ns_gemm / ns_colsum, into a copy of the same C.

Items: the smallest shapes that still cross every boundary of the three bodies - more than one tile in both directions
with ragged edges, more k tiles than slices and a short last slice, an overlapping im2col view (lda < M), the LSTM
pairing (B one row down, K - 1 rows), the fp32 one-pass product, column sums of both dtypes with a ragged last block of
quads and a ragged last quad, an empty item.  All outputs lie side by side in one flat buffer between guard bands.

Fixed-order mode (deterministic split-K scratch, column-sum work buffers): the whole buffer, guard bands included, is
bit-equal to the single launches', three times over, and every arrival counter is zero afterwards.
Atomic mode: every element against the float64 contract of tests/gemm_ref.py with the per-element bound that
tests/test_gemm_epilogue_gpu.py holds the single launches to (u = 2^-24): exact bf16 products 2 (K + 4) u mag, the
one-pass fp32 product 2e-2 max|A| max|B| sqrt(K), plus the fp32 store's 2^-23 |ref|; column sums 2 (rows + 4) u
sum|terms|, the fp32 summation bound of any order doubled, plus the store."""
import ctypes
import math

import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu

bf, f32 = torch.bfloat16, torch.float32
U = 2.0 ** -24
GUARD = 256


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _uniform(n, seed, dtype):
    return (torch.rand(n, generator=_gen(seed)) * 2.0 - 1.0).to(dtype)


# (name, kind, dtype, M, N, K, lda, a_off, b_off, split_k); A is [K rows x lda] (k-slow), B is [K rows x N]
PRODUCTS = [
    ("bf16", "p", bf, 136, 264, 520, 136, 0, 0, 3),
    ("im2col", "p", bf, 80, 136, 300, 16, 0, 0, 2),            # cin 16, width 5: row k of A starts 16 elements on
    ("lstm_pair", "p", bf, 136, 264, 519, 136, 0, 264, 2),     # h(row - 1) against dgates(row): B one row down, K - 1 rows
    ("f32", "p", f32, 80, 256, 388, 80, 0, 0, 3),
    ("empty", "p", bf, 136, 0, 520, 136, 0, 0, 1),
]
# (name, dtype, rows, C, ld)
SUMS = [("sum_bf16", bf, 520, 264, 264), ("sum_f32", f32, 300, 100, 104), ("sum_ragged_quad", f32, 300, 102, 104)]


class Case:
    """Operands on the host and the device, the layout of the flat output buffer, the scratch."""

    def __init__(self, dev, names):
        self.dev = dev
        self.products = [p for p in PRODUCTS if p[0] in names]
        self.sums = [s for s in SUMS if s[0] in names]
        self.A, self.B, self.X, self.off = {}, {}, {}, {}
        pos = GUARD
        for i, (name, _, dt, M, N, K, lda, a_off, b_off, sk) in enumerate(self.products):
            self.A[name] = _uniform(a_off + (K - 1) * lda + M + 8, 11 + i, dt)
            self.B[name] = _uniform(b_off + K * max(N, 8) + 8, 31 + i, dt)
            self.off[name] = pos
            pos += M * N
        for i, (name, dt, rows, C, ld) in enumerate(self.sums):
            self.X[name] = _uniform(rows * ld, 51 + i, dt)
            self.off[name] = pos
            pos += C
        self.total = pos + GUARD
        self.prior = _uniform(self.total, 7, f32)
        self.dA = {k: v.to(dev) for k, v in self.A.items()}
        self.dB = {k: v.to(dev) for k, v in self.B.items()}
        self.dX = {k: v.to(dev) for k, v in self.X.items()}

    def params(self, flat, det, scratch):
        """(ns_gemm_params list, ns_colsum_params list) writing into `flat`; det: with the fixed-order scratch"""
        from nspeech_amd import _lib
        lib = _lib.lib()
        lib.ns_gemm_splitk_work_bytes.restype = lib.ns_gemm_splitk_counters.restype = ctypes.c_size_t
        lib.ns_colsum_work_floats.restype = ctypes.c_size_t
        work, count, swork = scratch
        wo = co = so = 0
        ps, ss = [], []
        for name, _, dt, M, N, K, lda, a_off, b_off, sk in self.products:
            p = _lib.struct("ns_gemm_params")
            es = 2 if dt == bf else 4
            p.dtype, p.M, p.N, p.K = (_lib.NS_BF16 if dt == bf else _lib.NS_F32), M, N, K
            p.A, p.lda, p.a_mode = self.dA[name].data_ptr() + a_off * es, lda, 1
            p.B, p.ldb, p.b_mode = self.dB[name].data_ptr() + b_off * es, max(N, 8), 1
            p.C, p.ldc, p.c_dtype = flat.data_ptr() + 4 * self.off[name], max(N, 1), _lib.NS_F32
            p.accumulate, p.split_k, p.alpha, p.f32_passes = 2, sk, 1.0, 1
            if det and sk > 1:
                p.splitk_work, p.splitk_count = work.data_ptr() + wo, count.data_ptr() + 4 * co
                wo += lib.ns_gemm_splitk_work_bytes(M, N, sk)
                co += lib.ns_gemm_splitk_counters(M, N)
            ps.append(p)
        for name, dt, rows, C, ld in self.sums:
            p = _lib.struct("ns_colsum_params")
            p.x, p.dtype, p.ld, p.rows, p.C = self.dX[name].data_ptr(), (_lib.NS_BF16 if dt == bf else _lib.NS_F32), ld, rows, C
            p.out = flat.data_ptr() + 4 * self.off[name]
            if det:
                p.work = swork.data_ptr() + 4 * so
                so += lib.ns_colsum_work_floats(C)
            ss.append(p)
        assert wo <= work.numel() * 4 and co <= count.numel() and so <= swork.numel()
        return ps, ss

    def scratch(self):
        return (torch.empty(4 << 20, dtype=f32, device=self.dev), torch.zeros(4096, dtype=torch.int32, device=self.dev),
                torch.zeros(1 << 18, dtype=f32, device=self.dev))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _single(case, det, scratch):
    from nspeech_amd import _lib
    lib = _lib.lib()
    flat = case.prior.to(case.dev)
    ps, ss = case.params(flat, det, scratch)
    for p in ps:
        _lib.check(lib.ns_gemm(ctypes.byref(p), _stream()), "ns_gemm")
    for p in ss:
        _lib.check(lib.ns_colsum(ctypes.byref(p), _stream()), "ns_colsum")
    torch.cuda.synchronize()
    return flat


def _grouped(case, det, scratch):
    from nspeech_amd import _lib
    lib = _lib.lib()
    lib.ns_gemm_last_kernel.restype = ctypes.c_char_p
    flat = case.prior.to(case.dev)
    ps, ss = case.params(flat, det, scratch)
    ap = (_lib.STRUCTS["ns_gemm_params"] * len(ps))(*ps) if ps else None
    asum = (_lib.STRUCTS["ns_colsum_params"] * len(ss))(*ss) if ss else None
    _lib.check(lib.ns_gemm_group(ap, len(ps), asum, len(ss), _stream()), "ns_gemm_group")
    assert lib.ns_gemm_last_kernel() == b"gemm_group_kernel"
    torch.cuda.synchronize()
    return flat


ALL = tuple(p[0] for p in PRODUCTS) + tuple(s[0] for s in SUMS)
_CASES = {}


def _case(dev, names):
    if names not in _CASES:
        _CASES[names] = Case(dev, names)
    return _CASES[names]


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("names", [ALL, ("bf16",), ("sum_f32",), ("f32", "sum_bf16")], ids=["all", "one_product", "one_sum", "pair"])
def test_fixed_order_group_is_bit_equal_to_single_launches(dev, names):
    case = _case(dev, names)
    want = _single(case, True, case.scratch())
    assert not torch.equal(want, case.prior.to(dev))
    scratch = case.scratch()
    for rep in range(3):                                   # the counters of one run are the next one's zeroed counters
        got = _grouped(case, True, scratch)
        diff = (_bits(got) != _bits(want)).nonzero().flatten()
        assert diff.numel() == 0, "run %d: %d words differ from the single launches, first at %d (layout %r)" % (
            rep, diff.numel(), int(diff[0]), case.off)
    assert int(scratch[1].abs().sum()) == 0, "split-K tile counters left non-zero"
    lib = __import__("nspeech_amd")._lib.lib()
    lib.ns_colsum_work_floats.restype = ctypes.c_size_t
    so = 0
    for name, dt, rows, C, ld in case.sums:                # every column sum's own counters, wherever its slot starts
        assert int(_bits(scratch[2])[so:so + 1024].abs().sum()) == 0, name
        so += lib.ns_colsum_work_floats(C)


def test_atomic_group_meets_the_float64_contract(dev):
    case = _case(dev, ALL)
    got = _grouped(case, False, case.scratch()).cpu().double()
    prior = case.prior.double()
    worst = 0.0
    for name, _, dt, M, N, K, lda, a_off, b_off, sk in case.products:
        if M * N == 0:
            continue
        ref = R.gemm_ref(case.A[name], case.B[name], case.prior, M, N, K, lda, N, N, a_mode=1, b_mode=1, a_off=a_off,
                         b_off=b_off, c_off=case.off[name], accumulate=2, split_k=sk)
        if dt == bf:
            acc = 2.0 * (K + 4) * U * ref.mag[0]
        else:
            maxA = R.operand_a(case.A[name], M, K, lda, 1, a_off).abs().max().item()
            maxB = R.operand_b(case.B[name], K, N, N, 1, b_off).abs().max().item()
            acc = torch.full_like(ref.mag[0], 2e-2 * maxA * maxB * math.sqrt(K))
        bound = acc + 2.0 ** -23 * ref.exact[0].abs()
        err = (got[case.off[name]:case.off[name] + M * N].reshape(M, N) - ref.C[0]).abs()
        ratio = float((err / bound).max())
        print("%s: worst err / bound %.3g" % (name, ratio))
        assert ratio <= 1.0, (name, ratio)
        worst = max(worst, ratio)
    for name, dt, rows, C, ld in case.sums:
        x = case.X[name].double().reshape(rows, ld)[:, :C]
        o = case.off[name]
        ref = x.sum(0) + prior[o:o + C]
        bound = 2.0 * (rows + 4) * U * (x.abs().sum(0) + prior[o:o + C].abs()) + 2.0 ** -23 * ref.abs()
        ratio = float(((got[o:o + C] - ref).abs() / bound).max())
        print("%s: worst err / bound %.3g" % (name, ratio))
        assert ratio <= 1.0, (name, ratio)
    # what no item owns comes back bit for bit
    owned = torch.zeros(case.total, dtype=torch.bool)
    for name, _, dt, M, N, K, lda, a_off, b_off, sk in case.products:
        owned[case.off[name]:case.off[name] + M * N] = True
    for name, dt, rows, C, ld in case.sums:
        owned[case.off[name]:case.off[name] + C] = True
    assert torch.equal(got[~owned], prior[~owned])


def test_recording_context_launches_one_group(dev):
    """ops.gemm_group: the accepted calls go out as one launch with scratch of the context's own, a refused product and
    a cast run at once, and the result is the single launches'."""
    from nspeech_amd import _lib, ops
    case = _case(dev, ALL)
    lib = _lib.lib()
    lib.ns_gemm_last_kernel.restype = ctypes.c_char_p
    keep = ops.DETERMINISTIC_SPLITK
    ops.DETERMINISTIC_SPLITK = True
    try:
        def run(flat, extra):
            for name, _, dt, M, N, K, lda, a_off, b_off, sk in case.products:
                ops.gemm(case.dA[name], case.dB[name], flat, M, N, K, lda, max(N, 8), max(N, 1), a_mode=1, b_mode=1, a_off=a_off,
                         b_off=b_off, c_off=case.off[name], accumulate=2, split_k=sk, f32_passes=1)
            # k-contiguous A: another kernel form, the plan refuses it and it runs at once
            ops.gemm(case.dA["bf16"], case.dB["bf16"], extra, 8, 264, 136, 136, 264, 264, a_mode=0, b_mode=1,
                     accumulate=2, f32_passes=1)
            for name, dt, rows, C, ld in case.sums:
                ops.colsum(case.dX[name], ld, rows, C, flat, out_off=case.off[name])
            return flat, extra
        want, want_x = run(case.prior.to(dev), torch.zeros(8 * 264, device=dev))
        got, got_x = case.prior.to(dev), torch.zeros(8 * 264, device=dev)
        with ops.gemm_group() as grp:
            run(got, got_x)
            assert lib.ns_gemm_last_kernel() == b"gemm_mfma_kernel<0, 1, false, 64, 128>"      # the refused one, at once
        torch.cuda.synchronize()
        assert lib.ns_gemm_last_kernel() == b"gemm_group_kernel"
        assert grp.launches == [7]                     # 4 products and 3 sums with an output; the empty one launches nothing
        assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(got_x), _bits(want_x))
        assert float(got_x.abs().max()) > 0
    finally:
        ops.DETERMINISTIC_SPLITK = keep
