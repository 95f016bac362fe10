"""tests/gemm_ref.py against explicit Python loops: the float64 reference of ns_gemm must not be wrong in the way a
kernel is.  The loops below address every operand as include/nspeech_hip.h words it, one scalar at a time, at
M, N, K <= 5; the reference works on whole index arrays."""
import math

import pytest
import torch

import gemm_ref as R

bf = torch.bfloat16


def _rand(n, seed, dtype=torch.float32, lo=1.0, hi=3.0):
    """n values of magnitude lo .. hi with random signs (a wrong index moves a result by O(1))"""
    g = torch.Generator().manual_seed(seed)
    mag = lo + (hi - lo) * torch.rand(n, generator=g)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    return (mag * sign).to(dtype)


def _act(x, act):
    if act == 1:
        return max(x, 0.0)
    if act == 2:
        return math.tanh(x)
    if act == 3:
        return 1.0 / (1.0 + math.exp(-x))
    if act == 4:
        return x / (1.0 + abs(x))
    return x


def _loops(kw, A, B, Cp, M, N, K, lda, ldb, ldc):
    """the contract, one scalar at a time; returns (C region, mag, col_sum, second sum) as nested lists"""
    g = kw.get
    a_mode, b_mode = g("a_mode", 0), g("b_mode", 0)
    a_off, b_off, c_off = g("a_off", 0), g("b_off", 0), g("c_off", 0)
    alpha = g("alpha", 1.0)
    batch = g("batch", 1)
    sa, sb, sc = g("batch_strides", (0, 0, 0))
    fl = lambda t: None if t is None else [float(x) for x in t.reshape(-1)]
    Af, Bf, Cf = fl(A), fl(B), fl(Cp)
    Al, Bl = fl(g("a_lo")), fl(g("b_lo"))
    bias, addend, gate, sz = fl(g("bias")), fl(g("addend")), fl(g("gate")), fl(g("stat_z"))
    mean, istd = fl(g("stat_mean")), fl(g("stat_istd"))
    out = [[[0.0] * N for _ in range(M)] for _ in range(batch)]
    mag = [[[0.0] * N for _ in range(M)] for _ in range(batch)]
    s1, s2 = [0.0] * N, [0.0] * N
    for z in range(batch):
        for m in range(M):
            valid = True
            if g("row_mask") is not None:
                period, lo, hi, shift = g("row_mask")
                valid = lo <= (m + shift) % period < hi
            for n in range(N):
                acc = absacc = 0.0
                for k in range(K):
                    ia = a_off + z * sa + (m * lda + k if a_mode == 0 else k * lda + m)
                    kb, base = k, b_off + z * sb
                    if g("b_seg") is not None:
                        seg_len, seg_stride = g("b_seg")
                        base += (k // seg_len) * seg_stride
                        kb = k % seg_len
                    ib = base + (n * ldb + kb if b_mode == 0 else kb * ldb + n)
                    a, b = Af[ia], Bf[ib]
                    if Al is not None:
                        a, b = a + Al[ia], b + Bl[ib]
                    acc += a * b
                    absacc += abs(a * b)
                pre = alpha * acc
                mg = abs(alpha) * absacc
                if bias is not None:
                    pre += bias[g("bias_off", 0) + n]
                    mg += abs(bias[g("bias_off", 0) + n])
                if addend is not None:
                    ad = addend[g("addend_off", 0) + m * g("ld_add") + n]
                    pre += ad
                    mg += abs(ad)
                v = _act(pre, g("act", 0))
                if gate is not None and not gate[g("gate_off", 0) + m * g("ld_gate") + n] > 0.0:
                    v = 0.0
                if not valid:
                    v = 0.0
                if g("accumulate", 0):
                    old = Cf[c_off + z * sc + m * ldc + n]
                    v += old
                    mg += abs(old)
                if Cp.dtype == bf:
                    v = float(torch.tensor(v, dtype=torch.float64).to(bf))
                out[z][m][n], mag[z][m][n] = v, mg
                if valid and z == 0:
                    s1[n] += v
                    if sz is not None:
                        s2[n] += v * ((sz[g("stat_z_off", 0) + m * g("ld_stat_z") + n] - mean[n]) * istd[n])
                    else:
                        s2[n] += v * v
    return out, mag, s1, s2


def _check(M, N, K, lda, ldb, ldc, a_len, b_len, c_len, c_dtype=torch.float32, dtype=torch.float32, **kw):
    A, B = _rand(a_len, 1, dtype), _rand(b_len, 2, dtype)
    Cp = _rand(c_len, 3, c_dtype)
    want, wmag, s1, s2 = _loops(kw, A, B, Cp, M, N, K, lda, ldb, ldc)
    stats = dict(col_sum=True, col_sumsq=True)
    got = R.gemm_ref(A, B, Cp, M, N, K, lda, ldb, ldc, **kw, **stats)
    want = torch.tensor(want, dtype=torch.float64)
    # two float64 evaluations in different orders: a few ulps of the magnitudes
    tol = 1e-13 * (1.0 + torch.tensor(wmag, dtype=torch.float64))
    if c_dtype == bf:       # a value a hair from a rounding boundary may land on either neighbour; none does at these seeds
        assert torch.equal(got.C, want)
    assert ((got.C - want).abs() <= tol).all(), (got.C, want)
    assert ((got.mag - torch.tensor(wmag, dtype=torch.float64)).abs() <= tol).all()
    stol = 1e-12 * (1.0 + want[0].abs().sum(0)) * 10.0
    assert ((got.col_sum - torch.tensor(s1, dtype=torch.float64)).abs() <= stol).all()
    assert ((got.col_sumsq - torch.tensor(s2, dtype=torch.float64)).abs() <= stol * 10.0).all()
    return got


@pytest.mark.parametrize("a_mode,b_mode", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("dtype", [torch.float32, bf])
def test_operand_modes_offsets_and_leading_dimensions(a_mode, b_mode, dtype):
    M, N, K = 4, 5, 3
    lda = (K if a_mode == 0 else M) + 2
    ldb = (K if b_mode == 0 else N) + 1
    _check(M, N, K, lda, ldb, N + 3, 64, 64, 64, dtype=dtype, a_mode=a_mode, b_mode=b_mode, a_off=3, b_off=5, c_off=7)


@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
def test_alpha_bias_addend_activation(act):
    for add_dtype in (torch.float32, bf):
        _check(3, 5, 4, 4, 4, 6, 32, 32, 40, act=act, alpha=-0.5, bias=_rand(9, 4), bias_off=2,
               addend=_rand(40, 5, add_dtype), addend_off=3, ld_add=7, c_off=1)


def test_alpha_zero_reads_as_one():
    A, B, Cp = _rand(12, 1), _rand(12, 2), _rand(9, 3)
    a, b = R.gemm_ref(A, B, Cp, 3, 3, 4, 4, 4, 3, alpha=0.0), R.gemm_ref(A, B, Cp, 3, 3, 4, 4, 4, 3, alpha=1.0)
    assert torch.equal(a.C, b.C)


def test_gate_switches_off_non_positive_entries_including_both_zeros():
    gate = _rand(40, 6)
    gate[4], gate[5], gate[11] = 0.0, -0.0, float("nan")
    got = _check(4, 5, 3, 3, 3, 5, 16, 16, 24, gate=gate, gate_off=2, ld_gate=6, act=2, alpha=1.5, c_off=2)
    g = gate[2:].reshape(-1)[:30].reshape(5, 6)[:4, :5]
    assert torch.equal(got.off[0], ~(g > 0))
    assert got.off[0, 0, 2] and got.off[0, 0, 3] and got.off[0, 1, 3]          # +0.0, -0.0, NaN
    assert (got.C[got.off] == 0).all()


@pytest.mark.parametrize("accumulate", [0, 1, 2])
def test_row_mask_and_accumulate(accumulate):
    got = _check(5, 4, 3, 3, 3, 6, 16, 16, 40, row_mask=(3, 1, 3, 2), accumulate=accumulate, c_off=4, bias=_rand(4, 7))
    assert got.valid.tolist() == [lo <= (m + 2) % 3 < hi for m in range(5) for lo, hi in [(1, 3)]]
    assert not got.valid.all() and got.valid.any()


def test_bf16_output_is_rounded_and_statistics_follow_the_stored_values():
    got = _check(5, 4, 5, 5, 5, 4, 32, 32, 24, c_dtype=bf, bias=_rand(4, 8), row_mask=(4, 1, 4, 0))
    assert torch.equal(got.C, got.C.to(bf).double())
    s1, s2, a1, a2 = R.column_stats(got.C[0], got.valid)
    assert torch.equal(s1, got.col_sum) and torch.equal(s2, got.col_sumsq)
    assert torch.equal(a2, s2) and (a1 >= s1.abs()).all()


@pytest.mark.parametrize("z_dtype", [torch.float32, bf])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_stat_z_form(z_dtype, accumulate):
    _check(5, 3, 4, 4, 4, 5, 24, 16, 40, stat_z=_rand(40, 9, z_dtype), ld_stat_z=4, stat_z_off=3,
           stat_mean=_rand(3, 10, lo=0.1, hi=0.5), stat_istd=_rand(3, 11), accumulate=accumulate, c_off=2,
           row_mask=(4, 1, 3, 1))


def test_batch_strides():
    _check(3, 4, 5, 5, 5, 4, 80, 90, 70, batch=3, batch_strides=(22, 27, 19), accumulate=2, a_off=1, b_off=2, c_off=3)


def test_pre_split_operands_are_the_sums():
    lo_a, lo_b = _rand(16, 12, bf, 2.0 ** -9, 2.0 ** -8), _rand(16, 13, bf, 2.0 ** -9, 2.0 ** -8)
    _check(3, 4, 4, 4, 4, 4, 16, 16, 12, dtype=bf, a_lo=lo_a, b_lo=lo_b)


def test_segmented_b_walk_in_loops():
    # two segments of 2, walked backwards
    _check(3, 4, 4, 5, 2, 4, 32, 40, 12, b_seg=(2, -8), b_off=8)
    _check(3, 4, 4, 5, 4, 4, 32, 40, 12, b_seg=(2, -12), b_off=12, b_mode=1)


def test_segmented_b_walk_is_the_three_tap_sum():
    """the conv data-gradient pattern as tests/test_gemm_gpu.py writes it out: taps walked backwards through segments"""
    taps, Cin, Cout, Mr = 3, 4, 5, 5
    W = _rand(taps * Cin * Cout, 14).reshape(taps, Cin, Cout)
    dY = _rand((Mr + taps - 1) * Cout, 15).reshape(Mr + taps - 1, Cout)
    dX = torch.zeros(Mr, Cin)
    got = R.gemm_ref(dY, W, dX, Mr, Cin, taps * Cout, Cout, Cout, Cin, a_mode=0, b_mode=0,
                     b_off=(taps - 1) * Cin * Cout, b_seg=(Cout, -Cin * Cout))
    dy, w = dY.double(), W.double()
    ref = torch.zeros(Mr, Cin, dtype=torch.float64)
    for j in range(taps):
        ref += dy[j:j + Mr] @ w[taps - 1 - j].t()
    assert (got.C[0] - ref).abs().max().item() <= 1e-12


def test_cache_holds_the_products_only():
    A, B, Cp = _rand(20, 1), _rand(20, 2), _rand(16, 3)
    cache = {}
    a = R.gemm_ref(A, B, Cp, 4, 4, 5, 5, 5, 4, cache=cache)
    b = R.gemm_ref(A, B, Cp, 4, 4, 5, 5, 5, 4, cache=cache, bias=_rand(4, 4), act=2)
    c = R.gemm_ref(A, B, Cp, 4, 4, 5, 5, 5, 4, bias=_rand(4, 4), act=2)
    assert set(cache) == {"prod", "absprod"} and torch.equal(b.C, c.C) and not torch.equal(a.C, b.C)
