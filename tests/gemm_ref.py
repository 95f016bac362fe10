"""The ns_gemm contract (include/nspeech_hip.h) restated in float64 on the CPU.

gemm_ref() takes the arguments of ops.gemm with CPU tensors in place of device tensors and computes, from the operands
AS STORED (bf16 and fp32 convert to float64 exactly), what the call has to leave in C.  Every operand is addressed the
way the header words it - a flat buffer, an element offset, a leading dimension - through index arithmetic on whole
index arrays; no kernel's tiling, summation order or epilogue code is mirrored here.  tests/test_gemm_ref_cpu.py holds
this module against explicit Python loops.
"""
from types import SimpleNamespace

import torch

ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID, ACT_SOFTSIGN = 0, 1, 2, 3, 4


def _flat64(t):
    return t.detach().cpu().reshape(-1).double()


def _take(t, idx):
    return _flat64(t)[idx.reshape(-1)].reshape(idx.shape)


def _mn(M, N, ld, off):
    """element index of (m, n) in an [M, N] operand with leading dimension ld, first element at off"""
    return off + torch.arange(M)[:, None] * ld + torch.arange(N)[None, :]


def operand_a(A, M, K, lda, a_mode, a_off=0):
    m, k = torch.arange(M)[:, None], torch.arange(K)[None, :]
    return _take(A, a_off + (m * lda + k if a_mode == 0 else k * lda + m))


def operand_b(B, K, N, ldb, b_mode, b_off=0, b_seg=None):
    """B(k, n) as [K, N]; with b_seg = (len, stride) segment s = k // len of the K range starts at B + s * stride"""
    k, n = torch.arange(K)[:, None], torch.arange(N)[None, :]
    base = torch.zeros_like(k)
    if b_seg is not None and b_seg[0] > 0:
        s = k // b_seg[0]
        base, k = s * b_seg[1], k - s * b_seg[0]
    return _take(B, b_off + base + (n * ldb + k if b_mode == 0 else k * ldb + n))


def activation(x, act):
    if act == ACT_NONE:
        return x
    if act == ACT_RELU:
        return torch.clamp(x, min=0.0)
    if act == ACT_TANH:
        return torch.tanh(x)
    if act == ACT_SIGMOID:
        return torch.sigmoid(x)
    if act == ACT_SOFTSIGN:
        return x / (1.0 + x.abs())
    raise ValueError("act %r" % (act,))


def valid_rows(M, row_mask):
    """bool [M]: rows the mask keeps; a row is written as 0 unless lo <= (m + shift) % period < hi"""
    if row_mask is None or row_mask[0] <= 0:
        return torch.ones(M, dtype=torch.bool)
    period, lo, hi, shift = row_mask
    t = (torch.arange(M) + shift) % period
    return (t >= lo) & (t < hi)


def column_stats(Cv, valid, stat_z=None, stat_mean=None, stat_istd=None):
    """Column statistics of a stored [M, N] float64 C over the rows `valid`: (sum, second, sum |terms|, second |terms|).
    second = sum of squares, or with stat_z ([M, N] float64) sum C * (z - mean) * istd."""
    v = valid.double()[:, None]
    t1 = Cv * v
    t2 = (Cv * Cv if stat_z is None else Cv * ((stat_z - stat_mean[None, :]) * stat_istd[None, :])) * v
    return t1.sum(0), t2.sum(0), t1.abs().sum(0), t2.abs().sum(0)


def gemm_ref(A, B, C_prior, M, N, K, lda, ldb, ldc, a_mode=0, b_mode=0, a_off=0, b_off=0, c_off=0,
             bias=None, bias_off=0, act=0, alpha=1.0, accumulate=0, row_mask=None, col_sum=False,
             col_sumsq=False, split_k=1, b_seg=None, addend=None, addend_off=0, ld_add=0, f32_passes=None,
             gate=None, gate_off=0, ld_gate=0, a_lo=None, b_lo=None, batch=1, batch_strides=(0, 0, 0),
             stat_z=None, ld_stat_z=0, stat_mean=None, stat_istd=None, stat_z_off=0, cache=None):
    """What ops.gemm with the same arguments leaves behind.  A, B, C_prior, bias, addend, gate, stat_z, a_lo, b_lo: CPU
    tensors holding the same buffers as the call's device tensors (C_prior: C before the call; its dtype is C's).
    col_sum / col_sumsq: truthy where the call passes a tensor.  split_k and f32_passes do not change the contract.
    a_lo / b_lo: the operands are the sums hi + lo (what the three-segment product approximates).
    cache: an optional dict that keeps the two K-long sums between calls ON THE SAME OPERANDS.

    Returns a namespace of float64 tensors, [batch, M, N] unless noted:
      C        the region of C after the call (rounded to bf16 where C is bf16)
      exact    the same before that rounding: what an error bound with a store term is measured from (a kernel's fp32
               value a hair on the other side of a rounding boundary lands one bf16 step from C, legitimately)
      mag      |alpha| * (|A|.|B|) + |bias| + |addend| + |C_prior| (the last with accumulate only)
      absprod  (|A|.|B|)
      off      bool: elements the row mask or the gate switches off (C keeps its prior value there, or is 0)
      valid    bool [M]
      col_sum, col_sumsq   [N] or None, over the unmasked rows of C as stored (col_sumsq: the stat_z form with stat_z)
    """
    if alpha == 0.0:
        alpha = 1.0
    sa, sb, sc = batch_strides if batch > 1 else (0, 0, 0)
    if cache is not None and "prod" in cache:
        prod, absprod = cache["prod"], cache["absprod"]
    else:
        prods, absprods = [], []
        for z in range(batch):
            a = operand_a(A, M, K, lda, a_mode, a_off + z * sa)
            b = operand_b(B, K, N, ldb, b_mode, b_off + z * sb, b_seg)
            if a_lo is not None:
                a = a + operand_a(a_lo, M, K, lda, a_mode, a_off + z * sa)
                b = b + operand_b(b_lo, K, N, ldb, b_mode, b_off + z * sb, b_seg)
            prods.append(a @ b)
            absprods.append(a.abs() @ b.abs())
        prod, absprod = torch.stack(prods), torch.stack(absprods)
        if cache is not None:
            cache["prod"], cache["absprod"] = prod, absprod
    pre = alpha * prod
    mag = abs(alpha) * absprod
    if bias is not None:
        bv = _flat64(bias)[bias_off:bias_off + N]
        pre = pre + bv
        mag = mag + bv.abs()
    if addend is not None:
        av = _take(addend, _mn(M, N, ld_add, addend_off))
        pre = pre + av
        mag = mag + av.abs()
    v = activation(pre, act)
    valid = valid_rows(M, row_mask)
    off = (~valid)[None, :, None].expand(batch, M, N).clone()
    if gate is not None:
        off |= ~(_take(gate, _mn(M, N, ld_gate, gate_off)) > 0.0)
    v = torch.where(off, torch.zeros_like(v), v)
    if accumulate:
        prior = torch.stack([_take(C_prior, _mn(M, N, ldc, c_off + z * sc)) for z in range(batch)])
        v = v + prior
        mag = mag + prior.abs()
    exact = v
    if C_prior.dtype == torch.bfloat16:
        v = v.to(torch.bfloat16).double()
    out = SimpleNamespace(C=v, exact=exact, mag=mag, absprod=absprod, off=off, valid=valid, col_sum=None, col_sumsq=None)
    if col_sum or col_sumsq:
        zz = mean = istd = None
        if stat_z is not None:
            zz = _take(stat_z, _mn(M, N, ld_stat_z, stat_z_off))
            mean, istd = _flat64(stat_mean)[:N], _flat64(stat_istd)[:N]
        s1, s2, _, _ = column_stats(v[0], valid, zz, mean, istd)
        out.col_sum = s1
        out.col_sumsq = s2 if col_sumsq else None
    return out
