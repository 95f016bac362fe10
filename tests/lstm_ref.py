"""The contract of ns_lstm_seq_params (include/nspeech_hip.h) restated on torch-CPU, forward and backward written out by
hand: what every LSTM recurrence kernel (csrc/lstm.hip, lstm_cluster.hip, lstm_wide.hip) has to compute.

    gates [i, j, f, o] = xg[t] + h[t-1].W            (h[t+1] when reverse)
    c' = sig(f + forget_bias) c[t-1] + sig(i) tanh(j),  clipped to +-cell_clip when cell_clip > 0 (straight-through gradient)
    h' = sig(o) tanh(c')
    zoneout: c[t] = m_c ? c[t-1] : c',  h[t] = m_h ? h[t-1] : h',  m(t, n, u) = zone_masks(seed, thr, ...)[t, n, u] - indexed
             by the time index t, whichever way the recurrence runs; the state before the first step is 0
    lengths: rows with t >= lengths[n] emit h = 0, c = 0, saved gates 0 and dgates 0; the predecessor of a step is read
             back from those histories, so the reverse direction starts from zero at t = lengths[n] - 1 and the forward
             direction's state past the length is never used

`lstm_seq` with no rounding and dtype float64 is the PURE reference.  The kernels store some fields in bf16 or round an
operand to bf16; `rounding` names those points after the field whose storage type causes them, and with them set the
function is the STORAGE-EXACT reference of a kernel arrangement (PRESETS):

    h            h as stored - this is also the recurrent operand of the next step and the value a kept unit holds
    gates        the saved post-activation gates - this is what the backward pass reads (with zoneout it also rebuilds the
                 plain cell's c' from them, the saved c being the zoned state)
    dgates       the gate gradients as stored
    bwd_operand  the gate gradients as the backward recurrent product reads them (dgates_bf16, the stored bf16 dgates, or
                 the in-kernel rounding at f32_passes 1)
    dh_partial   (block, rounding): ns_lstm_wide_bwd forms dh[t-1] from per-workgroup partial sums over blocks of `block`
                 units (all four gates of them); a partial sum that crosses workgroups travels as bf16, the receiver's
                 own block stays fp32

c is always fp32 and never rounded.  The weights arrive already rounded by the caller (W for the forward product, W_bwd -
default W - for the backward one: the `mixed` arrangement multiplies by fp32 weights forward and their bf16 copy backward).

dtype float32 with `perm` (a permutation of the summation index) is the same arithmetic as an fp32 kernel would do it in
another summation order: the tests measure with it what summation order and fp32 rounding alone cost an arrangement.

`plant` is for the tests of the tests only (test_lstm_ref_cpu.py): each name plants one error a kernel could have, to show
that the GPU tests' shapes and tolerances would catch it."""
import numpy as np
import torch

PLANTS = ("no_forget_bias", "swap_jf", "mask_gt", "no_reverse_restart", "clip_masked_grad", "zone_by_step", "zone_swap_masks",
          "no_dh_carry", "dc_carry_no_f")


def bf16(x):
    """x as a bf16 buffer holds it (round to nearest even), back in x's own type."""
    return x.to(torch.bfloat16).to(x.dtype)


PRESETS = {
    "pure": {},
    "bf16": dict(h=bf16, gates=bf16, dgates=bf16, bwd_operand=bf16),      # bf16 storage, forward and backward
    "mixed_fwd": {},                                                      # fp32 storage, three split-bf16 passes
    "mixed_bwd": dict(bwd_operand=bf16),                                  # fp32 storage, one bf16 pass
    "cluster_f32_fwd": dict(gates=bf16),                                  # fp32 state, the gates saved as bf16
}
PRESETS["cluster_f32"] = dict(PRESETS["cluster_f32_fwd"], dgates=bf16, bwd_operand=bf16)      # + the bf16 backward on it
PRESETS["mixed"] = dict(PRESETS["mixed_fwd"], **PRESETS["mixed_bwd"])
PRESETS["wide_bf16"] = dict(PRESETS["bf16"], dh_partial=(32, bf16))
PRESETS["wide_mixed"] = dict(PRESETS["mixed"], dh_partial=(32, bf16))


def zone_threshold(rate):
    return int(float(rate) * 16777216.0)


def _fmix32(x):
    x = x.astype(np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = (x.astype(np.uint64) * np.uint64(0x85EBCA6B) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    x = x ^ (x >> np.uint32(13))
    x = (x.astype(np.uint64) * np.uint64(0xC2B2AE35) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return x ^ (x >> np.uint32(16))


def zone_masks(seed, thr, T, N, H):
    """bool [T, N, H], True = the unit keeps its old value: m(t, n, u) = (mix(seed, t, n, u) >> 8) < thr, mix = three
    rounds of the 32-bit murmur3 finaliser over seed ^ t * 0x9E3779B9, ^ n * 0x7FEB352D, ^ u * 0x846CA68B (mod 2^32)."""
    def times(n, k):
        return (np.arange(n, dtype=np.uint64) * np.uint64(k) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    x = _fmix32(np.uint32(seed & 0xFFFFFFFF) ^ times(T, 0x9E3779B9))[:, None, None]
    x = _fmix32(x ^ times(N, 0x7FEB352D)[None, :, None])
    x = _fmix32(x ^ times(H, 0x846CA68B)[None, None, :])
    return (x >> np.uint32(8)) < np.uint32(thr)


def lstm_seq(xg, W, lengths=None, reverse=False, forget_bias=1.0, cell_clip=0.0, zoneout=None, dh=None, rounding=None,
             W_bwd=None, dtype=torch.float64, perm=None, plant=()):
    """xg [N, T, 4H], W [H, 4H], lengths [N] or None, zoneout (thr_c, thr_h, seed_c, seed_h) or None, dh [N, T, H] or None
    (forward only).  Returns h, c [N, T, H], gates [N, T, 4H] (post-activation, as stored), valid [N, T] and, with dh,
    dgates [N, T, 4H] = d sum(h * dh) / d xg (as stored) and dh_partial_max (see _bwd_product)."""
    assert all(p in PLANTS for p in plant), plant
    rnd = dict(rounding or {})
    ident = lambda x: x
    r_h, r_g, r_dg, r_op = (rnd.get(k, ident) for k in ("h", "gates", "dgates", "bwd_operand"))
    N, T, G = xg.shape
    H = G // 4
    xg, W = xg.to(dtype), W.to(dtype)
    Wb = W if W_bwd is None else W_bwd.to(dtype)
    perm = torch.arange(H) if perm is None else perm
    Wp = W[perm]
    L = torch.full((N,), T, dtype=torch.long) if lengths is None else lengths.long()
    order = list(range(T - 1, -1, -1)) if reverse else list(range(T))
    sig, clip = torch.sigmoid, float(cell_clip)
    zero = torch.zeros(N, H, dtype=dtype)
    mc = mh = None
    if zoneout is not None:
        thr_c, thr_h, seed_c, seed_h = zoneout
        mc, mh = (torch.from_numpy(zone_masks(s, th, T, N, H)) for s, th in ((seed_c, thr_c), (seed_h, thr_h)))
        if "zone_swap_masks" in plant:
            mc, mh = mh, mc
    zi = (lambda step, t: step) if "zone_by_step" in plant else (lambda step, t: t)
    fb = 0.0 if "no_forget_bias" in plant else float(forget_bias)
    sj, sf = (2, 1) if "swap_jf" in plant else (1, 2)
    is_valid = (lambda t: (t <= L)[:, None]) if "mask_gt" in plant else (lambda t: (t < L)[:, None])

    hs, cs = xg.new_zeros(N, T, H), xg.new_zeros(N, T, H)
    gs = xg.new_zeros(N, T, G)
    hp, cp = zero, zero
    for step, t in enumerate(order):
        z = xg[:, t] + hp[:, perm] @ Wp
        i, j, f, o = sig(z[:, :H]), torch.tanh(z[:, sj * H:(sj + 1) * H]), sig(z[:, sf * H:(sf + 1) * H] + fb), sig(z[:, 3 * H:])
        c2 = f * cp + i * j
        if clip > 0:
            c2 = c2.clamp(-clip, clip)
        h2 = o * torch.tanh(c2)
        if mc is not None:
            c2 = torch.where(mc[zi(step, t)], cp, c2)
            h2 = torch.where(mh[zi(step, t)], hp, h2)
        v = is_valid(t)
        h2 = r_h(h2)
        hs[:, t], cs[:, t] = torch.where(v, h2, zero), torch.where(v, c2, zero)
        gs[:, t] = r_g(torch.cat([i, j, f, o], 1)) * v
        if "no_reverse_restart" in plant and reverse:
            hp, cp = h2, c2                      # the state runs on through the padding instead of restarting at the length
        else:
            hp, cp = hs[:, t], cs[:, t]          # the next step reads its predecessor back from the histories
    out = dict(h=hs, c=cs, gates=gs, valid=torch.arange(T)[None, :] < L[:, None])
    if dh is None:
        return out

    dh = dh.to(dtype)
    dgs = xg.new_zeros(N, T, G)
    dcc, dhc, op, partial_max = zero, zero, None, 0.0
    product = _bwd_product(Wb, perm, rnd.get("dh_partial"))
    for step in range(T - 1, -1, -1):
        t = order[step]
        cp = cs[:, order[step - 1]] if step > 0 else zero
        i, j, f, o = (gs[:, t, k * H:(k + 1) * H] for k in range(4))
        d = dh[:, t]
        if op is not None:
            rec, pmax = product(op)
            d, partial_max = d + rec, max(partial_max, pmax)
        dcin, dckeep, c = dcc, zero, cs[:, t]
        raw = f * cp + i * j                     # the plain cell's c' before the clip
        if mc is not None:
            if "no_dh_carry" not in plant:
                d = d + dhc
            kh, kc = mh[zi(step, t)], mc[zi(step, t)]
            dhc = torch.where(kh, d, zero)
            d = torch.where(kh, zero, d)
            dckeep, dcin = torch.where(kc, dcin, zero), torch.where(kc, zero, dcin)
            c = raw.clamp(-clip, clip) if clip > 0 else raw      # the saved c is the zoned state: h' was o tanh(c')
        tc = torch.tanh(c)
        dc = d * o * (1 - tc * tc) + dcin
        if "clip_masked_grad" in plant and clip > 0:
            dc = dc * (raw.abs() < clip)
        dg = torch.cat([dc * j * i * (1 - i), dc * i * (1 - j * j), dc * cp * f * (1 - f), d * tc * o * (1 - o)], 1)
        dcc = (dc if "dc_carry_no_f" in plant else dc * f) + dckeep
        v = is_valid(t)
        dg, dcc, dhc = dg * v, dcc * v, dhc * v
        dgs[:, t] = r_dg(dg)
        op = r_op(dg)
    out["dgates"], out["dh_partial_max"] = dgs, partial_max      # the largest partial sum that travelled rounded
    return out


def _bwd_product(Wb, perm, partial):
    """op [N, 4H] -> dh[n, u] = sum_k op[n, k] Wb[u, k] over the 4H gate columns k, and the largest |partial sum| that
    was rounded on the way."""
    H = Wb.shape[0]
    if partial is None:
        kperm = torch.cat([perm + g * H for g in range(4)])
        wt = Wb[:, kperm].t().contiguous()
        return lambda op: (op[:, kperm] @ wt, 0.0)
    block, r = partial
    nb = H // block
    bp = perm[perm < block]                      # the summation order inside a block
    ws = Wb.reshape(H, 4, nb, block)[..., bp].permute(2, 1, 3, 0).reshape(nb, 4 * block, H).contiguous()
    own = ((torch.arange(H) // block)[:, None] == torch.arange(nb)[None, :])[None]

    def product(op):
        ops = op.reshape(-1, 4, nb, block)[..., bp].permute(2, 0, 1, 3).reshape(nb, -1, 4 * block)   # [source block][n][gate, unit]
        part = torch.bmm(ops, ws).permute(1, 2, 0)                                                   # [n][u][source block]
        return torch.where(own, part, r(part)).sum(-1), float((part.abs() * ~own).max())
    return product
