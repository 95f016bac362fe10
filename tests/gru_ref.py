"""The contract of ns_gru_seq_params (include/nspeech_hip.h) restated on torch-CPU, forward and backward written out by
hand: what the persistent whole-sequence GRU kernels (csrc/gru.hip: ns_gru_seq_fwd / ns_gru_seq_bwd) have to compute.

    [r | u] = sigmoid(xg[t] + h . Wg_h)      c = tanh(xc[t] + (r * h) . Wc_h)      h' = u * h + (1 - u) * c
    h = h_init (or 0) before the first step; reverse walks t = T-1 .. 0
    lengths: a row with t >= lengths[n] emits h = 0, dzg = 0 and dzc = 0 exactly and carries the state - and, backward,
             the gradient carry - unchanged: the reverse direction meets h_init at t = lengths[n] - 1, and a length of 0
             leaves a row of zeros and dh_init = 0.  The saved gates ru, c and rh of such steps are not part of the
             contract (the kernel writes finite values there; here they are what the carried state gives).
    backward (the recurrence in the comment above gru_bwd_kernel), steps in the reverse of the forward order, carry = 0
    before the first, dh = masked ? 0 : carry + dh_out[t]:
             dzc = dh (1 - u)(1 - c^2)     dzu = dh (h_prev - c) u (1 - u)     carry' = masked ? carry : dh u
             drh = dzc . Wc_h^T            dzr = drh h_prev r (1 - r)          carry' += drh r + [dzr | dzu] . Wg_h^T
             dh_init = the carry behind the last step: OVERWRITTEN, whatever the buffer held
    windows: [(t0, t1), ...] evaluates the sequence as models/tacotron.py: _gru_pair launches it - one launch per window
             on the steps [t0, t1), forward in order with h_init = the STORED history row t0 - 1 (window 0: the caller's
             h_init), backward in reverse order with a window's dh_init added to dh_out[t0 - 1] before the window in front
             of it runs.  Forward direction without lengths only.

`gru_seq` with no rounding and dtype float64 is the PURE reference.  `rounding` names the points where a kernel form
rounds, after the field that causes them; with them set the function is the STORAGE-EXACT reference of an arrangement
(PRESETS).  Read off csrc/gru.hip:

    never rounded  the state a lane carries (hst), the gradient carry, the saved ru and c, dh_init: fp32 in every form.
                   h' = u hst + (1 - u) c and r * hst are formed from the fp32 state, not from the operand image.
    fwd_product    f32_passes / dtype of the forward call: how the two forward products read their operands - h and
                   r * h from the LDS images, the weights from registers.  "bf16": both rounded to bf16 (one pass; bf16
                   storage hands the weights over as bf16 already).  "split": x = hi + lo, hi = bf16(x), lo = bf16(x - hi)
                   for both, and the product is hi.hi + lo.hi + hi.lo (three passes, lo.lo dropped).
    bwd_product    the same for the two backward products (operands dzc and [dzr | dzu]).
    h              dtype: h as stored.  This is what the backward pass reads h_prev from (at a sequence's first step it
                   reads the fp32 h_init instead) and what a window's h_init is a copy of - so with bf16 storage a window
                   edge rounds the state, which a whole-sequence launch never does.
    rh, dz         dtype: rh, and dzg / dzc, as stored.

dtype float32 with `perm` (a permutation of the summation index) is the same arithmetic as an fp32 kernel would do it in
another summation order: the tests measure with it what summation order and fp32 rounding alone cost an arrangement.

`plant` is for the tests of the tests only (test_gru_ref_cpu.py): each name plants one error a kernel (window_no_handover:
a caller) could have, to show that the GPU tests' shapes and tolerances would catch it."""
import torch

PLANTS = ("mask_gt", "state_zeroed_masked", "reverse_start_T", "first_hprev_from_history", "swap_u", "reset_after",
          "swap_ru", "dzu_from_h", "carry_no_drh_r", "carry_no_dh_u", "dh_on_masked", "dh_init_accumulate",
          "window_no_handover")


def bf16(x):
    """x as a bf16 buffer holds it (round to nearest even), back in x's own type."""
    return x.to(torch.bfloat16).to(x.dtype)


PRESETS = {
    "pure": {},
    "f32x3": dict(fwd_product="split", bwd_product="split"),              # fp32 storage, three split-bf16 passes
    "f32x1": dict(fwd_product="bf16", bwd_product="bf16"),                # fp32 storage, one bf16 pass
    "mixed": dict(fwd_product="split", bwd_product="bf16"),               # f32x3 forward, f32x1 backward on its saved gates
    "bf16": dict(fwd_product="bf16", bwd_product="bf16", h=bf16, rh=bf16, dz=bf16),
}


def _product(kind, W):
    """x [N, K] -> x . W [K, M] as a kernel form reads the operands (module docstring: fwd_product)."""
    if kind is None:
        return lambda x: x @ W
    Wh = bf16(W)
    if kind == "bf16":
        return lambda x: bf16(x) @ Wh
    assert kind == "split", kind
    Wl = bf16(W - Wh)

    def three_passes(x):
        xh = bf16(x)
        xl = bf16(x - xh)
        return (xh @ Wl + xl @ Wh) + xh @ Wh
    return three_passes


def _forward(xg, xc, Wg, Wc, L, reverse, h0, rnd, perm, plant):
    """One launch.  Returns h (as stored), ru, c, rh (as stored) [N, T, .]."""
    ident = lambda x: x
    r_h, r_rh = rnd.get("h", ident), rnd.get("rh", ident)
    N, T, H2 = xg.shape
    H = H2 // 2
    pg, pc = _product(rnd.get("fwd_product"), Wg[perm]), _product(rnd.get("fwd_product"), Wc[perm])
    zero = xg.new_zeros(N, H)
    hs, rus, cs, rhs = xg.new_zeros(N, T, H), xg.new_zeros(N, T, H2), xg.new_zeros(N, T, H), xg.new_zeros(N, T, H)
    hp = zero if h0 is None else h0
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        v = ((t <= L) if "mask_gt" in plant else (t < L))[:, None]
        ru = torch.sigmoid(xg[:, t] + pg(hp[:, perm]))
        r, u = (ru[:, H:], ru[:, :H]) if "swap_ru" in plant else (ru[:, :H], ru[:, H:])
        rh = r * hp
        if "reset_after" in plant:
            c = torch.tanh(xc[:, t] + r * pc(hp[:, perm]))
        else:
            c = torch.tanh(xc[:, t] + pc(rh[:, perm]))
        hn = (1 - u) * hp + u * c if "swap_u" in plant else u * hp + (1 - u) * c
        hs[:, t] = torch.where(v, r_h(hn), zero)
        rus[:, t], cs[:, t], rhs[:, t] = ru, c, r_rh(rh)
        if "reverse_start_T" in plant and reverse:
            hp = hn                              # the state runs through the padding instead of waiting for t = len - 1
        elif "state_zeroed_masked" in plant:
            hp = torch.where(v, hn, zero)
        else:
            hp = torch.where(v, hn, hp)          # carried through masked steps
    return hs, rus, cs, rhs


def _backward(hs, rus, cs, Wg, Wc, L, reverse, h0, dh, rnd, perm, plant, front=None, prefill=None):
    """One launch, on the stored history and the saved gates of its forward launch.  front = the history row in front
    of the launch's first step (a window's; None = a zero pad row) - only a planted error reads it.  Returns dzg, dzc
    (as stored), dh_init and the largest |carry + dh_out| of a valid step."""
    ident = lambda x: x
    r_dz = rnd.get("dz", ident)
    N, T, H = hs.shape
    pc = _product(rnd.get("bwd_product"), Wc.t()[perm].contiguous())
    pg = _product(rnd.get("bwd_product"), Wg.t()[torch.cat([perm, perm + H])].contiguous())
    perm2 = torch.cat([perm, perm + H])
    zero = hs.new_zeros(N, H)
    hini = zero if h0 is None else h0
    dzgs, dzcs = hs.new_zeros(N, T, 2 * H), hs.new_zeros(N, T, H)
    carry, total_max = zero, 0.0
    for t in (range(T) if reverse else range(T - 1, -1, -1)):
        tp = t + 1 if reverse else t - 1
        v = ((t <= L) if "mask_gt" in plant else (t < L))[:, None]
        first = (t == L - 1)[:, None] if reverse else torch.full((N, 1), t == 0)
        hist = hs[:, tp] if 0 <= tp < T else (zero if front is None else front)
        hp = hist if "first_hprev_from_history" in plant else torch.where(first, hini, hist)
        ru, c = rus[:, t], cs[:, t]
        r, u = (ru[:, H:], ru[:, :H]) if "swap_ru" in plant else (ru[:, :H], ru[:, H:])
        d = torch.where(v, carry + dh[:, t], zero)
        total_max = max(total_max, float(d.abs().max()))
        dzc = d * (1 - u) * (1 - c * c)
        dzu = d * ((hs[:, t] if "dzu_from_h" in plant else hp) - c) * u * (1 - u)
        keep = zero if "state_zeroed_masked" in plant else carry + dh[:, t] if "dh_on_masked" in plant else carry
        cn = torch.where(v, zero if "carry_no_dh_u" in plant else d * u, keep)
        drh = pc(dzc[:, perm])
        dzr = drh * hp * r * (1 - r)
        if "carry_no_drh_r" not in plant:
            cn = cn + drh * r
        dzg = torch.cat([dzu, dzr] if "swap_ru" in plant else [dzr, dzu], 1)
        carry = cn + pg(dzg[:, perm2])
        dzgs[:, t], dzcs[:, t] = r_dz(dzg), r_dz(dzc)
    if "dh_init_accumulate" in plant and prefill is not None:
        carry = carry + prefill
    return dzgs, dzcs, carry, total_max


def gru_seq(xg, xc, Wg, Wc, lengths=None, reverse=False, h_init=None, dh=None, rounding=None, dtype=torch.float64, perm=None,
            plant=(), windows=None, dh_init_prefill=None):
    """xg [N, T, 2H], xc [N, T, H], Wg [H, 2H], Wc [H, H], lengths [N] or None, h_init [N, H] or None, dh [N, T, H] or None
    (forward only), windows [(t0, t1), ...] or None (one launch), dh_init_prefill: what the dh_init buffers hold before
    the launch (a number; only a planted error sees it).  Returns h, rh (as stored), ru, c [N, T, .], valid [N, T] and,
    with dh, dzg, dzc (as stored) = d sum(h * dh) / d (xg, xc), dh_init [N, H] = d / d h_init and dh_total_max."""
    assert all(p in PLANTS for p in plant), plant
    rnd = dict(rounding or {})
    N, T, H2 = xg.shape
    H = H2 // 2
    xg, xc, Wg, Wc = xg.to(dtype), xc.to(dtype), Wg.to(dtype), Wc.to(dtype)
    h0 = None if h_init is None else h_init.to(dtype)
    perm = torch.arange(H) if perm is None else perm
    L = torch.full((N,), T, dtype=torch.long) if lengths is None else lengths.long()
    if windows is None:
        windows = [(0, T)]
    else:
        assert lengths is None and not reverse and windows[0][0] == 0 and windows[-1][1] == T
        assert all(a[1] == b[0] for a, b in zip(windows, windows[1:]))
    hs, rus, cs, rhs = xg.new_zeros(N, T, H), xg.new_zeros(N, T, H2), xg.new_zeros(N, T, H), xg.new_zeros(N, T, H)
    inits = []
    for t0, t1 in windows:
        w = slice(t0, t1)
        hi = h0 if t0 == 0 else hs[:, t0 - 1].clone()        # a copy of the stored row: rounded where h is
        inits.append(hi)
        Lw = (L - t0).clamp(0, t1 - t0)
        hs[:, w], rus[:, w], cs[:, w], rhs[:, w] = _forward(xg[:, w], xc[:, w], Wg, Wc, Lw, reverse, hi, rnd, perm, plant)
    out = dict(h=hs, ru=rus, c=cs, rh=rhs, valid=torch.arange(T)[None, :] < L[:, None])
    if dh is None:
        return out
    dh = dh.to(dtype).clone()
    dzgs, dzcs, total_max = xg.new_zeros(N, T, H2), xg.new_zeros(N, T, H), 0.0
    for (t0, t1), hi in reversed(list(zip(windows, inits))):
        w = slice(t0, t1)
        Lw = (L - t0).clamp(0, t1 - t0)
        dzgs[:, w], dzcs[:, w], dhi, tm = _backward(hs[:, w], rus[:, w], cs[:, w], Wg, Wc, Lw, reverse, hi, dh[:, w], rnd, perm,
                                                   plant, front=hs[:, t0 - 1] if t0 else None, prefill=dh_init_prefill)
        total_max = max(total_max, tm)
        if t0 and "window_no_handover" not in plant:
            dh[:, t0 - 1] = dh[:, t0 - 1] + dhi                # the caller's accumulate onto the row in front
    out.update(dzg=dzgs, dzc=dzcs, dh_init=dhi, dh_total_max=total_max)
    return out
