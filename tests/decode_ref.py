"""The contracts of the kernels that run free-running synthesis, restated on torch-CPU in float64 from
include/nspeech_hip.h: ns_taco2_decode_params, ns_taco1_decode_params, ns_lstm_step_params, ns_rows32_params (dense and
cell form, with ns_rows32_pack / ns_rows32_pack_rows' two packed layouts) and the two key transposes.  Nothing here is
taken from the kernels except where a sentence says so; tests/test_decode_ref_cpu.py proves the loops against the
oracle's cells run free, the steps against tests/lstm_ref.py and a plain product, the layouts against each other.

Tacotron-2 (ns_taco2_decode), step s = 0 .. S-1, histories in slot s + 1 of [N, S+1, X] buffers whose slot 0 is zero:
    p1 = relu(f1[s+1] + align[s-1] . pv)               p2 = relu(p1 W2 + b2)            (f1[1] given; pv = values . W1c)
    xa = [p2 | speaker projection | h_att[s-1]]        z = xa Watt + batt, gates [i, j, f, o], forget bias 1
    q = h_att Wq;  e, align as in ns_taco2_attn_params (taps at t + k - (kw-1)//2);  ctx = align . values
    (c1, h1) = LSTM([h_att | ctx | h1[s-1]] w_l1 + b_l1)     (c2, h2) = LSTM([h1 | h2[s-1]] w_l2 + b_l2)
    f1[s+2] = h2 wpf + bpf                             every cell clipped to +-cell_clip where cell_clip > 0
Written: align, p1, xa, q, ca, ga, hc[:, :, :A], h2.

Tacotron-1 (ns_taco1_decode): the attention LSTM becomes GRUCell ([r | u] = sig([x | h] Wg + bg), c = tanh([x | r h] Wc
+ bc), h' = u h + (1 - u) c), no location term, then
    x1 = [h_att | ctx] w_proj + b_proj    h1 = GRU_1(x1, h1)    y1 = x1 + h1    h2 = GRU_2(y1, h2)    y2 = y1 + h2
    f1[s+2] = y2 wpf + bpf
Written: align, p1, xa, xc, hc[:, :, :A], ru, cc, q, y2.

One step (ns_lstm_step, the cell form of ns_rows32): z = a . W + xg + bias, gates [i, j, f, o];
    c' = clip(sig(f + forget_bias) c_prev + sig(i) tanh(j));  h' = sig(o) tanh(c')        (c_prev NULL = zeros)
    zoneout expectation, where a rate > 0:  c = zc c_prev + (1 - zc) c',  h = zh h_prev + (1 - zh) h'   (AFTER the clip)
Dense form of ns_rows32: y = act(a . w + bias + add).

`dtype` float32 with `perm_seed`: the same arithmetic with every sum in another order (what fp32 rounding alone costs).
`bf16_storage`: the storage-exact reference for att.dtype = bf16, read off csrc/attn_cluster.hip / attn_gru.hip exactly as
tests/attn_ref.py states it: the caller hands the bf16 operands in rounded, the loops carry fp32 between workgroups and
round p1, xa, xc, hc, ga where they are stored and only there; the decoder cells' weights and states are fp32.  The
contexts of the decoder cells come from the fp32 alignments (never from align_t).  For a step, `product` names the operand
arrangement: "exact" (fp32 FMAs, or bf16 operands the caller rounded), "one" (both operands rounded to bf16), "two" (the
weights rounded), "three" (split3 of attn_ref).

The split (csrc/common.h: hi = bf16(x), lo = bf16(x - hi), round to nearest even; ns_rows32_store, rows32_pack_kernel,
ldsplit8): bf16 keeps 8 significand bits, so |x - hi| <= 2^-8 |x|, x - hi is exact in fp32, and |x - hi - lo| <= 2^-8
|x - hi| <= 2^-16 |x|: hi + lo keeps 16 bits (SPLIT_EPS).  A three-pass product lo.hi + hi.lo + hi.hi leaves out lo.lo
(<= 2^-16 |a||w|) and what neither pair holds (2 x 2^-16 |a||w|): 3 x 2^-16 |a||w| summed over k, THREE_EPS x mag.

Lipschitz constants of the cell (cell_bounds): with every gate pre-activation within b of the reference's,
    |dc'| <= (1/4)|c_prev| b  [forget]  +  (1/4) b  [input, |tanh| <= 1]  +  b  [candidate, sig <= 1, tanh' <= 1]
    |dh'| <= (1/4) b  [output, |tanh c| <= 1]  +  |dc'|  [sig <= 1, tanh' <= 1];  the clip and the zoneout mix are 1-Lipschitz.
The activations themselves (common.h: v_exp_f32 + v_rcp_f32 forms, "absolute error ~1e-7") are given ACT_EPS = 8 u each
(u = 2^-24): tanh = 1 - 2 r with r near 1/2 carries 2 x (exp, add and rcp: 3 u / 2) + u = 4 u, doubled; the products and sums
of the update add at most 4 u (|c_prev| + 1).  So b_c = (5/4 + |c_prev|/4) b + 16 u (|c_prev| + 2), b_h = b/4 + b_c + 16 u (1 + |h_prev|).

`plant` is for tests/test_decode_ref_cpu.py only: each name plants one error these kernels could make."""
import numpy as np
import torch
import torch.nn.functional as F

from attn_ref import _Sum, _masked_softmax, _taps, bf16, split3

U = 2.0 ** -24
SPLIT_EPS = 2.0 ** -16
THREE_EPS = 3.0 * 2.0 ** -16
ACT_EPS = 8 * U

LOOP_PLANTS = ("ctx_term_stale", "l2_hprev_is_input", "no_forget_bias_l2", "gates_ifjo", "clip_attention_only",
               "no_residual_y1", "gru_rh_stale", "second_row_first_length", "mask_len_plus1", "even_kw_pad_left",
               "no_speaker_rows", "feedback_from_l1")
STEP_PLANTS = ("zoneout_swapped", "clip_after_zoneout", "forget_bias_one", "gates_ifjo", "add_after_act", "cell_tile_order",
               "c_prev_ignored")
PLANTS = LOOP_PLANTS + tuple(p for p in STEP_PLANTS if p not in LOOP_PLANTS)
TACO2_DECODE = ("align", "p1", "xa", "q", "ca", "ga", "hc", "h2")
TACO1_DECODE = ("align", "p1", "xa", "xc", "hc", "ru", "cc", "q", "y2")


def _valid(lengths, Ti, plant):
    L = lengths.long().clone()
    if "second_row_first_length" in plant:           # the second row of a pair masked with the first row's length
        L[1::2] = L[0::2][:L[1::2].numel()]
    if "mask_len_plus1" in plant:
        L = (L + 1).clamp(max=Ti)
    return torch.arange(Ti)[None, :] < L[:, None]


def _lstm(z, c_prev, H, forget_bias, clip, ifjo=False):
    i, j, f, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
    if ifjo:
        j, f = f, j
    gi, gj, gf, go = torch.sigmoid(i), torch.tanh(j), torch.sigmoid(f + forget_bias), torch.sigmoid(o)
    c = gf * c_prev + gi * gj
    clipped = None
    if clip > 0:
        clipped = c.abs() > clip
        c = c.clamp(-clip, clip)
    return go * torch.tanh(c), c, torch.cat([gi, gj, gf, go], 1), clipped


def _gru(sm, xin, h, Wg, bg, Wc, bc, tag, h_for_r=None):
    """GRUCell; h_for_r (a plant) = the state the candidate's r * h is built from."""
    xa = torch.cat(xin + [h], 1)
    ru = torch.sigmoid(sm.mm(xa, Wg, tag + "g") + bg)
    H = h.shape[1]
    r, u = ru[:, :H], ru[:, H:]
    xc = torch.cat(xin + [r * (h if h_for_r is None else h_for_r)], 1)
    cc = torch.tanh(sm.mm(xc, Wc, tag + "c") + bc)
    return u * h + (1 - u) * cc, ru, cc, xa, xc


def _attend(sm, keys, values, pv, q, v, valid, loc=None):
    xt = keys + q[:, None, :]
    if loc is not None:
        xt = xt + loc
    e = sm.sum_last(v * torch.tanh(xt), "e")
    align = _masked_softmax(e, valid)
    pt = sm.perm(keys.shape[1], "ctx")
    ctx = torch.einsum("nt,nte->ne", align[:, pt], values[:, pt])
    return align, ctx, torch.einsum("nt,nte->ne", align[:, pt], pv[:, pt])


def _finish(H, extra, st, rounded, lengths, Ti):
    out = {k: torch.stack(t, 1) for k, t in H.items()}
    out.update({k: torch.stack(t, 1) for k, t in extra.items() if t and t[0] is not None})
    for k in rounded:
        out[k] = st(out[k])
    out["valid"] = torch.arange(Ti)[None, :] < lengths.long()[:, None]
    return out


def taco2_decode(x, dtype=torch.float64, perm_seed=None, bf16_storage=False, plant=()):
    """x: keys [N, Ti, A], values [N, Ti, E], pv [N, Ti, D1], f1 [N, S+1, D1] (slot 1 is read), W2 [D1, D2], b2, Watt
    [D2+Dsp+A, 4A], batt, Wq [A, A], Wcl [kw, A], v [A], lengths [N], cell_clip, spk [N, Dsp] or None, w_l1 [A+E+D, 4D],
    b_l1, w_l2 [2D, 4D], b_l2, wpf [D, D1], bpf [D1].  Returns the written histories [N, S+1, X] (hc = its A columns) and,
    for the CPU checks, z1, z2, ctx, h1, c1, c2 and the per-cell clip masks."""
    assert all(p in PLANTS for p in plant), plant
    sm = _Sum(perm_seed)
    st = bf16 if bf16_storage else (lambda t: t)
    g = lambda k: x[k].to(dtype)
    keys, values, pv, W2, b2, Watt, batt, Wq, Wcl, v = (g(k) for k in ("keys", "values", "pv", "W2", "b2", "Watt", "batt", "Wq", "Wcl", "v"))
    w1, b1, w2, b2d, wpf, bpf = (g(k) for k in ("w_l1", "b_l1", "w_l2", "b_l2", "wpf", "bpf"))
    spk = x.get("spk")
    clip = float(x.get("cell_clip", 0.0))
    dclip = 0.0 if "clip_attention_only" in plant else clip
    N, Ti, A = keys.shape
    S, D, D2 = x["f1"].shape[1] - 1, wpf.shape[0], W2.shape[1]
    Dsp = 0 if spk is None else spk.shape[1]
    kw = Wcl.shape[0]
    half = kw // 2 if ("even_kw_pad_left" in plant and kw % 2 == 0) else (kw - 1) // 2
    valid = _valid(x["lengths"], Ti, plant)
    zero = lambda w: torch.zeros(N, w, dtype=dtype)
    ifjo = "gates_ifjo" in plant
    H = dict(p1=[zero(W2.shape[0])], xa=[zero(D2 + Dsp + A)], hc=[zero(A)], ca=[zero(A)], ga=[zero(4 * A)], q=[zero(A)],
             align=[zero(Ti)], h2=[zero(D)], z1=[zero(W2.shape[0])], z2=[zero(D2)])
    extra = dict(ctx=[], h1=[], c1=[], c2=[], clip_a=[], clip_1=[], clip_2=[])
    h, c, h1, c1, h2, c2, align = zero(A), zero(A), zero(D), zero(D), zero(D), zero(D), zero(Ti)
    f, terms = g("f1")[:, 1], [zero(W2.shape[0]), zero(W2.shape[0])]
    for s in range(S):
        z1 = f + terms[-2 if "ctx_term_stale" in plant else -1]
        p1 = torch.relu(z1)
        z2 = sm.mm(p1, W2, "w2") + b2
        p2 = torch.relu(z2)
        xa = torch.cat([p2] + ([spk.to(dtype)] if Dsp else []) + [h], 1)
        if "no_speaker_rows" in plant and Dsp:
            z = sm.mm(torch.cat([p2, h], 1), torch.cat([Watt[:D2], Watt[D2 + Dsp:]], 0), "watt2") + batt
        else:
            z = sm.mm(xa, Watt, "watt") + batt
        h, c, gates, ka = _lstm(z, c, A, 1.0, clip)
        q = sm.mm(h, Wq, "wq")
        align, ctx, term = _attend(sm, keys, values, pv, q, v, valid, sm.mm(_taps(align, kw, half), Wcl, "wcl"))
        terms.append(term)
        h1, c1, _, k1 = _lstm(sm.mm(torch.cat([h, ctx, h1], 1), w1, "l1") + b1, c1, D, 1.0, dclip, ifjo)
        hp2 = h1 if "l2_hprev_is_input" in plant else h2
        h2, c2, _, k2 = _lstm(sm.mm(torch.cat([h1, hp2], 1), w2, "l2") + b2d, c2, D, 0.0 if "no_forget_bias_l2" in plant else 1.0,
                              dclip, ifjo)
        f = sm.mm(h1 if "feedback_from_l1" in plant else h2, wpf, "wpf") + bpf
        for k_, t_ in (("p1", p1), ("xa", xa), ("hc", h), ("ca", c), ("ga", gates), ("q", q), ("align", align), ("h2", h2),
                       ("z1", z1), ("z2", z2)):
            H[k_].append(t_)
        for k_, t_ in (("ctx", ctx), ("h1", h1), ("c1", c1), ("c2", c2)) + ((("clip_a", ka), ("clip_1", k1), ("clip_2", k2)) if clip > 0 else ()):
            extra[k_].append(t_)
    return _finish(H, extra, st, ("p1", "xa", "hc", "ga"), x["lengths"], Ti)


def taco1_decode(x, dtype=torch.float64, perm_seed=None, bf16_storage=False, plant=()):
    """x: keys, values [N, Ti, E], pv, f1 (slot 1), W2, b2, Wg [D2+Dsp+A, 2A], bg, Wc [D2+Dsp+A, A], bc, Wq, v, lengths, spk or
    None, w_proj [A+E, D], b_proj, wg_1 [2D, 2D], bg_1, wc_1 [2D, D], bc_1, wg_2, bg_2, wc_2, bc_2, wpf [D, D1], bpf."""
    assert all(p in PLANTS for p in plant), plant
    sm = _Sum(perm_seed)
    st = bf16 if bf16_storage else (lambda t: t)
    g = lambda k: x[k].to(dtype)
    keys, values, pv, W2, b2, Wg, bg, Wc, bc, Wq, v = (g(k) for k in ("keys", "values", "pv", "W2", "b2", "Wg", "bg", "Wc", "bc", "Wq", "v"))
    wp, bp, wpf, bpf = g("w_proj"), g("b_proj"), g("wpf"), g("bpf")
    G = {i: tuple(g("%s_%d" % (k, i)) for k in ("wg", "bg", "wc", "bc")) for i in (1, 2)}
    spk = x.get("spk")
    N, Ti, A = keys.shape
    S, D, D1, D2 = x["f1"].shape[1] - 1, wpf.shape[0], W2.shape[0], W2.shape[1]
    Dsp = 0 if spk is None else spk.shape[1]
    XA = D2 + Dsp + A
    valid = _valid(x["lengths"], Ti, plant)
    zero = lambda w: torch.zeros(N, w, dtype=dtype)
    H = dict(p1=[zero(D1)], xa=[zero(XA)], xc=[zero(XA)], hc=[zero(A)], ru=[zero(2 * A)], cc=[zero(A)], q=[zero(A)],
             align=[zero(Ti)], y2=[zero(D)], z1=[zero(D1)], z2=[zero(D2)])
    extra = dict(ctx=[])
    h, h1, h2 = zero(A), zero(D), zero(D)
    older = dict(a=zero(A), h1=zero(D), h2=zero(D))
    f, terms = g("f1")[:, 1], [zero(D1), zero(D1)]
    stale = "gru_rh_stale" in plant
    for s in range(S):
        z1 = f + terms[-2 if "ctx_term_stale" in plant else -1]
        p1 = torch.relu(z1)
        z2 = sm.mm(p1, W2, "w2") + b2
        p2 = torch.relu(z2)
        xin = [p2] + ([spk.to(dtype)] if Dsp else [])
        if "no_speaker_rows" in plant and Dsp:
            keep = torch.cat([torch.arange(D2), torch.arange(D2 + Dsp, XA)])
            hn, ru, cc, _, _ = _gru(sm, [p2], h, Wg[keep], bg, Wc[keep], bc, "a2", older["a"] if stale else None)
            xa, xc = torch.cat(xin + [h], 1), torch.cat(xin + [ru[:, :A] * h], 1)
        else:
            hn, ru, cc, xa, xc = _gru(sm, xin, h, Wg, bg, Wc, bc, "a", older["a"] if stale else None)
        older["a"], h = h, hn
        q = sm.mm(h, Wq, "wq")
        align, ctx, term = _attend(sm, keys, values, pv, q, v, valid)
        terms.append(term)
        x1 = sm.mm(torch.cat([h, ctx], 1), wp, "proj") + bp
        n1 = _gru(sm, [x1], h1, *G[1], "g1", older["h1"] if stale else None)[0]
        older["h1"], h1 = h1, n1
        y1 = h1 if "no_residual_y1" in plant else x1 + h1
        n2 = _gru(sm, [y1], y1 if "l2_hprev_is_input" in plant else h2, *G[2], "g2", older["h2"] if stale else None)[0]
        older["h2"], h2 = h2, n2
        y2 = y1 + h2
        f = sm.mm(y1 if "feedback_from_l1" in plant else y2, wpf, "wpf") + bpf
        for k_, t_ in (("p1", p1), ("xa", xa), ("xc", xc), ("hc", h), ("ru", ru), ("cc", cc), ("q", q), ("align", align),
                       ("y2", y2), ("z1", z1), ("z2", z2)):
            H[k_].append(t_)
        extra["ctx"].append(ctx)
    return _finish(H, extra, st, ("p1", "xa", "xc", "hc"), x["lengths"], Ti)


# ------------------------------------------------------------------------------------------------------- one step
def _product(sm, a, w, product, tag):
    """a [N, K] @ w [K, C] as the named operand arrangement runs it (module docstring)."""
    if product == "one":
        return sm.mm(bf16(a), bf16(w), tag)
    if product == "two":
        return sm.mm(a, bf16(w), tag)
    if product == "three":
        if sm.g is not None:
            p = sm.perm(w.shape[0], tag)
            a, w = a[..., p], w[p]
        return split3(a, w)
    assert product == "exact", product
    return sm.mm(a, w, tag)


def _cell_step(z, x, H, dtype, plant, st):
    N = z.shape[0]
    cp = x["c_prev"].to(dtype) if x.get("c_prev") is not None and "c_prev_ignored" not in plant else torch.zeros(N, H, dtype=dtype)
    hp = x["h_prev"].to(dtype) if x.get("h_prev") is not None else torch.zeros(N, H, dtype=dtype)
    fb = 1.0 if "forget_bias_one" in plant else float(x.get("forget_bias", 1.0))
    clip = float(x.get("cell_clip", 0.0))
    zc, zh = float(x.get("zoneout_cell", 0.0)), float(x.get("zoneout_output", 0.0))
    if "zoneout_swapped" in plant:
        zc, zh = zh, zc
    late = "clip_after_zoneout" in plant
    h, c, gates, clipped = _lstm(z, cp, H, fb, 0.0 if late else clip, "gates_ifjo" in plant)
    if zc > 0 or zh > 0:
        c = zc * cp + (1 - zc) * c
        h = zh * hp + (1 - zh) * h
    if late and clip > 0:
        c = c.clamp(-clip, clip)
    return dict(z=z, h=st(h), c=c, c_prev=cp, h_prev=hp, clipped=clipped)


def lstm_step(x, dtype=torch.float64, perm_seed=None, bf16_storage=False, product="exact", plant=()):
    """ns_lstm_step.  x: a [N, K], wT [4H, K] (the TF kernel transposed), xg [N, 4H] or None, bias [4H] or None, c_prev
    [N, H] or None, h_prev or None, forget_bias, zoneout_cell, zoneout_output, cell_clip.  With bf16_storage the caller hands
    a, wT, h_prev in rounded and h is rounded where it is stored.  Returns z, h, c (and c_prev, h_prev as read)."""
    assert all(p in PLANTS for p in plant), plant
    sm = _Sum(perm_seed)
    a, w = x["a"].to(dtype), x["wT"].to(dtype).t()
    H = w.shape[1] // 4
    z = _product(sm, a, w, product, "w")
    for k in ("xg", "bias"):
        if x.get(k) is not None:
            z = z + x[k].to(dtype)
    return _cell_step(z, x, H, dtype, plant, bf16 if bf16_storage else (lambda t: t))


def rows32_cell(x, dtype=torch.float64, perm_seed=None, bf16_storage=False, product="three", plant=()):
    """The cell form of ns_rows32.  x: a [N, K], w [K, 4H] (the TF kernel as stored), bias or None, and the cell's operands
    as for lstm_step.  bf16_storage has nothing to round (every operand and result is fp32); product "one" = f32_passes 1."""
    assert all(p in PLANTS for p in plant), plant
    sm = _Sum(perm_seed)
    w = x["w"].to(dtype)
    z = _product(sm, x["a"].to(dtype), w, product, "w")
    if x.get("bias") is not None:
        z = z + x["bias"].to(dtype)
    return _cell_step(z, x, w.shape[1] // 4, dtype, plant, lambda t: t)


def _act(z, act):
    return [lambda t: t, torch.relu, torch.tanh, torch.sigmoid, F.softsign][act](z)


def rows32_dense(x, dtype=torch.float64, perm_seed=None, bf16_storage=False, product="three", plant=()):
    """The dense form of ns_rows32: y = act(a . w + bias + add).  Returns z (the pre-activation) and y."""
    assert all(p in PLANTS for p in plant), plant
    sm = _Sum(perm_seed)
    z = _product(sm, x["a"].to(dtype), x["w"].to(dtype), product, "w")
    if x.get("bias") is not None:
        z = z + x["bias"].to(dtype)
    add = x["add"].to(dtype) if x.get("add") is not None else 0
    if "add_after_act" in plant:
        return dict(z=z, y=_act(z, int(x.get("act", 0))) + add)
    return dict(z=z + add, y=_act(z + add, int(x.get("act", 0))))


def product_mag(x, wkey="w"):
    """mag = |a| . |w| + |bias| + |add| + |xg| per pre-activation element (float64), the magnitude the step bounds scale with."""
    w = x[wkey].double().abs()
    m = x["a"].double().abs() @ (w.t() if wkey == "wT" else w)
    for k in ("bias", "add", "xg"):
        if x.get(k) is not None:
            m = m + x[k].double().abs()
    return m


def preact_bound(x, product, wkey="w"):
    """b_z per element of the pre-activation (module docstring of tests/test_decode_contract_gpu.py, "step products")."""
    K = x["a"].shape[1]
    mag = product_mag(x, wkey)
    exact = 2 * (K + 4) * U * mag
    if product in ("exact", "one"):
        return exact
    three = torch.minimum(exact + THREE_EPS * mag,
                          torch.full_like(mag, 3e-5 * float(x["a"].abs().max()) * float(x[wkey].abs().max()) * K ** 0.5))
    if product == "three":
        return three
    assert product == "two", product
    return three + 2.0 ** -9 * mag


def cell_bounds(bz, c_prev, h_prev):
    """(b_h, b_c) per element from the pre-activation bound of the four gates (module docstring); bz [N, 4H]."""
    H = c_prev.shape[1]
    b = torch.stack([bz[:, j * H:(j + 1) * H] for j in range(4)], 0).max(0).values
    b_c = (1.25 + c_prev.abs() / 4) * b + 16 * U * (c_prev.abs() + 2)
    return b / 4 + b_c + 16 * U * (1 + h_prev.abs()), b_c


def dense_bound(bz, z, act):
    """b_y: relu, tanh and softsign are 1-Lipschitz, sigmoid 1/4; the evaluated activations add ACT_EPS, the sum z + add is
    inside mag already."""
    return bz * (0.25 if act == 3 else 1.0) + (ACT_EPS if act in (2, 3) else 2 * U * z.abs() if act == 4 else 0.0)


# ------------------------------------------------------------------------------------------ the two packed layouts
def _bf16_bits(t):
    return t.to(torch.bfloat16)


def split_hi_lo(x):
    """(hi, lo) of common.h's split as bf16 tensors."""
    x = x.float()
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


def pack_rows(a, rows_K):
    """fp32 [N <= 32, K <= ceil32(rows_K)] -> the packed activation rows a kernel reads, as a flat fp32-typed tensor of
    ns_rows32_rows_bytes(rows_K) / 4 elements: [row tile][chunk][lane = (k / 8 % 4) * 16 + n % 16][plane hi | lo][k % 8]."""
    nkc = (rows_K + 31) // 32
    full = torch.zeros(32, nkc * 32)
    full[:a.shape[0], :a.shape[1]] = a.float()
    hi, lo = split_hi_lo(full)
    planes = torch.stack([hi, lo], 0).view(2, 2, 16, nkc, 4, 8)              # [plane, tile, r16, kc, g, j]
    return planes.permute(1, 3, 4, 2, 0, 5).contiguous().view(-1).view(torch.float32)


def unpack_rows(rows, K, N, planes=False):
    """Host-side reading of packed rows -> hi + lo as float64 [N, K] (planes=True: the (hi, lo) pair)."""
    nkc = (K + 31) // 32
    raw = rows.view(torch.bfloat16).float().cpu().numpy().astype(np.float64).reshape(2, nkc, 4, 16, 2, 8)
    pl = [raw[:, :, :, :, p, :].transpose(0, 3, 1, 2, 4).reshape(32, nkc * 32)[:N, :K] for p in (0, 1)]
    return (pl[0], pl[1]) if planes else pl[0] + pl[1]


def _tile_columns(C, cell_units, plant=()):
    """Column of w that lane column r16 of tile t holds, [tiles, 16] (-1 = none): dense 16 t + r16; cell form gate r16 / 4,
    unit 4 t + r16 % 4."""
    tiles = (cell_units + 3) // 4 if cell_units else (C + 15) // 16
    t, r = np.meshgrid(np.arange(tiles), np.arange(16), indexing="ij")
    if not cell_units:
        col = t * 16 + r
        return np.where(col < C, col, -1)
    gate, unit = (r % 4, t * 4 + r // 4) if "cell_tile_order" in plant else (r // 4, t * 4 + r % 4)
    return np.where(unit < cell_units, gate * cell_units + unit, -1)


def pack_weights(w, cell_units=0, plant=()):
    """fp32 [K, C] -> ns_rows32_pack's layout [tile][chunk][lane = g * 16 + r16][plane][8]: lane (r16, g) holds its column
    at k = 32 kc + 8 g .. + 7; rows past K and columns past C are zero."""
    K, C = w.shape
    nkc = (K + 31) // 32
    cols = _tile_columns(C, cell_units, plant)
    wp = torch.zeros(nkc * 32, C + 1)
    wp[:K, :C] = w.float()
    sel = wp[:, torch.from_numpy(np.where(cols < 0, C, cols)).long()]           # [k, tile, r16]
    hi, lo = split_hi_lo(sel)
    planes = torch.stack([hi, lo], 0).view(2, nkc, 4, 8, cols.shape[0], 16)      # [plane, kc, g, j, tile, r16]
    return planes.permute(4, 1, 2, 5, 0, 3).contiguous().view(-1).view(torch.float32)


def unpack_weights(packed, K, C, cell_units=0, plant=()):
    """The packed weights back as hi + lo, float64 [K, C]."""
    nkc = (K + 31) // 32
    cols = _tile_columns(C, cell_units, plant)
    raw = packed.view(torch.bfloat16).float().cpu().numpy().astype(np.float64).reshape(cols.shape[0], nkc, 4, 16, 2, 8)
    val = (raw[:, :, :, :, 0, :] + raw[:, :, :, :, 1, :]).transpose(1, 2, 4, 0, 3).reshape(nkc * 32, cols.shape[0], 16)
    out = np.zeros((K, C))
    ok = cols >= 0
    out[:, cols[ok]] = val[:K][:, ok]
    return out


# ------------------------------------------------------------------------------------------------ the key transposes
def keys_transpose(x, dtype=torch.float64, perm_seed=None, bf16_storage=False, plant=()):
    """ns_taco2_keys_transpose: keys_t[n, u, t] = keys[n, padl + t, u] for t < T_in and - read from keys_transpose_kernel
    (csrc/attn.hip), the header did not say - exactly 0 in the columns [T_in, Tia).  x: keys [N, Pi, A], Ti, Tia, padl."""
    Ti, Tia, padl = x["Ti"], x["Tia"], x["padl"]
    k = x["keys"].to(dtype)
    out = torch.zeros(k.shape[0], k.shape[2], Tia, dtype=dtype)
    out[:, :, :Ti] = k[:, padl:padl + Ti].transpose(1, 2)
    return out


def keys_transpose_add(x, dtype=torch.float64, perm_seed=None, bf16_storage=False, plant=()):
    """ns_taco2_keys_transpose_add: keys[n, padl + t, u] += keys_t[n, u, t] for t < T_in, one add per element; every other
    row of keys (the pad rows) unchanged; columns [T_in, Tia) of keys_t are not read."""
    Ti, padl = x["Ti"], x["padl"]
    out = x["keys"].to(dtype).clone()
    out[:, padl:padl + Ti] += x["keys_t"].to(dtype)[:, :, :Ti].transpose(1, 2)
    return out
