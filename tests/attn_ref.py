"""The contracts of ns_taco2_attn_params, ns_taco1_attn_params, ns_attention_step_params and
ns_attention_step_bwd_params (include/nspeech_hip.h) restated on torch-CPU in float64: what every attention recurrence
kernel (csrc/attn.hip, attn_cluster.hip, attn_gru.hip) has to compute.  Nothing here is taken from the kernels; the
gradients come from torch.autograd on the forward pass written below (tests/test_attn_ref_cpu.py checks both against
scalar loops and against the oracle's unfolded cells).

Tacotron-2, step s = 0 .. S-1, histories in slot s + 1 of [N, S+1, X] buffers whose slot 0 is zero:
    p1 = relu(f1[s+1] + ctx[s-1] W1c)                  p2 = relu(p1 W2 + b2)
    xa = [p2 | speaker projection | h[s-1]]            z = xa Watt + batt,  gates [i, j, f, o] (LSTMBlockCell)
    c  = sig(f + 1) c[s-1] + sig(i) tanh(j), clipped to +-cell_clip (straight-through gradient);  h = sig(o) tanh(c)
    q  = h Wq
    e[t] = sum_u v[u] tanh(keys[t, u] + q[u] + sum_k align[s-1][t + k - (kw-1)//2] Wcl[k, u])   (zero outside [0, Ti))
    align[s] = softmax of e over t < length (0 from the length on);  ctx[s] = sum_t align[s][t] values[t]
    hc = [h | ctx];  ga holds the gates after their activations (the forget gate after its bias).
Given dhc = dL/dhc: df1 = dL/d(pre-activation of p1) = dL/df1, dp2 = dL/d(pre-activation of p2), dga = dL/dz, dq, de =
dL/de, and the parameter / memory gradients dkeys, dvalues, dv, dwcl.

Tacotron-1 replaces the LSTM by GRUCell ([r | u] = sig([x | h] Wg + bg), c = tanh([x | r h] Wc + bc), h' = u h +
(1 - u) c) and drops the location term; dzg / dzc are the gradients of the two pre-activations.

`dtype` float32 with `perm_seed` is the same arithmetic as an fp32 kernel would do it with every sum taken in another
order: the GPU tests measure with it what fp32 rounding alone costs at a shape (second term of their fp32 rule).

Storage-exact arrangement (`bf16_storage=True`), read off csrc/attn_cluster.hip and csrc/attn_gru.hip with T = bf16:
the operands the caller hands in as bf16 (values, pv and the weight matrices) arrive already rounded; inside the
persistent kernels the recurrent state travels between workgroups as fp32 granules, so nothing the loop reads back was
stored as bf16 in the forward pass - p1, xa, xc, hc and ga are rounded when they are stored and only there.  The
backward kernel reads the SAVED gates (ga; Tacotron-1 keeps ru and cc in fp32) and the saved relu outputs (their sign
only), so its cell derivative is formed from bf16(gates); the contexts hc[:, :, A:] come from bf16(align) (align_t)
after the loop.  Gradient outputs are rounded where they are stored; dvalues is the hoisted product of the stored
(bf16) alignments and context gradients.

One-pass arrangement (`bwd_operand=bf16`, csrc/attn.hip at f32_passes = 1, fp32 storage): every ns_gemm product of the
backward loop - dq . Wq^T, dga . Watt^T (recurrent and prenet rows), dp2 . W2^T, df1 . W1c^T - runs on operands rounded to
bf16, as does the hoisted dvalues product where ns_gemm takes its matrix-core path (`dvalues_rounded`); the attention
kernels themselves (energies, softmax, da, dq sums, post-pass) stay exact fp32.  The models pair it with a THREE-pass
forward (`fwd_three_pass`): the same products forward as lo.hi + hi.lo + hi.hi of the operands' bf16 halves (split3).
That costs 2^-17 of a value - inside the fp32 rule, but 100 times fp32 noise: without it the reference's gate gradients
sit that far from the kernel's and round to another bf16 as a one-pass operand once in a few hundred values.

`plant` is for tests/test_attn_ref_cpu.py only: each name plants one error a kernel could have."""
import torch
import torch.nn.functional as F

PLANTS = ("taps_shifted", "mask_len_plus1", "drop_slice_last", "no_energy_carry", "no_clip_bwd", "no_speaker_rows",
          "gru_rh_is_h", "dwcl_no_padding")
TACO2_HIST = ("p1", "xa", "hc", "ca", "ga", "q", "align")
TACO2_GRAD = ("df1", "dp2", "dga", "dq", "de", "dkeys", "dvalues", "dv", "dwcl")
TACO1_HIST = ("p1", "xa", "xc", "hc", "ru", "cc", "q", "align")
TACO1_GRAD = ("df1", "dp2", "dzg", "dzc", "dq", "de")


def bf16(x):
    """x as a bf16 buffer holds it (round to nearest even), back in x's own type.  Under autograd the rounding is
    straight-through: a kernel that stores a value as bf16 does not round the gradient that later flows past it."""
    y = x.detach().to(torch.bfloat16).to(x.dtype)
    return x + (y - x.detach()) if x.requires_grad else y


def project_memory(values, W1c):
    """pv = values . W1c, the caller-side operand of the projected-memory form."""
    return values.double() @ W1c.double()


def hoisted_da0(dhc, values, A):
    """da0[n, slot, t] = dhc[n, slot, A:] . values[n, t], the caller-side operand of the projected-memory backward."""
    return torch.einsum("nse,nte->nst", dhc.double()[:, :, A:], values.double())


class _Sum(object):
    """Matrix products and sums whose summation index is permuted (perm_seed given) - in float64 that changes nothing
    worth naming, in float32 it is another kernel's summation order."""

    def __init__(self, seed, bwd_operand=None, fwd_three_pass=False):
        self.g = None if seed is None else torch.Generator().manual_seed(seed)
        self.cache = {}
        self.r = bwd_operand
        self.three = fwd_three_pass

    def perm(self, n, tag):
        if (n, tag) not in self.cache:
            self.cache[(n, tag)] = torch.arange(n) if self.g is None else torch.randperm(n, generator=self.g)
        return self.cache[(n, tag)]

    def mm(self, a, w, tag, one_pass=False):
        """a @ w; one_pass marks the products that ns_gemm / the LSTM step kernel run (three split-bf16 passes forward
        with fwd_three_pass, bf16-rounded operands backward with bwd_operand); the rest are exact fp32 FMAs."""
        if self.g is not None:
            p = self.perm(w.shape[0], tag)
            a, w = a[..., p], w[p]
        if one_pass and (self.r is not None or self.three):
            return _KernelProduct.apply(a, w, self.r, self.three)
        return a @ w

    def sum_last(self, x, tag):
        if self.g is None:
            return x.sum(-1)
        return x[..., self.perm(x.shape[-1], tag)].sum(-1)


def split3(a, w):
    """a @ w as three split-bf16 passes (csrc/common.h: mfma_split<3>): hi = bf16(x), lo = bf16(x - hi), the product is
    lo.hi + hi.lo + hi.hi - the lo.lo term and what the two halves do not hold (2^-17 of a value) are left out."""
    ah, wh = bf16(a), bf16(w)
    al, wl = bf16(a - ah), bf16(w - wh)
    return al @ wh + ah @ wl + ah @ wh


class _KernelProduct(torch.autograd.Function):
    """a @ w for a constant w as a kernel arrangement runs it: forward exact or in three split-bf16 passes; the
    gradient with respect to a is r(g) @ r(w)^T (r = the rounding of a one-pass backward, or None)."""

    @staticmethod
    def forward(ctx, a, w, r, three_pass):
        ctx.save_for_backward(w if r is None else r(w))
        ctx.r = r
        return split3(a, w) if three_pass else a @ w

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        return (g if ctx.r is None else ctx.r(g)) @ w.t(), None, None, None


def _taps(a, kw, half):
    """a [N, Ti] -> [N, Ti, kw]: tap k of position t is a[t + k - half], zero outside [0, Ti)."""
    return F.pad(a, (half, kw - 1 - half)).unfold(1, kw, 1)


def _masked_softmax(e, valid):
    return torch.softmax(torch.where(valid, e, torch.full_like(e, -float("inf"))), dim=1)


def _valid(lengths, Ti, plant):
    L = lengths.long() + (1 if "mask_len_plus1" in plant else 0)
    v = torch.arange(Ti)[None, :] < L[:, None]
    if "drop_slice_last" in plant:       # the last position of the first of a row's eight slices of ceil(length / 8)
        v = v.clone()                    # positions never takes part (rows of length 1 have nothing to lose)
        for n, length in enumerate(lengths.tolist()):
            if length > 1:
                v[n, (length + 7) // 8 - 1] = False
    return v


class _CellFromSaved(torch.autograd.Function):
    """The LSTM cell update whose backward forms its derivative from the SAVED (rounded) gates, as a kernel that stores
    them as bf16 does: forward exact, backward from r(i), r(j), r(f), r(o), fp32 c and c_prev."""

    @staticmethod
    def forward(ctx, z, c_prev, clip, r):
        A = c_prev.shape[1]
        i, j, f, o = torch.sigmoid(z[:, :A]), torch.tanh(z[:, A:2 * A]), torch.sigmoid(z[:, 2 * A:3 * A] + 1.0), torch.sigmoid(z[:, 3 * A:])
        c = f * c_prev + i * j
        if clip > 0:
            c = c.clamp(-clip, clip)
        h = o * torch.tanh(c)
        ctx.save_for_backward(r(i), r(j), r(f), r(o), c, c_prev)
        return h, c

    @staticmethod
    def backward(ctx, dh, dc_in):
        i, j, f, o, c, cp = ctx.saved_tensors
        tc = torch.tanh(c)
        dc = dh * o * (1 - tc * tc) + dc_in
        dz = torch.cat([dc * j * i * (1 - i), dc * i * (1 - j * j), dc * cp * f * (1 - f), dh * tc * o * (1 - o)], 1)
        return dz, dc * f, None, None


def taco2(x, dhc=None, dtype=torch.float64, perm_seed=None, bf16_storage=False, bwd_operand=None, dvalues_rounded=True,
          fwd_three_pass=False, plant=()):
    """x: dict of keys [N, Ti, A], values [N, Ti, E], f1 [N, S+1, D1], W1c [E, D1], W2 [D1, D2], b2, Watt [D2+Dsp+A, 4A],
    batt, Wq [A, A], Wcl [kw, A], v [A], lengths [N], cell_clip, spk [N, Dsp] or None, pv [N, Ti, D1] or None (the
    projected memory as the kernel is given it; None = values . W1c inside).  Returns the histories [N, S+1, X] (plus
    z1, z2: the two prenet pre-activations) and, with dhc [N, S+1, A+E], the gradients."""
    assert all(p in PLANTS for p in plant), plant
    sm = _Sum(perm_seed, bwd_operand, fwd_three_pass)
    st = bf16 if bf16_storage else (lambda t: t)
    grad = dhc is not None
    leaf = lambda t: t.to(dtype).clone().requires_grad_(grad)
    keys, values, f1, v, Wcl = leaf(x["keys"]), leaf(x["values"]), leaf(x["f1"]), leaf(x["v"]), leaf(x["Wcl"])
    pv = leaf(x["pv"]) if x.get("pv") is not None else None
    W1c, W2, b2, Watt, batt, Wq = (x[k].to(dtype) for k in ("W1c", "W2", "b2", "Watt", "batt", "Wq"))
    spk = x.get("spk")
    clip = float(x.get("cell_clip", 0.0))
    N, Ti, A = keys.shape
    E, S1, D1, D2 = values.shape[2], f1.shape[1], W1c.shape[1], W2.shape[1]
    Dsp = 0 if spk is None else spk.shape[1]
    kw = Wcl.shape[0]
    half = (kw - 1) // 2 + (1 if "taps_shifted" in plant else 0)
    valid = _valid(x["lengths"], Ti, plant)
    zero = lambda w: torch.zeros(N, w, dtype=dtype)
    H = dict(p1=[zero(D1)], xa=[zero(D2 + Dsp + A)], hc=[zero(A + E)], ca=[zero(A)], ga=[zero(4 * A)], q=[zero(A)],
             align=[zero(Ti)], z1=[zero(D1)], z2=[zero(D2)])
    kept = dict(z2=[], z=[], q=[], e=[], xt=[], ctx=[])
    h, c, ctx_term, align = zero(A), zero(A), zero(D1), zero(Ti)
    hcs = []
    for s in range(S1 - 1):
        z1 = f1[:, s + 1] + ctx_term
        p1 = torch.relu(z1)
        z2 = sm.mm(p1, W2, "w2", True) + b2
        p2 = torch.relu(z2)
        xa = torch.cat([p2] + ([spk.to(dtype)] if Dsp else []) + [h], 1)
        if "no_speaker_rows" in plant and Dsp:
            z = sm.mm(torch.cat([p2, h], 1), torch.cat([Watt[:D2], Watt[D2 + Dsp:]], 0), "watt2", True) + batt
        else:
            z = sm.mm(xa, Watt, "watt", True) + batt
        if bf16_storage:
            h, c = _CellFromSaved.apply(z, c, clip, bf16)
        else:
            i, j, f, o = torch.sigmoid(z[:, :A]), torch.tanh(z[:, A:2 * A]), torch.sigmoid(z[:, 2 * A:3 * A] + 1.0), torch.sigmoid(z[:, 3 * A:])
            c_raw = f * c + i * j
            c = c_raw + (c_raw.clamp(-clip, clip) - c_raw).detach() if clip > 0 else c_raw
            tc = torch.tanh(c)
            if "no_clip_bwd" in plant and clip > 0:      # the value of the clipped cell, the derivative of the unclipped one
                tr = torch.tanh(c_raw)
                tc = tc.detach() + tr - tr.detach()
            h = o * tc
        with torch.no_grad():
            gates = torch.cat([torch.sigmoid(z[:, :A]), torch.tanh(z[:, A:2 * A]), torch.sigmoid(z[:, 2 * A:3 * A] + 1.0),
                               torch.sigmoid(z[:, 3 * A:])], 1)
        q = sm.mm(h, Wq, "wq", True)
        taps = _taps(align.detach() if "no_energy_carry" in plant else align, kw, half)
        xt = keys + q[:, None, :] + sm.mm(taps, Wcl, "wcl")
        e = sm.sum_last(v * torch.tanh(xt), "e")
        align = _masked_softmax(e, valid)
        al_ctx = st(align) if bf16_storage else align
        pt = sm.perm(Ti, "ctx")
        ctx = torch.einsum("nt,nte->ne", al_ctx[:, pt], values[:, pt])
        ctx_term = torch.einsum("nt,nte->ne", align[:, pt], pv[:, pt]) if pv is not None else sm.mm(ctx, W1c, "w1c", True)
        if grad:
            for k_, t_ in (("z2", z2), ("z", z), ("q", q), ("e", e), ("xt", xt), ("ctx", ctx)):
                t_.retain_grad()
                kept[k_].append(t_)
        hc = torch.cat([h, ctx], 1)
        hcs.append(hc)
        for k_, t_ in (("p1", p1), ("xa", xa), ("hc", hc), ("ca", c), ("ga", gates), ("q", q), ("align", align), ("z1", z1),
                       ("z2", z2)):
            H[k_].append(t_.detach())
    out = {k_: torch.stack(t_, 1) for k_, t_ in H.items()}
    for k_ in ("p1", "xa", "hc", "ga"):
        out[k_] = st(out[k_])
    out["valid"] = torch.arange(Ti)[None, :] < x["lengths"].long()[:, None]
    if not grad:
        return out
    (torch.stack(hcs, 1) * dhc.to(dtype)[:, 1:]).sum().backward()
    slot = lambda ts: torch.cat([torch.zeros(N, 1, ts[0].shape[1], dtype=dtype), torch.stack([t.grad for t in ts], 1)], 1)
    out["df1"] = st(f1.grad.clone())
    out["df1"][:, 0] = 0
    out["dp2"], out["dga"], out["dq"] = st(slot(kept["z2"])), st(slot(kept["z"])), st(slot(kept["q"]))
    out["de"] = slot(kept["e"])
    out["dkeys"], out["dv"] = keys.grad, v.grad
    out["dvalues"] = values.grad + (pv.grad @ W1c.t() if pv is not None and pv.grad is not None else 0)
    out["dwcl"] = Wcl.grad
    if bf16_storage or bwd_operand is not None:
        # dvalues is one product after the loop, align_t^T . dctx_t, on bf16 operands (bf16 storage, or one pass where
        # ns_gemm takes its matrix-core path: dvalues_rounded, see the caller): dctx of a
        # slot is dhc's context columns plus the next slot's STORED prenet gradient through W1c (projected-memory form) or
        # what the loop carried (plain form)
        if pv is not None:
            df1n = torch.cat([out["df1"][:, 2:], torch.zeros(N, 1, D1, dtype=dtype)], 1)
            dctx = st(dhc.to(dtype)[:, 1:, A:] + bf16(df1n) @ bf16(W1c).t())
        else:
            dctx = torch.stack([t.grad for t in kept["ctx"]], 1)
        rv = bf16 if bf16_storage or dvalues_rounded else (lambda t: t)
        out["dvalues"] = torch.einsum("nst,nse->nte", rv(out["align"][:, 1:]), rv(dctx))
    if "dwcl_no_padding" in plant:           # the taps at the edges read the nearest alignment instead of zero
        dw = torch.zeros_like(Wcl)
        for s in range(S1 - 1):
            ap = F.pad(out["align"][:, s][:, None, :], (half, kw - 1 - half), mode="replicate")[:, 0].unfold(1, kw, 1)
            dw = dw + torch.einsum("ntk,ntu->ku", ap, kept["xt"][s].grad)
        out["dwcl"] = dw
    return out


def taco1(x, dhc=None, dtype=torch.float64, perm_seed=None, bf16_storage=False, plant=()):
    """x: keys, values, f1, W1c, W2, b2, Wg [D2+Dsp+A, 2A], bg, Wc [D2+Dsp+A, A], bc, Wq, v, lengths, spk or None, pv or
    None.  Histories p1, xa = [p2 | spk | h_prev], xc = [p2 | spk | r h_prev], hc = [h | ctx], ru, cc, q, align."""
    assert all(p in PLANTS for p in plant), plant
    sm = _Sum(perm_seed)
    st = bf16 if bf16_storage else (lambda t: t)
    grad = dhc is not None
    leaf = lambda t: t.to(dtype).clone().requires_grad_(grad)
    keys, values, f1 = leaf(x["keys"]), leaf(x["values"]), leaf(x["f1"])
    pv = leaf(x["pv"]) if x.get("pv") is not None else None
    W1c, W2, b2, Wg, bg, Wc, bc, Wq, v = (x[k].to(dtype) for k in ("W1c", "W2", "b2", "Wg", "bg", "Wc", "bc", "Wq", "v"))
    spk = x.get("spk")
    N, Ti, A = keys.shape
    E, S1, D1, D2 = values.shape[2], f1.shape[1], W1c.shape[1], W2.shape[1]
    Dsp = 0 if spk is None else spk.shape[1]
    valid = _valid(x["lengths"], Ti, plant)
    zero = lambda w: torch.zeros(N, w, dtype=dtype)
    XA = D2 + Dsp + A
    H = dict(p1=[zero(D1)], xa=[zero(XA)], xc=[zero(XA)], hc=[zero(A + E)], ru=[zero(2 * A)], cc=[zero(A)], q=[zero(A)],
             align=[zero(Ti)], z1=[zero(D1)], z2=[zero(D2)])
    kept = dict(z2=[], zg=[], zc=[], q=[], e=[])
    h, ctx_term = zero(A), zero(D1)
    hcs = []
    for s in range(S1 - 1):
        z1 = f1[:, s + 1] + ctx_term
        p1 = torch.relu(z1)
        z2 = sm.mm(p1, W2, "w2") + b2
        p2 = torch.relu(z2)
        xin = [p2] + ([spk.to(dtype)] if Dsp else [])
        xa = torch.cat(xin + [h], 1)
        if "no_speaker_rows" in plant and Dsp:
            zg = sm.mm(torch.cat([p2, h], 1), torch.cat([Wg[:D2], Wg[D2 + Dsp:]], 0), "wg2") + bg
        else:
            zg = sm.mm(xa, Wg, "wg") + bg
        ru = torch.sigmoid(zg)
        r, u = ru[:, :A], ru[:, A:]
        xc = torch.cat(xin + [h if "gru_rh_is_h" in plant else r * h], 1)
        zc = sm.mm(xc, Wc, "wc") + bc
        cc = torch.tanh(zc)
        h = u * h + (1 - u) * cc
        q = sm.mm(h, Wq, "wq")
        e = sm.sum_last(v * torch.tanh(keys + q[:, None, :]), "e")
        align = _masked_softmax(e, valid)
        al_ctx = st(align) if bf16_storage else align
        pt = sm.perm(Ti, "ctx")
        ctx = torch.einsum("nt,nte->ne", al_ctx[:, pt], values[:, pt])
        ctx_term = torch.einsum("nt,nte->ne", align[:, pt], pv[:, pt]) if pv is not None else sm.mm(ctx, W1c, "w1c")
        if grad:
            for k_, t_ in (("z2", z2), ("zg", zg), ("zc", zc), ("q", q), ("e", e)):
                t_.retain_grad()
                kept[k_].append(t_)
        hc = torch.cat([h, ctx], 1)
        hcs.append(hc)
        for k_, t_ in (("p1", p1), ("xa", xa), ("xc", xc), ("hc", hc), ("ru", ru), ("cc", cc), ("q", q), ("align", align),
                       ("z1", z1), ("z2", z2)):
            H[k_].append(t_.detach())
    out = {k_: torch.stack(t_, 1) for k_, t_ in H.items()}
    for k_ in ("p1", "xa", "xc", "hc"):
        out[k_] = st(out[k_])
    out["valid"] = torch.arange(Ti)[None, :] < x["lengths"].long()[:, None]
    if not grad:
        return out
    (torch.stack(hcs, 1) * dhc.to(dtype)[:, 1:]).sum().backward()
    slot = lambda ts: torch.cat([torch.zeros(N, 1, ts[0].shape[1], dtype=dtype), torch.stack([t.grad for t in ts], 1)], 1)
    out["df1"] = st(f1.grad.clone())
    out["df1"][:, 0] = 0
    out["dp2"], out["dzg"], out["dzc"], out["dq"] = (st(slot(kept[k_])) for k_ in ("z2", "zg", "zc", "q"))
    out["de"] = slot(kept["e"])
    return out


def attention_step(keys, values, q, aprev, Wcl, v, lengths, pv=None, dtype=torch.float64, plant=()):
    """One ns_attention_step: energies, masked softmax, context (and the second weighted sum over pv).  Wcl None = no
    location term."""
    keys, values, q, aprev, v = (t.to(dtype) for t in (keys, values, q, aprev, v))
    N, Ti, A = keys.shape
    xt = keys + q[:, None, :]
    if Wcl is not None:
        kw = Wcl.shape[0]
        xt = xt + _taps(aprev, kw, (kw - 1) // 2 + (1 if "taps_shifted" in plant else 0)) @ Wcl.to(dtype)
    e = (v * torch.tanh(xt)).sum(-1)
    align = _masked_softmax(e, _valid(lengths, Ti, plant))
    out = dict(e=e, align=align, ctx=torch.einsum("nt,nte->ne", align, values))
    if pv is not None:
        out["pv_out"] = torch.einsum("nt,nte->ne", align, pv.to(dtype))
    return out


def attention_step_bwd(keys, values, q, aprev, Wcl, v, lengths, dctx_ext, dctx_carry=None, gk_next=None, dtype=torch.float64,
                       plant=()):
    """One ns_attention_step_bwd by autograd.  gk_next [N, Ti, kw] holds, for the step AFTER this one, the gradient of
    the loss with respect to tap k of position t of its location filter's input (this step's alignments); with it
    (has_carry) the alignments receive sum_k gk_next[t - k + half][k] on top of dctx . values.  Returns da, de, dq,
    gk (the same per-tap terms of this step, for the step before) and dctx = dctx_ext + dctx_carry."""
    dt = dtype
    keys, values, v, Wcl = keys.to(dt), values.to(dt), v.to(dt), Wcl.to(dt)
    qg = q.to(dt).clone().requires_grad_(True)
    N, Ti, A = keys.shape
    kw = Wcl.shape[0]
    half = (kw - 1) // 2
    taps = _taps(aprev.to(dt), kw, half).clone().requires_grad_(True)
    e = (v * torch.tanh(keys + qg[:, None, :] + taps @ Wcl)).sum(-1)
    e.retain_grad()
    align = _masked_softmax(e, _valid(lengths, Ti, plant))
    align.retain_grad()
    dctx = dctx_ext.to(dt) + (dctx_carry.to(dt) if dctx_carry is not None else 0)
    loss = (torch.einsum("nt,nte->ne", align, values) * dctx).sum()
    if gk_next is not None and "no_energy_carry" not in plant:
        loss = loss + (_taps(align, kw, half) * gk_next.to(dt)).sum()
    loss.backward()
    valid = _valid(lengths, Ti, plant)
    return dict(da=align.grad * valid, de=e.grad, dq=qg.grad, gk=taps.grad, dctx=dctx, align=align.detach())
