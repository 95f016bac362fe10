"""Prenet dropout (hparam prenet_dropout; ns_taco2_attn_params.drop_* / ns_taco1_attn_params.drop_* / ns_dropout_rows in
include/nspeech_hip.h) restated on the CPU: the reference the GPU tests compare with, not a test.

The masks, written from the header's comment and csrc/common.h's three lines, not imported from nspeech_amd.ops: unit u
of batch row n at index t of the stream `seed` is DROPPED iff (mix(seed, t, n, u) >> 8) < thr, where
    mix = fmix(fmix(fmix(seed ^ t * 0x9E3779B9) ^ n * 0x7FEB352D) ^ u * 0x846CA68B)        (uint32 wrap-around)
    fmix(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16    (murmur3's finaliser)
and thr = int(rate * 2^24).  t is the decoder step s (0-based: its values live in history slot s + 1; the text position
for Tacotron-1's encoder prenet), n the row of the BATCH, and each of the two layers has a seed of its own.

The recurrences are tests/attn_ref.py's (float64 torch, gradients by autograd, the same storage-exact convention for
bf16 storage and the same permuted float32 evaluation) with
    p1 = relu(z1) * keep1[s] * scale        p2 = relu(z2) * keep2[s] * scale        scale = float32(1 / (1 - rate))
The histories p1 / xa hold the dropped, scaled values; df1 / dp2 are the gradients with respect to z1 / z2, so they carry
keep * scale.  With thr = 0 nothing is multiplied: the functions then ARE attn_ref.taco2 / attn_ref.taco1
(tests/test_prenet_dropout_ref_cpu.py asserts equality).

`plant` names one error a kernel could have (tests/test_prenet_dropout_ref_cpu.py shows that each moves a compared buffer
of the GPU cases by more than ten bounds):
    no_scale_bwd                 the backward pass takes the mask from the saved sign and forgets the factor `scale`
    n_is_group_local             n counts from the first row of the launch group of 32 utterances, not of the batch
    one_stream_for_both_layers   layer 2 draws from layer 1's seed
    t_is_slot_not_step           t = s + 1, the history slot
    scale_before_relu_only_fwd   the forward pass scales the product before the bias (layer 1: before the frame term)
                                 joins it and the ReLU is taken, relu(scale * x.W + b) * keep; the backward pass is the
                                 correct kernel's (sign of the saved output, times scale)

patched_prenet() is the same dropout inside the float64 model oracles (oracle/taco2_oracle.py, taco1_oracle.py: their
module attribute `prenet`, replaced for the duration of a test)."""
import numpy as np
import torch

import attn_ref as R
from attn_ref import _masked_softmax, _Sum, _taps, _valid, bf16

PLANTS = ("no_scale_bwd", "n_is_group_local", "one_stream_for_both_layers", "t_is_slot_not_step", "scale_before_relu_only_fwd")
GROUP = 32          # utterances per launch of ns_taco2_attn_cluster_fwd / _bwd and of the step forms' row blocks


def threshold(rate):
    return int(float(rate) * 16777216.0)


def scale_of(rate):
    """1 / (1 - rate) as the float32 the parameter blocks carry."""
    return float(np.float32(1.0 / (1.0 - float(rate))))


def _fmix(x):
    x = x.astype(np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = (x.astype(np.uint64) * np.uint64(0x85EBCA6B)).astype(np.uint32)
    x = x ^ (x >> np.uint32(13))
    x = (x.astype(np.uint64) * np.uint64(0xC2B2AE35)).astype(np.uint32)
    return x ^ (x >> np.uint32(16))


def _mul(a, c):
    return (a.astype(np.uint64) * np.uint64(c)).astype(np.uint32)


def dropped(seed, thr, T, N, U, t0=0, n0=0):
    """bool [T, N, U]: True where unit u of batch row n0 + n is dropped at index t0 + t."""
    t = (np.arange(T, dtype=np.uint64) + np.uint64(t0)).astype(np.uint32)[:, None, None]
    n = (np.arange(N, dtype=np.uint64) + np.uint64(n0)).astype(np.uint32)[None, :, None]
    u = np.arange(U, dtype=np.uint32)[None, None, :]
    x = _fmix(np.uint32(seed & 0xFFFFFFFF) ^ _mul(t, 0x9E3779B9))
    x = _fmix(x ^ _mul(n, 0x7FEB352D))
    x = _fmix(x ^ _mul(u, 0x846CA68B))
    return (x >> np.uint32(8)) < np.uint32(thr)


def keep_masks(drop, S, N, D1, D2, plant=()):
    """drop = dict(thr, seed1, seed2, scale) -> (keep1 [S, N, D1], keep2 [S, N, D2]) as bool arrays, True = kept."""
    assert all(p in PLANTS for p in plant), plant
    t0 = 1 if "t_is_slot_not_step" in plant else 0
    seed2 = drop["seed1"] if "one_stream_for_both_layers" in plant else drop["seed2"]

    def one(seed, U):
        if "n_is_group_local" in plant:
            return ~np.concatenate([dropped(seed, drop["thr"], S, min(GROUP, N - n0), U, t0=t0) for n0 in range(0, N, GROUP)], 1)
        return ~dropped(seed, drop["thr"], S, N, U, t0=t0)
    return one(drop["seed1"], D1), one(seed2, D2)


class _Layer(object):
    """relu -> keep -> scale of one prenet layer with the plants of the module docstring; a.mm-style product `prod` and
    what joins it before the ReLU (`bias`) come apart for the scale_before_relu_only_fwd plant."""

    def __init__(self, drop, keep, dtype, plant):
        self.on = drop is not None and drop["thr"] != 0
        self.plant = plant
        if self.on:
            self.keep = torch.from_numpy(keep).to(dtype)
            self.scale = float(drop["scale"])

    def __call__(self, s, prod, bias):
        z = prod + bias
        a = torch.relu(z)
        if not self.on:
            return z, a
        k = self.keep[s]
        y = a * k * self.scale
        if "no_scale_bwd" in self.plant:
            y = a * k + (y - a * k).detach()
        if "scale_before_relu_only_fwd" in self.plant:
            y = y + (torch.relu(self.scale * prod + bias) * k - y).detach()
        return z, y


def taco2(x, dhc=None, drop=None, dtype=torch.float64, perm_seed=None, bf16_storage=False, plant=()):
    """attn_ref.taco2 (its plain arrangement: exact products forward and backward) with prenet dropout.  x as there;
    drop = dict(thr, scale, seed1, seed2) or None.  Returns the histories (plus z1, z2) and, with dhc, the gradients."""
    assert all(p in PLANTS for p in plant), plant
    sm = _Sum(perm_seed)
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
    half = (kw - 1) // 2
    valid = _valid(x["lengths"], Ti, ())
    k1, k2 = keep_masks(drop, S1 - 1, N, D1, D2, plant) if drop is not None and drop["thr"] else (None, None)
    layer1, layer2 = _Layer(drop, k1, dtype, plant), _Layer(drop, k2, dtype, plant)
    zero = lambda w: torch.zeros(N, w, dtype=dtype)
    H = dict(p1=[zero(D1)], xa=[zero(D2 + Dsp + A)], hc=[zero(A + E)], ca=[zero(A)], ga=[zero(4 * A)], q=[zero(A)],
             align=[zero(Ti)], z1=[zero(D1)], z2=[zero(D2)])
    kept = dict(z2=[], z=[], q=[], e=[])
    h, c, ctx_term, align = zero(A), zero(A), zero(D1), zero(Ti)
    hcs = []
    for s in range(S1 - 1):
        z1, p1 = layer1(s, ctx_term, f1[:, s + 1])
        z2, p2 = layer2(s, sm.mm(p1, W2, "w2", True), b2)
        xa = torch.cat([p2] + ([spk.to(dtype)] if Dsp else []) + [h], 1)
        z = sm.mm(xa, Watt, "watt", True) + batt
        if bf16_storage:
            h, c = R._CellFromSaved.apply(z, c, clip, bf16)
        else:
            i, j, f, o = torch.sigmoid(z[:, :A]), torch.tanh(z[:, A:2 * A]), torch.sigmoid(z[:, 2 * A:3 * A] + 1.0), torch.sigmoid(z[:, 3 * A:])
            c_raw = f * c + i * j
            c = c_raw + (c_raw.clamp(-clip, clip) - c_raw).detach() if clip > 0 else c_raw
            h = o * torch.tanh(c)
        with torch.no_grad():
            gates = torch.cat([torch.sigmoid(z[:, :A]), torch.tanh(z[:, A:2 * A]), torch.sigmoid(z[:, 2 * A:3 * A] + 1.0),
                               torch.sigmoid(z[:, 3 * A:])], 1)
        q = sm.mm(h, Wq, "wq", True)
        xt = keys + q[:, None, :] + sm.mm(_taps(align, kw, half), Wcl, "wcl")
        e = sm.sum_last(v * torch.tanh(xt), "e")
        align = _masked_softmax(e, valid)
        al_ctx = st(align) if bf16_storage else align
        pt = sm.perm(Ti, "ctx")
        ctx = torch.einsum("nt,nte->ne", al_ctx[:, pt], values[:, pt])
        ctx_term = torch.einsum("nt,nte->ne", align[:, pt], pv[:, pt]) if pv is not None else sm.mm(ctx, W1c, "w1c", True)
        if grad:
            for k_, t_ in (("z2", z2), ("z", z), ("q", q), ("e", e)):
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
    if k1 is not None:
        out["keep1"], out["keep2"] = torch.from_numpy(k1).permute(1, 0, 2), torch.from_numpy(k2).permute(1, 0, 2)      # [N, S, U]
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
    if bf16_storage:            # the hoisted product of the stored alignments and context gradients (attn_ref.taco2)
        if pv is not None:
            df1n = torch.cat([out["df1"][:, 2:], torch.zeros(N, 1, D1, dtype=dtype)], 1)
            dctx = st(dhc.to(dtype)[:, 1:, A:] + bf16(df1n) @ bf16(W1c).t())
        else:
            raise NotImplementedError("bf16 storage comes with the projected-memory form here")
        out["dvalues"] = torch.einsum("nst,nse->nte", bf16(out["align"][:, 1:]), bf16(dctx))
    return out


def taco1(x, dhc=None, drop=None, dtype=torch.float64, perm_seed=None, bf16_storage=False, plant=()):
    """attn_ref.taco1 with prenet dropout, as taco2() above."""
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
    valid = _valid(x["lengths"], Ti, ())
    k1, k2 = keep_masks(drop, S1 - 1, N, D1, D2, plant) if drop is not None and drop["thr"] else (None, None)
    layer1, layer2 = _Layer(drop, k1, dtype, plant), _Layer(drop, k2, dtype, plant)
    zero = lambda w: torch.zeros(N, w, dtype=dtype)
    XA = D2 + Dsp + A
    H = dict(p1=[zero(D1)], xa=[zero(XA)], xc=[zero(XA)], hc=[zero(A + E)], ru=[zero(2 * A)], cc=[zero(A)], q=[zero(A)],
             align=[zero(Ti)], z1=[zero(D1)], z2=[zero(D2)])
    kept = dict(z2=[], zg=[], zc=[], q=[], e=[])
    h, ctx_term = zero(A), zero(D1)
    hcs = []
    for s in range(S1 - 1):
        z1, p1 = layer1(s, ctx_term, f1[:, s + 1])
        z2, p2 = layer2(s, sm.mm(p1, W2, "w2"), b2)
        xin = [p2] + ([spk.to(dtype)] if Dsp else [])
        xa = torch.cat(xin + [h], 1)
        zg = sm.mm(xa, Wg, "wg") + bg
        ru = torch.sigmoid(zg)
        r, u = ru[:, :A], ru[:, A:]
        xc = torch.cat(xin + [r * h], 1)
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
    if k1 is not None:
        out["keep1"], out["keep2"] = torch.from_numpy(k1).permute(1, 0, 2), torch.from_numpy(k2).permute(1, 0, 2)
    if not grad:
        return out
    (torch.stack(hcs, 1) * dhc.to(dtype)[:, 1:]).sum().backward()
    slot = lambda ts: torch.cat([torch.zeros(N, 1, ts[0].shape[1], dtype=dtype), torch.stack([t.grad for t in ts], 1)], 1)
    out["df1"] = st(f1.grad.clone())
    out["df1"][:, 0] = 0
    out["dp2"], out["dzg"], out["dzc"], out["dq"] = (st(slot(kept[k_])) for k_ in ("z2", "zg", "zc", "q"))
    out["de"] = slot(kept["e"])
    return out


def dropout_rows(x, seed, thr, scale, t0=0, n0=0):
    """ns_dropout_rows on x [N, T, U] (float64 arithmetic on x's values): x * keep(seed, t0 + t, n0 + n, u) * float32(scale)."""
    N, T, U = x.shape
    keep = torch.from_numpy(~dropped(seed, thr, T, N, U, t0=t0, n0=n0)).permute(1, 0, 2)
    return x.double() * keep.double() * float(np.float32(scale)), keep


def patched_prenet(O, masks_by_scope, scale):
    """A replacement for the module attribute `prenet` of oracle.taco2_oracle / oracle.taco1_oracle (set it with pytest's
    monkeypatch on the module whose forward is run; O = oracle.taco2_oracle, which owns _relu and the MASK_* aids).
    masks_by_scope: {variable scope: (keep1, keep2)}, bool arrays, True = kept -
        [S, N, U]   for a prenet called once per decoder step with x [N, C]: call number i of a forward pass takes keep[i % S]
        [Ti, N, U]  for a prenet called once with x [N, Ti, C] (Tacotron-1's encoder prenet): keep[t] goes to position t
    A scope that is not in the dict keeps the oracle's identity form.
    Branch bookkeeping (tests/util.py: model_relu_masks reads a prenet ReLU's branch from the STORED p1 / p2, where a
    dropped unit is 0): the entry left in O.MASK_LOG is the oracle's own sign AND keep; under O.MASK_FORCE the forced mask
    already contains the drop, only the scale is left to apply, and a difference between forced and own branch counts for
    O.FLIP_LOG at the kept units only."""
    calls = {}
    scale = float(np.float32(scale))

    def layer(z, keep):
        keep_t = torch.from_numpy(np.ascontiguousarray(keep))
        if O.MASK_FORCE is not None:
            mb = torch.from_numpy(O.MASK_FORCE.pop(0))
            assert mb.shape == z.shape, (mb.shape, z.shape)
            if O.MASK_LOG is not None:
                O.MASK_LOG.append(((z.detach() > 0) & keep_t).numpy())
            if O.FLIP_LOG is not None:
                zd = z.detach()
                fl = ((zd > 0) & keep_t) != mb.bool()
                O.FLIP_LOG.append((int(fl.sum()), float(zd[fl].abs().max()) if bool(fl.any()) else 0.0,
                                   float(zd.pow(2).mean().sqrt()), zd.numel()))
            return z * mb.to(z.dtype) * scale
        y = O._relu(z)
        if O.MASK_LOG is not None:
            O.MASK_LOG[-1] = O.MASK_LOG[-1] & keep
        return y * keep_t.to(z.dtype) * scale

    def prenet(x, p, scope):
        if scope not in masks_by_scope:
            x = O._relu(x @ p[scope + "/dense_1/kernel"] + p[scope + "/dense_1/bias"])
            return O._relu(x @ p[scope + "/dense_2/kernel"] + p[scope + "/dense_2/bias"])
        k1, k2 = masks_by_scope[scope]
        if x.dim() == 2:
            i = calls.get(scope, 0)
            calls[scope] = i + 1
            k1, k2 = k1[i % k1.shape[0]], k2[i % k2.shape[0]]
        else:
            k1, k2 = np.transpose(k1, (1, 0, 2)), np.transpose(k2, (1, 0, 2))
        x = layer(x @ p[scope + "/dense_1/kernel"] + p[scope + "/dense_1/bias"], k1)
        return layer(x @ p[scope + "/dense_2/kernel"] + p[scope + "/dense_2/bias"], k2)
    return prenet
