"""tests/decode_ref.py proven without a GPU: the two decoder loops against the oracle's cells run free with the frame
fed back through the UNFOLDED output projection and prenet (which also proves the fold `folded_feedback` relies on and
pv = values . W1[context rows]); the steps against tests/lstm_ref.py and a plain product; the packed layouts against
each other; then, for every case of tests/test_decode_contract_gpu.py, what its inputs must exercise and that every
planted error leaves the case's bounds; last the ABI of the five parameter blocks and the refusals the headers state."""
import ctypes
import re

import numpy as np
import pytest
import torch

import attn_ref as AR
import decode_ref as R
import lstm_ref
import test_decode_contract_gpu as G
from oracle import taco1_oracle as O1
from oracle import taco2_oracle as O2

f64 = torch.float64


# --------------------------------------------------------------------------------------- the oracle's cells, run free
def _tiny(taco1, N, S, Ti, lengths, kw, Dsp, clip, seed, A=8, E=6, D=10, D1=12, D2=6, M=5, r=2):
    """Oracle parameters at small widths and the ABI operands built from the same numbers."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=f64)
    P = "decoder/"
    XA = D2 + Dsp + A
    p = {P + "decoder_prenet/dense_1/kernel": rn(M + E, D1) * 0.4, P + "decoder_prenet/dense_1/bias": rn(D1) * 0.5,
         P + "decoder_prenet/dense_2/kernel": rn(D1, D2) * 0.4, P + "decoder_prenet/dense_2/bias": rn(D2) * 0.5,
         P + "attention/query_layer/kernel": rn(A, A) * 0.5, P + "attention/attention_v": rn(A),
         P + "output_projection/kernel": rn(D, M * r) * 0.5, P + "output_projection/bias": rn(M * r) * 0.3}
    keys, values = rn(N, Ti, A), rn(N, Ti, E)
    spk = rn(N, Dsp) if Dsp else None
    W1 = p[P + "decoder_prenet/dense_1/kernel"]
    Wp, bp = p[P + "output_projection/kernel"], p[P + "output_projection/bias"]
    x = dict(keys=keys, values=values, pv=values @ W1[M:], W2=p[P + "decoder_prenet/dense_2/kernel"],
             b2=p[P + "decoder_prenet/dense_2/bias"], Wq=p[P + "attention/query_layer/kernel"], v=p[P + "attention/attention_v"],
             lengths=torch.tensor(lengths, dtype=torch.int32), spk=spk, cell_clip=clip,
             wpf=Wp[:, -M:] @ W1[:M], bpf=bp[-M:] @ W1[:M] + p[P + "decoder_prenet/dense_1/bias"])
    f1 = torch.full((N, S + 1, D1), 1e30, dtype=f64)
    f1[:, 1] = p[P + "decoder_prenet/dense_1/bias"]                 # the <GO> frame and the initial context are zeros
    x["f1"] = f1
    if taco1:
        for nm, din, dh in (("attention_gru", D2 + Dsp, A), ("gru_1", D, D), ("gru_2", D, D)):
            p[P + nm + "/gates/kernel"], p[P + nm + "/gates/bias"] = rn(din + dh, 2 * dh) * 0.4, rn(2 * dh) * 0.3
            p[P + nm + "/candidate/kernel"], p[P + nm + "/candidate/bias"] = rn(din + dh, dh) * 0.4, rn(dh) * 0.3
        p[P + "attention_projection/kernel"], p[P + "attention_projection/bias"] = rn(A + E, D) * 0.4, rn(D) * 0.3
        x.update(Wg=p[P + "attention_gru/gates/kernel"], bg=p[P + "attention_gru/gates/bias"], Wc=p[P + "attention_gru/candidate/kernel"],
                 bc=p[P + "attention_gru/candidate/bias"], w_proj=p[P + "attention_projection/kernel"],
                 b_proj=p[P + "attention_projection/bias"])
        for i in (1, 2):
            x.update({"wg_%d" % i: p[P + "gru_%d/gates/kernel" % i], "bg_%d" % i: p[P + "gru_%d/gates/bias" % i],
                      "wc_%d" % i: p[P + "gru_%d/candidate/kernel" % i], "bc_%d" % i: p[P + "gru_%d/candidate/bias" % i]})
    else:
        p[P + "attention_lstm/kernel"], p[P + "attention_lstm/bias"] = rn(XA, 4 * A) * 0.8, rn(4 * A) * 0.3
        p[P + "lstm_1/kernel"], p[P + "lstm_1/bias"] = rn(A + E + D, 4 * D) * 0.6, rn(4 * D) * 0.3
        p[P + "lstm_2/kernel"], p[P + "lstm_2/bias"] = rn(2 * D, 4 * D) * 0.6, rn(4 * D) * 0.3
        p[P + "attention/location_conv/kernel"], p[P + "attention/location_layer/kernel"] = rn(kw, 1, 4), rn(4, A)
        x.update(Watt=p[P + "attention_lstm/kernel"], batt=p[P + "attention_lstm/bias"], w_l1=p[P + "lstm_1/kernel"],
                 b_l1=p[P + "lstm_1/bias"], w_l2=p[P + "lstm_2/kernel"], b_l2=p[P + "lstm_2/bias"],
                 Wcl=p[P + "attention/location_conv/kernel"][:, 0, :] @ p[P + "attention/location_layer/kernel"])
    return p, x, M


def _oracle_free(taco1, p, x, M, S):
    """tacotron2.py:78-83 / tacotron.py:80-86 under TacoTestHelper from the oracle's cells: the frame goes through the
    output projection and the whole first prenet layer, nothing folded, the context through the whole prenet too."""
    keys, values, L, spk = x["keys"], x["values"], x["lengths"].long(), x["spk"]
    N, A, E = keys.shape[0], keys.shape[2], values.shape[2]
    D = x["wpf"].shape[0]
    Dd = "decoder"
    z = lambda w: torch.zeros(N, w, dtype=f64)
    h, c, h1, c1, h2, c2, ctx, frame, align = z(A), z(A), z(D), z(D), z(D), z(D), z(E), z(M), z(keys.shape[1])
    out = dict(hc=[], align=[], last=[])
    O2.CELL_CLIP = float(x["cell_clip"]) or None
    try:
        for s in range(S):
            pre = O2.prenet(torch.cat([frame, ctx], -1), p, Dd + "/decoder_prenet")
            if spk is not None:
                pre = torch.cat([pre, spk], -1)
            if taco1:
                h = O1.gru_cell(pre, h, *(p[Dd + "/attention_gru/" + k] for k in ("gates/kernel", "gates/bias", "candidate/kernel", "candidate/bias")))
                align = O1.bahdanau_alignments(h, keys, L, p, Dd + "/attention")
            else:
                c, h = O2.lstm_block_cell(pre, c, h, p[Dd + "/attention_lstm/kernel"], p[Dd + "/attention_lstm/bias"])
                align = O2.location_sensitive_alignments(h, align, keys, L, p, Dd + "/attention")
            ctx = (align[:, :, None] * values).sum(1)
            if taco1:
                x1 = torch.cat([h, ctx], -1) @ p[Dd + "/attention_projection/kernel"] + p[Dd + "/attention_projection/bias"]
                h1 = O1.gru_cell(x1, h1, *(p[Dd + "/gru_1/" + k] for k in ("gates/kernel", "gates/bias", "candidate/kernel", "candidate/bias")))
                y1 = x1 + h1
                h2 = O1.gru_cell(y1, h2, *(p[Dd + "/gru_2/" + k] for k in ("gates/kernel", "gates/bias", "candidate/kernel", "candidate/bias")))
                last = y1 + h2
            else:
                c1, h1 = O2.lstm_block_cell(torch.cat([h, ctx], -1), c1, h1, p[Dd + "/lstm_1/kernel"], p[Dd + "/lstm_1/bias"])
                c2, h2 = O2.lstm_block_cell(h1, c2, h2, p[Dd + "/lstm_2/kernel"], p[Dd + "/lstm_2/bias"])
                last = h2
            frame = (last @ p[Dd + "/output_projection/kernel"] + p[Dd + "/output_projection/bias"])[:, -M:]
            for k, t in (("hc", h), ("align", align), ("last", last)):
                out[k].append(t)
    finally:
        O2.CELL_CLIP = None
    return {k: torch.stack(t, 1) for k, t in out.items()}


@pytest.mark.parametrize("taco1", [False, True], ids=["taco2", "taco1"])
@pytest.mark.parametrize("kw,Dsp,lengths,clip", [(7, 0, (9, 5), 0.0), (8, 3, (9, 1), 0.3), (5, 0, (7,), 0.0)])
def test_decode_loops_match_the_oracles_run_free(taco1, kw, Dsp, lengths, clip):
    S = 6
    p, x, M = _tiny(taco1, len(lengths), S, 9, lengths, kw, Dsp, 0.0 if taco1 else clip, seed=kw + Dsp)
    want = _oracle_free(taco1, p, x, M, S)
    got = (R.taco1_decode if taco1 else R.taco2_decode)(x)
    for k, mine in (("hc", "hc"), ("align", "align"), ("last", "y2" if taco1 else "h2")):
        err = float((got[mine][:, 1:] - want[k]).abs().max())
        assert err < 1e-12, (k, err)
        assert float(got[mine][:, 0].abs().max()) == 0.0
    if clip and not taco1:
        assert all(bool(got[k].any()) for k in ("clip_a", "clip_1", "clip_2")), "the clip never acted in the oracle comparison"


# ----------------------------------------------------------------------------------------------------- the steps
@pytest.mark.parametrize("clip,fb", [(0.0, 1.0), (0.4, 0.0)])
def test_step_references_are_lstm_seq_one_step_at_a_time(clip, fb):
    g = torch.Generator().manual_seed(3)
    N, Kx, H = 4, 6, 8
    xin, Wx, W, b = torch.randn(N, 2, Kx, generator=g), torch.randn(Kx, 4 * H, generator=g), torch.randn(H, 4 * H, generator=g), torch.randn(4 * H, generator=g)
    seq = lstm_ref.lstm_seq(xin.double() @ Wx.double() + b.double(), W, forget_bias=fb, cell_clip=clip)
    full = torch.cat([Wx, W], 0)
    zero = torch.zeros(N, H)
    for t, (hp, cp) in enumerate(((zero, None), (seq["h"][:, 0], seq["c"][:, 0]))):
        a = torch.cat([xin[:, t].double(), hp.double()], 1)
        one = R.lstm_step(dict(a=a, wT=full.t(), bias=b, c_prev=cp, forget_bias=fb, cell_clip=clip))
        two = R.rows32_cell(dict(a=a, w=full, bias=b, c_prev=cp, forget_bias=fb, cell_clip=clip), product="exact")
        # the same with the input product hoisted into xg, as ns_lstm_step takes it
        three = R.lstm_step(dict(a=hp.double(), wT=W.t(), xg=xin[:, t].double() @ Wx.double(), bias=b, c_prev=cp, forget_bias=fb, cell_clip=clip))
        for got in (one, two, three):
            assert float((got["h"] - seq["h"][:, t]).abs().max()) < 1e-13 and float((got["c"] - seq["c"][:, t]).abs().max()) < 1e-13
    if clip:
        assert bool(one["clipped"].any())


def test_zoneout_expectation_and_dense_form_are_what_the_header_says():
    g = torch.Generator().manual_seed(5)
    N, K, H = 3, 8, 4
    a, w, cp, hp = (torch.randn(*s, generator=g, dtype=f64) for s in ((N, K), (K, 4 * H), (N, H), (N, H)))
    plain = R.rows32_cell(dict(a=a, w=w, c_prev=cp), product="exact")
    zone = R.rows32_cell(dict(a=a, w=w, c_prev=cp, h_prev=hp, zoneout_cell=0.1, zoneout_output=0.3), product="exact")
    assert torch.allclose(zone["c"], 0.1 * cp + 0.9 * plain["c"], atol=1e-15) and torch.allclose(zone["h"], 0.3 * hp + 0.7 * plain["h"], atol=1e-15)
    bias, add = torch.randn(4 * H, generator=g, dtype=f64), torch.randn(N, 4 * H, generator=g, dtype=f64)
    for act, fn in ((0, lambda t: t), (1, torch.relu), (2, torch.tanh)):
        y = R.rows32_dense(dict(a=a, w=w, bias=bias, add=add, act=act), product="exact")["y"]
        want = fn(torch.from_numpy(a.numpy() @ w.numpy()) + bias + add)
        assert float((y - want).abs().max()) < 1e-14
    # the three-pass arrangement is within the split's truncation of the product, the one-pass one is the rounded operands'
    mag = a.abs() @ w.abs()
    assert bool(((R.rows32_dense(dict(a=a, w=w), product="three")["y"] - a @ w).abs() <= R.THREE_EPS * mag).all())
    assert torch.equal(R.rows32_dense(dict(a=a, w=w), product="one")["y"], AR.bf16(a) @ AR.bf16(w))


# --------------------------------------------------------------------------------------------------- the layouts
def test_split_keeps_sixteen_bits():
    """common.h: hi = bf16(x) keeps 8 significand bits (|x - hi| <= 2^-8 |x|), lo = bf16(x - hi) the next 8: hi + lo
    is x to 2^-16 |x| (decode_ref.SPLIT_EPS) - and not to 2^-17 for every value."""
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.randn(4096, generator=g), torch.randn(4096, generator=g) * 1e-3, torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -17])])
    hi, lo = R.split_hi_lo(x)
    err = (x.double() - hi.double() - lo.double()).abs()
    assert bool((err <= R.SPLIT_EPS * x.double().abs()).all())
    assert bool(((x.double() - hi.double()).abs() <= 2.0 ** -8 * x.double().abs()).all())
    assert float((err / x.double().abs()).max()) > 2.0 ** -18


@pytest.mark.parametrize("N,K,wide", [(1, 8, 8), (17, 40, 104), (32, 264, 264)])
def test_packed_rows_round_trip(N, K, wide):
    g = torch.Generator().manual_seed(N + K)
    a = torch.randn(N, K, generator=g)
    host = torch.zeros(32, (wide + 31) // 32 * 32)
    col = (wide - K) // 32 * 32
    host[:N, col:col + K] = a
    rows = R.pack_rows(host, wide)
    assert rows.numel() * 4 == 2 * ((wide + 31) // 32) * 64 * 32          # ns_rows32_rows_bytes
    back = R.unpack_rows(rows, wide, 32)
    assert np.abs(back[:N, col:col + K] - a.double().numpy()).max() <= R.SPLIT_EPS * float(a.abs().max())
    back[:N, col:col + K] = 0
    assert np.abs(back).max() == 0
    # element (n, k) sits where ns_rows32_store puts it (common.h)
    raw = rows.view(torch.bfloat16)
    nkc = (wide + 31) // 32
    for n, k in ((0, col), (N - 1, col + K - 1)):
        i16 = (((n >> 4) * nkc + (k >> 5)) * 64 + ((k >> 3) & 3) * 16 + (n & 15)) * 2
        hi, lo = R.split_hi_lo(host[n, k])
        assert raw[i16 * 8 + (k & 7)] == hi and raw[(i16 + 1) * 8 + (k & 7)] == lo


@pytest.mark.parametrize("K,C,H", [(8, 16, 0), (40, 72, 0), (264, 80, 20), (40, 16, 4)])
def test_packed_weights_round_trip(K, C, H):
    g = torch.Generator().manual_seed(K + C)
    w = torch.randn(K, C, generator=g)
    packed = R.pack_weights(w, H)
    assert packed.numel() * 4 == ((C + 15) // 16) * ((K + 31) // 32) * 64 * 32     # ns_rows32_packed_bytes
    assert np.abs(R.unpack_weights(packed, K, C, H) - w.double().numpy()).max() <= R.SPLIT_EPS * float(w.abs().max())
    # lane (r16, g) of tile t, chunk kc holds k = 32 kc + 8 g + j of its column: rows32_pack_kernel's index
    raw = packed.view(torch.bfloat16)
    nkc = (K + 31) // 32
    tile, kc, r16, gq, j = (C + 15) // 16 - 1, nkc - 1, 5, 0, 3
    col = (r16 >> 2) * H + tile * 4 + (r16 & 3) if H else tile * 16 + r16
    k = kc * 32 + gq * 8 + j
    want = w[k, col] if k < K and col < C and (not H or tile * 4 + (r16 & 3) < H) else torch.tensor(0.0)
    i = ((tile * nkc + kc) * 64 + gq * 16 + r16) * 2
    assert raw[i * 8 + j] == R.split_hi_lo(want)[0]
    if H:
        assert not torch.equal(packed, R.pack_weights(w, H, plant=("cell_tile_order",)))


def test_key_transposes():
    keys = torch.arange(2 * 6 * 3, dtype=f64).reshape(2, 6, 3)
    kt = R.keys_transpose(dict(keys=keys, Ti=3, Tia=8, padl=2))
    assert kt.shape == (2, 3, 8) and float(kt[:, :, 3:].abs().max()) == 0 and kt[1, 2, 1] == keys[1, 3, 2]
    back = R.keys_transpose_add(dict(keys=keys, keys_t=kt, Ti=3, padl=2))
    assert torch.equal(back[:, 2:5], 2 * keys[:, 2:5]) and torch.equal(back[:, :2], keys[:, :2]) and torch.equal(back[:, 5:], keys[:, 5:])


# ------------------------------------------------------------------------- what the GPU cases' inputs must exercise
@pytest.mark.parametrize("c", G.LOOP_CASES, ids=G.loop_id)
def test_loop_inputs_exercise_what_the_cases_are_for(c):
    x, pure, emu32, _ = G.loop_inputs(c)
    refs = G.loop_references(c)
    for k in G.loop_names(c):
        assert bool(torch.isfinite(emu32[k]).all()), k
    for got, need in G.loop_kink_margin(c, pure, emu32).values():
        assert got >= need
    for zk in ("z1", "z2"):
        z = pure[zk][:, 1:]
        assert bool((z > 0).any()) and bool((z < 0).any()), "%s: every ReLU on the same side" % zk
    for n, L in enumerate(c.lengths):
        if L > 1:
            assert bool(((pure["align"][n, 1:] > 1e-3).sum(-1) > 1).all()), "row %d: a one-hot alignment hides tap and mask errors" % n
        assert float(pure["align"][n, 1:, L:].abs().max() if L < c.Ti else 0) == 0
    if c.clip > 0:
        assert all(bool(pure[k].any()) for k in ("clip_a", "clip_1", "clip_2")), "the clip does not act on every LSTM"
    if c.dtype == G.bf:
        assert all(len(refs["bounds"][k]) == 2 for k in G.loop_names(c))


LOOP_PLANT_CASES = {
    # plant -> the case meant to catch it (family, name, N)
    "ctx_term_stale": [("decode2", "A64-s9t9-clip", 2), ("decode1", "n2s9t20-spk", 2)],
    "l2_hprev_is_input": [("decode2", "A64-s2t9-kw8-spk", 1), ("decode1", "n3s2t9", 3)],
    "no_forget_bias_l2": [("decode2", "A64-s9t9-kw8-spk", 2), ("decode2", "A256-s3t37", 1)],
    "gates_ifjo": [("decode2", "A64-s1t9", 1)],
    "clip_attention_only": [("decode2", "A64-s9t9-clip", 1), ("decode2", "A256-s3t37-clip", 2)],
    "no_residual_y1": [("decode1", "n1s1t9", 1)],
    "gru_rh_stale": [("decode1", "n5s2t13-spk", 5), ("decode1", "n17s2t5", 17)],
    "second_row_first_length": [("decode2", "A64-s1t9", 2), ("decode2", "A64-s2t256", 2), ("decode1", "n2s2t256", 2), ("decode1", "n17s2t5", 17)],
    "mask_len_plus1": [("decode2", "A64-s2t256", 2), ("decode1", "n3s2t9", 3)],
    "even_kw_pad_left": [("decode2", "A64-s2t9-kw8-spk", 2), ("decode2", "A64-s2t256-kw8", 1)],
    "no_speaker_rows": [("decode2", "A64-s2t9-kw8-spk", 2), ("decode1", "n5s2t13-spk", 5)],
    "feedback_from_l1": [("decode2", "A64-s2t9-kw8-spk", 1), ("decode1", "n3s2t9", 3)],
}


def _loop_caught(c, plant):
    """The largest (planted - reference) / bound over the compared buffers, for each reference the case is held against."""
    x, pure, _, _ = G.loop_inputs(c)
    refs = G.loop_references(c)
    fn = G._loop_fn(c)
    worst = 0.0
    for against in ("pure", "exact") if c.dtype == G.bf else ("pure",):
        bad = fn(x, bf16_storage=against == "exact", plant=(plant,))
        ratio = 0.0
        for k in G.loop_names(c):
            bmax = [b for b in refs["bounds"][k] if b[0] == against][0][1]
            ratio = max(ratio, G._dist(G._cut(bad[k]), G._cut(refs[against][k]))[0] / bmax)
        worst = ratio if against == "pure" else min(worst, ratio)          # a kernel with the error fails if EITHER check does
    return worst


@pytest.mark.parametrize("plant", R.LOOP_PLANTS)
def test_planted_loop_errors_leave_the_bounds(plant):
    for family, name, N in LOOP_PLANT_CASES[plant]:
        for c in (c for c in G.LOOP_CASES if (c.family, c.name, c.N) == (family, name, N)):
            ratio = _loop_caught(c, plant)
            print("%s in %s: %.1f bounds" % (plant, G.loop_id(c), ratio))
            if c.dtype == G.bf and c.Ti == 256 and plant in ("second_row_first_length", "mask_len_plus1"):
                continue            # one position of 256 moves align by less than a bf16 flip: the fp32 twin is the case meant to catch it
            assert ratio > (2.0 if c.dtype == G.f32 else 1.0), (plant, G.loop_id(c), ratio)


def test_every_plant_has_its_case():
    assert set(LOOP_PLANT_CASES) == set(R.LOOP_PLANTS) and len(R.PLANTS) >= 10


def _signs(t, seed):
    return torch.where(torch.rand(t.shape, generator=torch.Generator().manual_seed(seed)) < 0.5, -1.0, 1.0).double()


@pytest.mark.parametrize("c", G.ROWS_CASES, ids=G.rows_id)
def test_rows32_bounds_carry_the_preactivation_bound(c):
    """Moving z by +-b_z with random signs moves the reference by less than the h / c / y bounds; the planted errors that
    apply leave them."""
    x, ref, bounds = G.rows_reference(c)
    product = "exact" if c.passes == 3 else "one"
    xb = dict(x, a=AR.bf16(x["a"]), w=AR.bf16(x["w"])) if c.passes == 1 else x
    bz = R.preact_bound(xb, "three" if c.passes == 3 else "one")
    assert bool((bz > 0).all()) and bool(torch.isfinite(bz).all())
    shift = bz * _signs(bz, c.N + c.K)
    if c.cell:
        moved = R._cell_step(ref["z"] + shift, x, c.CH, f64, (), lambda t: t)
        assert bool(((moved["h"] - ref["h"]).abs() < bounds["h"]).all()) and bool(((moved["c"] - ref["c"]).abs() < bounds["c"]).all())
        o = G.CELL_OPTS[c.opt]
        plants = ["gates_ifjo", "cell_tile_order"] + (["zoneout_swapped"] if o.get("zoneout") else []) + \
                 (["forget_bias_one"] if o.get("forget_bias", 1.0) != 1.0 else []) + (["c_prev_ignored"] if o.get("c_prev", True) else []) + \
                 (["clip_after_zoneout"] if o.get("zoneout") and o.get("clip") else [])
        for plant in plants:
            if plant == "cell_tile_order":       # the weights read back through the wrong tile order
                bad = R.rows32_cell(dict(x, w=torch.from_numpy(R.unpack_weights(R.pack_weights(x["w"], c.CH, plant=(plant,)), c.K, 4 * c.CH, c.CH))),
                                    product=product)
            else:
                bad = R.rows32_cell(x, product=product, plant=(plant,))
            r = max(float(((bad[k] - ref[k]).abs() / bounds[k]).max()) for k in ("h", "c"))
            assert r > 2.0, (plant, r)
        if o.get("clip"):
            assert bool(ref["clipped"].any()), "the clip does not act"
    else:
        y = R._act(ref["z"] + shift, x["act"])
        assert bool(((y - ref["y"]).abs() <= bounds["y"] * (1 + 1e-9)).all())
        if x["add"] is not None and x["act"]:
            bad = R.rows32_dense(x, product=product, plant=("add_after_act",))
            assert float(((bad["y"] - ref["y"]).abs() / bounds["y"]).max()) > 2.0


@pytest.mark.parametrize("c", G.STEP_CASES, ids=G.step_id)
def test_lstm_step_bounds_carry_the_preactivation_bound(c):
    x, ref, bounds, passes = G.step_reference(c)
    product = {0: "exact", 1: "one", 2: "two", 3: "three"}[passes]
    xb = dict(x, a=AR.bf16(x["a"]), wT=AR.bf16(x["wT"])) if passes == 1 else x
    bz = R.preact_bound(xb, product, "wT")
    moved = R._cell_step(ref["z"] + bz * _signs(bz, c.N + c.H), x, c.H, f64, (), lambda t: t)
    assert bool(((moved["h"] - ref["h"]).abs() < bounds["h"]).all()) and bool(((moved["c"] - ref["c"]).abs() < bounds["c"]).all())
    # the arrangement the kernel runs stays inside its own bound of the reference it is held against
    if passes in (2, 3):
        run = R.lstm_step(x, product=product)
        assert bool(((run["z"] - ref["z"]).abs() <= bz).all())
    o = G.STEP_OPTS[c.opt]
    plants = ["gates_ifjo"] + (["forget_bias_one"] if x["forget_bias"] != 1.0 and x["c_prev"] is not None else []) + (["zoneout_swapped"] if o.get("zoneout") else []) + \
             (["c_prev_ignored"] if o.get("c_prev", True) else []) + (["clip_after_zoneout"] if o.get("zoneout") and o.get("clip") else [])
    for plant in plants:
        bad = R.lstm_step(x, product="one" if passes == 1 else "exact", plant=(plant,))
        r = max(float(((bad[k] - ref[k]).abs() / bounds[k]).max()) for k in ("h", "c"))
        assert r > 2.0, (plant, G.step_id(c), r)
    if o.get("clip"):
        assert bool(ref["clipped"].any()), "the clip does not act"


def test_tables_reach_every_form():
    assert sorted({G.rows32_key(c.N, c.K, c.cell, c.apk, c.passes) for c in G.ROWS_CASES}) == G.ALL_ROWS32_KEYS and len(G.ALL_ROWS32_KEYS) == 32
    for vals, got in (((8, 40, 264, 520, 1032, 2080), {c.K for c in G.ROWS_CASES}), ((1, 16, 17, 32), {c.N for c in G.ROWS_CASES}),
                      ((16, 72), {c.CH for c in G.ROWS_CASES if not c.cell}), ((4, 20, 64), {c.CH for c in G.ROWS_CASES if c.cell})):
        assert set(vals) == got
    assert {(c.cell, c.opt) for c in G.ROWS_CASES} == {(1, i) for i in range(len(G.CELL_OPTS))} | {(0, i) for i in range(len(G.DENSE_OPTS))}
    assert {(c.form, G.step_tiling(c.N, c.H)) for c in G.STEP_CASES} == {(f, t) for f in G.STEP_FORMS for t in ("big", "half")}
    assert {c.K for c in G.STEP_CASES} == {40, 392} and {c.opt for c in G.STEP_CASES} == set(range(len(G.STEP_OPTS)))
    d2 = [c for c in G.LOOP_CASES if c.family == "decode2"]
    assert {(c.A, c.N, c.dtype) for c in d2} == {(A, N, t) for A in (64, 256) for N in (1, 2) for t in (G.f32, G.bf)}
    assert {c.S for c in d2 if c.A == 64} == {1, 2, 9} and {c.kw for c in d2} == {7, 8} and {c.Dsp for c in d2} == {0, 16}
    d1 = [c for c in G.LOOP_CASES if c.family == "decode1"]
    assert {c.N for c in d1} == {1, 2, 3, 5, 17} and {c.E % 16 for c in d1} == {8} and {c.E for c in d1} == {8, 24} and {c.S for c in d1} == {1, 2, 9}


# -------------------------------------------------------------------------------------------------------- the ABI
def _header_fields(name):
    src = open(G_header()).read()
    body = re.search(r"typedef\s+struct\s*\{((?:(?!typedef).)*?)\}\s*%s\s*;" % name, src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.match(r"(?:const\s+)?\w+\s*\*?\s*(.+)$", decl)
            names += [n.strip().lstrip("* ") for n in m.group(1).split(",")]
    return names


def G_header():
    from nspeech_amd import _lib
    return _lib.HEADER_PATH


@pytest.mark.parametrize("name,first,last", [("ns_taco2_decode_params", ("att", "D", "w_l1", "b_l1", "w_l2", "b_l2", "wpf", "bpf", "h2"), "h2"),
                                             ("ns_taco1_decode_params", ("att", "D", "values", "w_proj", "b_proj", "wg_1", "bg_1", "wc_1", "bc_1"), "y2"),
                                             ("ns_lstm_step_params", ("dtype", "N", "H", "K", "a", "a_sn", "wT", "xg", "xg_sn", "bias"), "cell_clip"),
                                             ("ns_rows32_params", ("N", "K", "C", "a", "a_sn", "a_rows", "a_rows_K", "a_rows_col", "packed", "f32_passes"), "cell_clip"),
                                             ("ns_attention_step_params", ("dtype", "N", "Ti", "Pi", "padl_i", "Tia", "A", "E", "kw", "lengths"), "ctx_rows_col")])
def test_field_order_of_the_parameter_blocks(name, first, last):
    from nspeech_amd import _lib
    got = [f[0] for f in _lib.STRUCTS[name]._fields_]
    assert got == _header_fields(name), name
    assert tuple(got[:len(first)]) == first and got[-1] == last


def _dec2(**kw):
    from nspeech_amd import _lib
    one = ctypes.c_void_p(64)
    q = _lib.struct("ns_taco2_decode_params")
    base = dict(dtype=0, N=2, S=3, Ti=9, Pi=14, padl_i=2, Tia=16, A=64, E=64, D1=256, D2=128, kw=7)
    base.update({k: v for k, v in kw.items() if k != "D"})
    for k, v in base.items():
        setattr(q.att, k, v)
    for k in ("lengths", "keys", "values", "f1", "pv", "w2", "watt", "wq", "b2", "batt", "wcl", "v", "p1", "xa", "hc", "ca", "ga", "q", "align"):
        setattr(q.att, k, one)
    q.D = kw.get("D", 64)
    for k in ("w_l1", "b_l1", "w_l2", "b_l2", "wpf", "bpf", "h2"):
        setattr(q, k, one)
    return q


def _dec1(**kw):
    from nspeech_amd import _lib
    one = ctypes.c_void_p(64)
    q = _lib.struct("ns_taco1_decode_params")
    base = dict(dtype=0, N=2, S=3, Ti=9, Pi=14, padl_i=2, Tia=16, A=256, E=8, D1=256, D2=128)
    base.update({k: v for k, v in kw.items() if k != "D"})
    for k, v in base.items():
        setattr(q.att, k, v)
    for k in ("lengths", "keys", "pv", "f1", "w2", "wg", "wc", "wq", "b2", "bg", "bc", "v", "p1", "xa", "xc", "hc", "ru", "cc", "q", "align"):
        setattr(q.att, k, one)
    q.D = kw.get("D", 256)
    for k in ("values", "w_proj", "b_proj", "wg_1", "bg_1", "wc_1", "bc_1", "wg_2", "bg_2", "wc_2", "bc_2", "wpf", "bpf", "y2"):
        setattr(q, k, one)
    return q


def test_decode_entries_refuse_what_their_headers_say_without_a_launch():
    from nspeech_amd import _lib
    lib = _lib.lib()
    for name in ("ns_taco2_decode", "ns_taco1_decode"):
        assert getattr(lib, name + "_supported")(None) == 0
        fn = getattr(lib, name + "_work_bytes")
        fn.restype = ctypes.c_size_t
        assert fn(None) == 0
        null = _lib.struct(name + "_params")
        assert getattr(lib, name + "_supported")(ctypes.byref(null)) == 0
    work = ctypes.create_string_buffer(64)
    s2, s1 = lib.ns_taco2_decode_supported, lib.ns_taco1_decode_supported
    # (without a device the library assumes 256 CUs, so the supported shapes say 1 here too)
    assert s2(ctypes.byref(_dec2())) == 1 and s2(ctypes.byref(_dec2(N=1))) == 1
    assert s2(ctypes.byref(_dec2(N=3))) == 0
    for A, E, D in ((64, 64, 1024), (64, 512, 64), (256, 64, 64), (256, 512, 64), (128, 128, 128), (64, 16, 64)):
        assert s2(ctypes.byref(_dec2(A=A, E=E, D=D))) == 0, (A, E, D)
    assert s2(ctypes.byref(_dec2(A=256, E=512, D=1024))) == 1
    assert s1(ctypes.byref(_dec1())) == 1
    for D in (128, 255, 512):
        assert s1(ctypes.byref(_dec1(D=D))) == 0
    for entry, q in ((lib.ns_taco2_decode, _dec2(drop_thr=1)), (lib.ns_taco1_decode, _dec1(drop_thr=1)), (lib.ns_taco2_decode, _dec2(N=3)),
                     (lib.ns_taco1_decode, _dec1(D=128))):
        assert entry(ctypes.byref(q), work, None) != 0
        assert b"ns_taco" in lib.ns_last_error()


def test_step_entries_refuse_what_their_headers_say_without_a_launch():
    from nspeech_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(64)

    def rows(**kw):
        p = _lib.struct("ns_rows32_params")
        base = dict(N=4, K=64, C=16, a=one, a_sn=64, packed=one, f32_passes=3, out=one, out_sn=16)
        base.update(kw)
        for k, v in base.items():
            setattr(p, k, v)
        return p
    for bad in (dict(K=60), dict(N=33), dict(N=0), dict(f32_passes=2), dict(f32_passes=0), dict(a=None, a_rows=one, a_rows_K=128, a_rows_col=16),
                dict(a=None, a_rows=one, a_rows_K=64, a_rows_col=32), dict(cell_units=4), dict(out=None), dict(a_sn=62)):
        assert lib.ns_rows32(ctypes.byref(rows(**bad)), None) != 0, bad
        assert b"ns_rows32" in lib.ns_last_error()
    assert lib.ns_rows32_pack(one, ctypes.c_int64(16), 60, 16, 0, one, None) != 0
    assert lib.ns_rows32_pack(one, ctypes.c_int64(8), 64, 16, 0, one, None) != 0          # ldw < C
    assert lib.ns_rows32_pack(one, ctypes.c_int64(24), 64, 24, 5, one, None) != 0         # C != 4 H
    assert lib.ns_rows32_pack_rows(one, ctypes.c_int64(8), 33, 8, one, 32, 0, None) != 0
    assert lib.ns_rows32_pack_rows(one, ctypes.c_int64(8), 4, 8, one, 32, 32, None) != 0    # col0 + K beyond the rows
    for fn, args, want in ((lib.ns_rows32_packed_bytes, (40, 72), 5 * 2 * 64 * 32), (lib.ns_rows32_rows_bytes, (40,), 2 * 2 * 64 * 32),
                           (lib.ns_rows32_packed_bytes, (0, 16), 0), (lib.ns_rows32_rows_bytes, (0,), 0)):
        fn.restype = ctypes.c_size_t
        assert fn(*args) == want

    def step(**kw):
        p = _lib.struct("ns_lstm_step_params")
        base = dict(dtype=0, N=4, H=16, K=40, a=one, a_sn=48, wT=one, h_out=one, h_sn=16, c_out=one, co_sn=16, forget_bias=1.0)
        base.update(kw)
        for k, v in base.items():
            setattr(p, k, v)
        return p
    for bad in (dict(H=24), dict(H=8), dict(a_sn=44), dict(K=36), dict(a=None), dict(c_out=None)):
        assert lib.ns_lstm_step(ctypes.byref(step(**bad)), None) != 0, bad
        assert b"ns_lstm_step" in lib.ns_last_error()
