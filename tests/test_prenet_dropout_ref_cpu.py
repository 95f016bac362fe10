"""tests/prenet_dropout_ref.py against itself and against tests/attn_ref.py, on the CPU: with threshold 0 it IS attn_ref
(every history and gradient, bit for bit, in each arrangement the GPU tests use); its autograd gradients agree with
central differences; the masks the GPU cases use drop the share of units their rate says and differ between the two
layers; every planted error moves a buffer that tests/test_prenet_dropout_contract_gpu.py compares by more than ten times
the bound it applies there - on that module's own cases, data seeds and mask seeds; and on the inputs of the model-level
test the masked and the plain oracle differ by the threshold tests/test_prenet_dropout_models_gpu.py then asks of the GPU."""
import math

import numpy as np
import pytest
import torch

import attn_ref as R
import prenet_dropout_ref as PR
import test_attn_contract_gpu as TC
import test_prenet_dropout_contract_gpu as G
import test_prenet_dropout_models_gpu as GM

OFF = dict(thr=0, scale=2.0, seed1=G.SEED1, seed2=G.SEED2)


@pytest.mark.parametrize("dc", G.SMALL + [G._first("cluster2", "A64-bf16", "n4s9t20-spk-clip")], ids=G.dcase_id)
def test_threshold_zero_is_attn_ref(dc):
    c = dc.c
    x, dhc = TC._draw(c, 7)
    taco1 = c.family == "cluster1"
    mine, theirs = (PR.taco1, R.taco1) if taco1 else (PR.taco2, R.taco2)
    arrangements = [dict(), dict(dtype=torch.float32, perm_seed=5)]
    if c.dtype == torch.bfloat16:
        x = dict(x, pv=R.bf16(R.project_memory(x["values"], x["W1c"])))
        arrangements = [dict(bf16_storage=True), dict(bf16_storage=True, dtype=torch.float32, perm_seed=5)]
    for kw in arrangements:
        for drop in (None, OFF):
            a, b = mine(x, dhc, drop=drop, **kw), theirs(x, dhc, **kw)
            for k in TC.hist_names(c) + TC.grad_names(c) + ("z1", "z2"):
                assert torch.equal(a[k], b[k]), (k, kw)


def _tiny(taco1):
    g = torch.Generator().manual_seed(11)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    away = lambda t, lo: torch.sign(t) * (lo + t.abs())
    N, S, Ti, A, E, D1, D2, kw = 2, 2, 3, 4, 3, 6, 4, 3
    XA = D2 + A
    x = dict(keys=r(N, Ti, A), values=r(N, Ti, E), f1=away(r(N, S + 1, D1), 0.5), W1c=r(E, D1) * 0.2, W2=r(D1, D2) * 0.1,
             b2=away(r(D2) * 0.4, 0.6), Wq=r(A, A) * 0.5, v=r(A), lengths=torch.tensor([3, 2], dtype=torch.int32), spk=None,
             cell_clip=0.0)
    x["f1"][:, 0] = 0
    if taco1:
        x.update(Wg=r(XA, 2 * A) * 0.4, bg=r(2 * A) * 0.1, Wc=r(XA, A) * 0.4, bc=r(A) * 0.1)
    else:
        x.update(Watt=r(XA, 4 * A) * 0.4, batt=r(4 * A) * 0.1, Wcl=r(kw, A))
    return x, r(N, S + 1, A + E) * 0.3


@pytest.mark.parametrize("taco1", [False, True], ids=["taco2", "taco1"])
def test_autograd_gradients_agree_with_central_differences(taco1):
    x, dhc = _tiny(taco1)
    fn = PR.taco1 if taco1 else PR.taco2
    drop = G.drop_of(0.5)
    out = fn(x, dhc, drop=drop)
    assert 0 < int((~out["keep1"]).sum()) < out["keep1"].numel()

    def loss(xx):
        o = fn(xx, None, drop=drop)
        return float((o["hc"][:, 1:] * dhc[:, 1:]).sum())

    def fd(name, idx, eps=1e-6):
        hi, lo = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in x.items()}, {k: (v.clone() if torch.is_tensor(v) else v) for k, v in x.items()}
        hi[name][idx] += eps
        lo[name][idx] -= eps
        return (loss(hi) - loss(lo)) / (2 * eps)
    # df1 = dL/df1 (the gradient with respect to the first layer's pre-activation): every element of the live slots
    for idx in np.ndindex(*x["f1"].shape):
        if idx[1] == 0:
            continue
        assert abs(fd("f1", idx) - float(out["df1"][idx])) < 1e-7, ("f1", idx)
    # dp2 = dL/dz2: its sum over rows and steps is dL/db2
    for u in range(x["b2"].shape[0]):
        assert abs(fd("b2", (u,)) - float(out["dp2"][:, :, u].sum())) < 1e-7, ("b2", u)
    if not taco1:
        for name, key in (("keys", "dkeys"), ("values", "dvalues"), ("v", "dv"), ("Wcl", "dwcl")):
            for idx in list(np.ndindex(*x[name].shape))[::3]:
                assert abs(fd(name, idx) - float(out[key][idx])) < 1e-7, (name, idx)


def _mask_sets():
    """(label, dropped bool array, rate) of every mask a GPU case draws."""
    seen = set()
    for dc in G.ALL_DCASES:
        s, c = dc.c.shape, dc.c
        for seeds in ((G.SEED1, G.SEED2),) + (((G.OTHER1, G.OTHER2),) if dc in G.SMALL else ()):
            for seed, U in zip(seeds, (c.D1, c.D2)):
                key = (seed, dc.rate, s.S, s.N, U)
                if key not in seen:
                    seen.add(key)
                    yield "decoder %s" % (key,), PR.dropped(seed, PR.threshold(dc.rate), s.S, s.N, U), dc.rate
    for r in G.ROWS:
        yield "rows %s" % G.rows_id(r), PR.dropped(G.SEED1, PR.threshold(r.rate), r.T, r.N, r.U, t0=r.t0, n0=r.n0), r.rate
    for label, d, rate in GM.mask_sets():
        yield label, d, rate


def test_dropped_share_of_every_gpu_mask_is_the_rate():
    n_sets = 0
    for label, d, rate in _mask_sets():
        p = PR.threshold(rate) / 16777216.0
        sigma = math.sqrt(p * (1 - p) / d.size)
        assert abs(float(d.mean()) - p) <= 4 * sigma, (label, float(d.mean()), p, sigma)
        n_sets += 1
    assert n_sets > 40


def test_the_two_layers_draw_different_masks():
    for dc in G.ALL_DCASES:
        s, c = dc.c.shape, dc.c
        k1, k2 = PR.keep_masks(G.drop_of(dc.rate), s.S, s.N, c.D1, c.D2)
        if k2.size >= 64:            # (n1s1t1 at the step forms' widths has eight units in layer 2)
            assert not np.array_equal(k1[..., :c.D2], k2), G.dcase_id(dc)
    a, b = GM.mask_sets()[:2]
    assert not np.array_equal(a[1][..., :b[1].shape[-1]], b[1])


def test_mask_generator_matches_a_scalar_restatement():
    """dropped() one (t, n, u) at a time in Python integers, indices past 2^8 and a wrapped product included."""
    def fmix(x):
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & 0xFFFFFFFF
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & 0xFFFFFFFF
        return x ^ (x >> 16)
    thr = PR.threshold(0.3)
    d = PR.dropped(G.SEED2, thr, 3, 2, 5, t0=70000, n0=40)
    for t in range(3):
        for n in range(2):
            for u in range(5):
                x = fmix(G.SEED2 ^ (((70000 + t) * 0x9E3779B9) & 0xFFFFFFFF))
                x = fmix(x ^ (((40 + n) * 0x7FEB352D) & 0xFFFFFFFF))
                x = fmix(x ^ ((u * 0x846CA68B) & 0xFFFFFFFF))
                assert bool(d[t, n, u]) == ((x >> 8) < thr)


# plant -> the GPU cases it is shown on: fp32 storage (the fp32 rule's bound), one per family that can have the error;
# n_is_group_local needs a second group of 32 utterances, which a Tacotron-1 launch does not have
def _plant_cases():
    out = []
    for plant in PR.PLANTS:
        grp = plant == "n_is_group_local"
        for family, form in (("cluster2", "A64-f32"), ("step2", "pv-f32x00"), ("step2", "plain-f32x00"), ("cluster1", "f32")):
            if grp and family == "cluster1":
                continue
            for rate in G.RATES:
                out.append((plant, G._first(family, form, "n33s2t9" if grp else "n3s4t9", rate)))
    return out


@pytest.mark.parametrize("plant,dc", _plant_cases(), ids=lambda v: v if isinstance(v, str) else G.dcase_id(v))
def test_every_plant_moves_a_compared_buffer_by_ten_bounds(monkeypatch, plant, dc):
    c = dc.c
    refs = G.dreferences(dc, monkeypatch)
    x, dhc, pure = G.dinputs(dc)[:3]
    bad = G.ref_fn(dc)(x, dhc, plant=(plant,))
    worst = {}
    for k in TC.hist_names(c) + TC.grad_names(c):
        (against, bmax, _), = refs["bounds"][k]
        assert against == "pure"
        worst[k] = TC._dist(TC._cut(c, k, bad[k]), TC._cut(c, k, pure[k]))[0] / bmax
    print("%s on %s: %s" % (plant, G.dcase_id(dc), {k: round(v, 1) for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:4]}))
    assert max(worst.values()) > 10, worst


def test_masks_matter_on_the_model_tests_inputs(monkeypatch):
    """The float64 oracle with and without the model test's masks, on its inputs: the decoder outputs differ by more
    than ten times the bound that test puts on them - the threshold its masks-matter check uses on the GPU."""
    from oracle import taco2_oracle as O
    case = GM.MATTER
    hp, params, stats, inputs, lengths, mel, lin = GM.matter_inputs()
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in params.items()}
    p.update({k: torch.tensor(v, dtype=torch.float64) for k, v in stats.items()})
    run = lambda: O.taco2_forward(p, hp.values(), torch.tensor(inputs), torch.tensor(lengths), torch.tensor(mel, dtype=torch.float64),
                                  torch.tensor(lin, dtype=torch.float64))["decoder_outputs"].numpy()
    with torch.no_grad():
        plain = run()
        masks = GM.oracle_masks(case["seed"], case["rate"], 0, case["shape"][0], case["shape"][2] // hp.outputs_per_step)
        monkeypatch.setattr(O, "prenet", PR.patched_prenet(O, masks, PR.scale_of(case["rate"])))
        masked = run()
    d = float(np.abs(masked - plain).max() / np.abs(plain).max())
    print("masked vs plain oracle decoder outputs: rel max %.3e, threshold %.1e" % (d, GM.MATTER_THRESHOLD))
    assert GM.MATTER_THRESHOLD == 10 * GM.SMALL_OUT_BOUND
    assert d > GM.MATTER_THRESHOLD, d
