"""Generation from a conditioned WaveNetModel: a local condition (one row per `hold` samples from position t0 on,
ns_wavenet_generate_params.cond_rows / cond_hold / cond_t0) on the per-layer kernel against a float64 sliding-window
generator on oracle/wavenet_oracle.py: network_full, and conditions / biases on the MFMA chain (engine 2) against the
per-layer kernel on the same bf16 weights.

Small configuration: Q = S = 64, R = Dc = 32 (the chain's widths), dilations 1 2 4 8 twice (L = 8); and dilations
1 2 4 once (L = 3): both generation kernels walk the layers two at a time and have a tail there."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"L8": dict(dilations_depth=2, dilations_length=4), "L3": dict(dilations_depth=1, dilations_length=3)}


def _hp(**over):
    from nspeech_amd import hparams as hparams_mod
    hp = hparams_mod.load("wavenet")
    small = dict(quantization_channels=64, skip_channels=64, residual_channels=32, dilation_channels=32)
    small.update(over)
    for k, v in small.items():
        setattr(hp, k, v)
    return hp


def _randomise(m, seed, scale=0.3):
    """Biases start at zero and a square embedding as the identity (wavenet.py:20-33): give them values, so that a bias
    added to the wrong tensor or a swapped filter / gate half shows."""
    rng = np.random.RandomState(seed)
    p = m.numpy_params()
    for k in p:
        if k.endswith("_bias") or k.endswith("gc_embedding"):
            p[k] = (rng.randn(*p[k].shape) * scale).astype(np.float32)
    m.load_numpy_params(p)
    return p


def _rows_needed(total, hold, t0):
    return max(0, total - 1 + t0) // hold + 1


# ------------------------------------------------------------------ 1. fp32, per-layer kernel, against float64
def _oracle_generate(p, hpv, seed_ids, uniforms, gc, lc, hold, t0):
    """Sliding-window generation of ONE waveform with the full network in float64: for the draw of sample t + 1 the
    last rf positions t - rf + 1 .. t go through network_full, position m with the condition row max(0, m + t0) // hold;
    float64 softmax of the last logits and an inverse-CDF draw exactly as oracle generate_full.  Returns the waveform,
    the smallest distance of any u * cdf[-1] to a CDF edge, and the last distribution."""
    from oracle import wavenet_oracle as O
    rf = O.receptive_field_full(hpv)
    Q = hpv["quantization_channels"]
    wave_ = [int(v) for v in seed_ids]
    g = None if gc is None else O.embed_gc(p, hpv, np.asarray(gc)[None])
    margin, pr = np.inf, None
    for u in uniforms:
        t = len(wave_) - 1
        pos = np.arange(t - rf + 1, t + 1)
        x = torch.nn.functional.one_hot(torch.tensor(wave_[-rf:]), Q).double()[None]
        c = torch.tensor(lc[np.maximum(0, pos + t0) // hold], dtype=torch.float64)[None]
        pr = torch.softmax(O.network_full(p, hpv, x, g, c)[0, -1].double(), dim=0).numpy()
        cdf = np.cumsum(pr)
        margin = min(margin, np.abs(cdf - u * cdf[-1]).min())
        wave_.append(int(min(np.searchsorted(cdf, u * cdf[-1], side="right"), len(pr) - 1)))
    return np.asarray(wave_, np.int32), margin, pr


FP32_CASES = {
    "lc": (dict(lc_channels=3), False),
    "lc, biases, gc category": (dict(lc_channels=2, use_biases=True, gc_channels=4, gc_category_cardinality=3), True),
}
DATA_SEED = 9           # with it no draw of any case below comes within 1e-4 of a CDF edge (asserted on the oracle's values)


def _fp32_data(rf, Q, lcc, hold, t0, with_gc):
    rng = np.random.RandomState(DATA_SEED)
    B, n_new = 2, 8
    seeds = rng.randint(0, Q, size=(B, rf + 3))
    un = rng.rand(B, n_new)
    lc = rng.randn(B, _rows_needed(rf + 3 + n_new, hold, t0), lcc).astype(np.float32)
    gc = rng.randint(0, 3, size=B) if with_gc else None
    return seeds, un, lc, gc


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
@pytest.mark.parametrize("hold,t0", [(1, 0), (3, 0), (3, "clamp")])
@pytest.mark.parametrize("case", sorted(FP32_CASES))
def test_local_condition_fp32_draws_what_the_oracle_draws(dev, case, hold, t0, cfg):
    """(hold, t0) = (3, 0): a row boundary inside the seed and inside the drawn samples; (3, -(rf + 1)): the seed's first
    rf + 1 positions stand in front of row 0 and take it."""
    from nspeech_amd.models import create_model
    over, with_gc = FP32_CASES[case]
    hp = _hp(**dict(CONFIGS[cfg], **over))
    m = create_model("wavenet", hp, device="cuda:0", dtype="fp32", seed=9)
    params = _randomise(m, 11)
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in params.items()}
    if t0 == "clamp":
        t0 = -(m.rf + 1)
    seeds, un, lc, gc = _fp32_data(m.rf, hp.quantization_channels, hp.lc_channels, hold, t0, with_gc)
    B = seeds.shape[0]
    want = [_oracle_generate(p, hp.values(), seeds[b], un[b], None if gc is None else gc[b], lc[b], hold, t0) for b in range(B)]
    margins = [w[1] for w in want]
    print("smallest distance of a draw to a CDF edge: %.3e" % min(margins))
    assert min(margins) >= 1e-4, margins        # a condition on the inputs: the comparison below has no case left out
    got = m.generate(seeds, un.shape[1], uniforms=un, global_conditions=gc, local_conditions=lc, hold=hold, t0=t0).cpu().numpy()
    assert m.last_engine == 0
    for b in range(B):
        assert np.array_equal(got[b], want[b][0]), (b, got[b][-un.shape[1]:], want[b][0][-un.shape[1]:])
    err = np.abs(m.last_probs.cpu().numpy().reshape(B, -1)[B - 1] - want[B - 1][2]).max()
    print("last_probs against the oracle: %.3e" % err)
    assert err < 1e-5


# ------------------------------------------------------------------ 2. bf16, MFMA chain against the per-layer kernel
COND_SCALE = 1.0        # of the local condition's rows and the speaker embedding
BIAS_SEED = 21
BF16_CASES = {
    "a: biases + gc category": dict(use_biases=True, gc_channels=4, gc_category_cardinality=3),
    "b: lc": dict(lc_channels=5),
    "c: biases + gc category + lc": dict(use_biases=True, gc_channels=4, gc_category_cardinality=3, lc_channels=5),
}
HOLD = 3
BOUND = 3e-2            # engine 2 against a chain with fp32 layer inputs at these widths (test_wavenet_mfma_chain_close_to_valu_chain)


def _bf16_model(over, cfg):
    from nspeech_amd.models import create_model
    hp = _hp(**dict(CONFIGS[cfg], **over))
    m = create_model("wavenet", hp, device="cuda:0", dtype="bf16", seed=8)
    p = m.numpy_params()
    rng = np.random.RandomState(BIAS_SEED)
    for k in p:                               # biases randn * 0.3; the conditions - here the speaker's embedding - randn * COND_SCALE
        if k.endswith("_bias") or k.endswith("gc_embedding"):
            p[k] = (rng.randn(*p[k].shape) * (0.3 if k.endswith("_bias") else COND_SCALE)).astype(np.float32)
    p["wavenet/postprocessing/postprocess2"] = p["wavenet/postprocessing/postprocess2"] * 10.0
    m.load_numpy_params(p)
    return hp, m, p


def _swapped(p, hp):
    """every layer's lc_filter <-> lc_gate (a model with a local condition), else filter_bias <-> gate_bias"""
    q = dict(p)
    a, b = ("lc_filter", "lc_gate") if hp.lc_channels else ("filter_bias", "gate_bias")
    for k in p:
        if k.endswith("/" + a):
            q[k], q[k[:-len(a)] + b] = p[k[:-len(a)] + b], p[k]
    return q


def _layers_rolled(p, hp):
    """layer l conditions with layer l + 1's terms: the lc kernels of a model with a local condition, else the gc kernels
    and the filter / gate biases"""
    q = dict(p)
    names = ("lc_filter", "lc_gate") if hp.lc_channels else ("gc_filter", "gc_gate", "filter_bias", "gate_bias")
    L = hp.dilations_depth * hp.dilations_length
    for n in names:
        for l in range(L):
            q["wavenet/dilated_stack/layer%d/%s" % (l, n)] = p["wavenet/dilated_stack/layer%d/%s" % ((l + 1) % L, n)]
    return q


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
@pytest.mark.parametrize("case", sorted(BF16_CASES))
def test_conditioned_mfma_chain_close_to_per_layer_kernel(dev, case, cfg):
    """Same history -> the next sample's distribution within BOUND on both engines, at a draw that sits on a later
    condition row than the first; before that, the per-layer kernel alone shows that the bound sees a condition on the
    wrong row, on the wrong layer, or on the wrong half of the gated unit (each moves the distribution by more than
    4 * BOUND).  Case a has one fixed row: there is no time axis to roll.  Then a run of 48 draws."""
    hp, m, p = _bf16_model(BF16_CASES[case], cfg)
    Q, rf = hp.quantization_channels, m.rf
    rng = np.random.RandomState(5)
    B, n = 3, 7
    n_seed = rf + 2
    t0 = -(rf - 1)                            # the seed's first rf - 1 positions stand in front of row 0
    seeds = rng.randint(0, Q, size=(B, n_seed))
    un = rng.rand(B, 48)
    gc = rng.randint(0, 3, size=B) if hp.gc_channels else None
    kw = dict(global_conditions=gc) if gc is not None else {}
    lc = None
    if hp.lc_channels:
        lc = (rng.randn(B, _rows_needed(n_seed + 48, HOLD, t0), hp.lc_channels) * COND_SCALE).astype(np.float32)
        kw.update(local_conditions=lc, hold=HOLD, t0=t0)
        row = lambda t: max(0, t + t0) // HOLD          # noqa: E731  the row of the step that draws sample t + 1
        assert row(n_seed + n - 2) > row(n_seed - 1)
    a = m.generate(seeds, n, uniforms=un[:, :n], engine=2, **kw).cpu().numpy()
    assert m.last_engine == 2
    pa = m.last_probs.clone().view(B, Q)
    hist = a[:, :-1]

    def per_layer(**over):
        m.generate(hist, 1, uniforms=un[:, n - 1:n], fast=False, **dict(kw, **over))
        assert m.last_engine == 0
        return m.last_probs.clone().view(B, Q)
    pb = per_layer()
    # the bound can see a mistake
    moved = {}
    if lc is not None:
        moved["rows rolled along time"] = (per_layer(local_conditions=np.roll(lc, 1, axis=1)) - pb).abs().max().item()
    for name, q in (("terms rolled along the layers", _layers_rolled(p, hp)), ("filter and gate halves exchanged", _swapped(p, hp))):
        m.load_numpy_params(q)
        moved[name] = (per_layer() - pb).abs().max().item()
    # and a bias that the chain left out: without it the two engines would differ by what its absence moves here, so
    # each must move the distribution by more than BOUND itself
    gone = {}
    if hp.use_biases:
        for name, ends in (("no dense biases", ("/dense_bias",)), ("no skip biases", ("/slip_bias",)),
                           ("no post-processing biases", ("postprocess1_bias", "postprocess2_bias"))):
            m.load_numpy_params({k: np.zeros_like(v) if k.endswith(ends) else v for k, v in p.items()})
            gone[name] = (per_layer() - pb).abs().max().item()
    m.load_numpy_params(p)
    print("moves of last_probs on the per-layer kernel:", {k: "%.3f" % v for k, v in dict(moved, **gone).items()})
    assert all(v > 4 * BOUND for v in moved.values()), moved
    assert all(v > BOUND for v in gone.values()), gone
    # one draw from the same history
    err = (pa - pb).abs().max().item()
    print("engine 2 against the per-layer kernel, same history: max |dp| = %.3e" % err)
    assert err < BOUND
    assert (pa.sum(1) - 1).abs().max().item() < 1e-4 and (pb.sum(1) - 1).abs().max().item() < 1e-4
    assert np.array_equal(a[:, :n_seed], seeds)
    # a run
    a = m.generate(seeds, 48, uniforms=un, engine=2, **kw).cpu().numpy()
    b = m.generate(seeds, 48, uniforms=un, fast=False, **kw).cpu().numpy()
    assert a.min() >= 0 and a.max() < Q and np.array_equal(a[:, :n_seed], seeds)
    print("equal entries over the run: %.3f" % (a == b).mean())
    assert (a == b).mean() > 0.5              # histories part ways at the first differing draw


# ------------------------------------------------------------------ 3. zero terms change nothing
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_zero_biases_on_the_chain_change_nothing(dev, cfg):
    from nspeech_amd.models import create_model
    hp = _hp(**CONFIGS[cfg])
    s = create_model("simple_wavenet", hp, device="cuda:0", dtype="bf16", seed=8)
    ps = s.numpy_params()
    ps["wavenet/postprocessing/postprocess2"] = ps["wavenet/postprocessing/postprocess2"] * 10.0
    s.load_numpy_params(ps)
    f = create_model("wavenet", _hp(use_biases=True, **CONFIGS[cfg]), device="cuda:0", dtype="bf16", seed=8)
    pf = f.numpy_params()
    assert all(not pf[k].any() for k in pf if k.endswith("_bias")) and set(ps) < set(pf)
    pf.update(ps)
    f.load_numpy_params(pf)
    rng = np.random.RandomState(6)
    seeds = rng.randint(0, hp.quantization_channels, size=(2, s.rf + 1))
    un = rng.rand(2, 12)
    a = s.generate(seeds, 12, uniforms=un, engine=2)
    pa = s.last_probs.clone()
    b = f.generate(seeds, 12, uniforms=un, engine=2)
    assert s.last_engine == 2 and f.last_engine == 2 and "cond" in f._gen_keep[-1] and "cond" not in s._gen_keep[-1]
    assert torch.equal(a, b)
    assert torch.equal(pa, f.last_probs)


# ------------------------------------------------------------------ 4. defaults and refusals
def test_engine_defaults_and_refusals(dev):
    from nspeech_amd.models import create_model
    full = dict(use_biases=True, gc_channels=4, gc_category_cardinality=3, lc_channels=2)
    hp = _hp(**dict(CONFIGS["L8"], **full))
    Q = hp.quantization_channels
    m = create_model("wavenet", hp, device="cuda:0", dtype="bf16", seed=3)
    rng = np.random.RandomState(2)
    seeds = rng.randint(0, Q, size=(2, m.rf))
    lc = rng.randn(2, m.rf + 6, 2).astype(np.float32)
    kw = dict(global_conditions=np.array([0, 2]), local_conditions=lc)
    ids = m.generate(seeds, 6, **kw).cpu().numpy()
    assert m.last_engine == 2
    assert ids.min() >= 0 and ids.max() < Q and np.array_equal(ids[:, :m.rf], seeds)
    ids = m.generate(seeds, 6, exact=True, **kw).cpu().numpy()
    assert m.last_engine == 0
    assert ids.min() >= 0 and ids.max() < Q and np.array_equal(ids[:, :m.rf], seeds)
    with pytest.raises(ValueError):             # rows are never repeated past the end
        m.generate(seeds, 7, **kw)
    with pytest.raises(ValueError):
        m.generate(seeds, 6, hold=0, **kw)
    for engine in (1, 3):
        with pytest.raises(ValueError):
            m.generate(seeds, 6, engine=engine, **kw)
    with pytest.raises(NotImplementedError):    # a locally conditioned model without its condition
        m.generate(seeds, 6, global_conditions=np.array([0, 2]))
    g = create_model("wavenet", _hp(use_biases=True, **CONFIGS["L8"]), device="cuda:0", dtype="bf16", seed=3)
    g.generate(seeds, 2)
    assert g.last_engine == 2
    with pytest.raises(ValueError):
        g.generate(seeds, 2, engine=1)
    # off the chain's widths: the per-layer kernel
    hp16 = _hp(**dict(CONFIGS["L8"], residual_channels=16, dilation_channels=16, **full))
    n = create_model("wavenet", hp16, device="cuda:0", dtype="bf16", seed=3)
    ids = n.generate(seeds, 6, **kw).cpu().numpy()
    assert n.last_engine == 0
    assert ids.min() >= 0 and ids.max() < Q and np.array_equal(ids[:, :n.rf], seeds)


def test_more_layers_than_the_chain_holds_a_condition_for(dev):
    """At S = 512, Q = 256 the conditioned chain's LDS state passes the launcher's limit up to 73 layers; the unconditioned
    one up to the 128 the generator takes.  A conditioned model with 80 layers runs on the per-layer kernel by default, as
    it did before the chain took conditions; without its biases the same network still runs on the chain."""
    from nspeech_amd import ops
    from nspeech_amd.models import create_model
    wide = dict(dilations_depth=80, dilations_length=1, skip_channels=512, quantization_channels=256)
    assert ops.wavenet_chain_fits(73, 32, 512, 256, True) and not ops.wavenet_chain_fits(74, 32, 512, 256, True)
    assert ops.wavenet_chain_fits(128, 32, 512, 256, False)
    m = create_model("wavenet", _hp(use_biases=True, gc_channels=4, gc_category_cardinality=3, **wide), device="cuda:0",
                     dtype="bf16", seed=3)
    assert m.L == 80
    seeds = np.random.RandomState(2).randint(0, 256, size=(1, m.rf))
    ids = m.generate(seeds, 4, global_conditions=np.array([1])).cpu().numpy()
    assert m.last_engine == 0
    assert ids.min() >= 0 and ids.max() < 256 and np.array_equal(ids[:, :m.rf], seeds)
    s = create_model("simple_wavenet", _hp(**wide), device="cuda:0", dtype="bf16", seed=3)
    ids = s.generate(seeds, 4, engine=2).cpu().numpy()
    assert s.last_engine == 2
    assert ids.min() >= 0 and ids.max() < 256 and np.array_equal(ids[:, :s.rf], seeds)


# ------------------------------------------------------------------ 5. generate_wavenet.py
def test_cli_chunks_land_on_the_right_rows(dev, tmp_path):
    """--save_every 5 draws 12 samples in chunks of 5, 5 and 2 against 3 rows of 5 samples: the waveform written equals
    ONE generate() call with row 0 at the first generated sample."""
    from nspeech_amd.models import create_model
    from nspeech_amd.models.wavenet import mu_law_encode
    over = dict(CONFIGS["L8"], lc_channels=4)
    hp = _hp(**over)
    Q = hp.quantization_channels
    m = create_model("wavenet", hp, device="cuda:0", dtype="bf16", seed=5)
    p = m.numpy_params()
    p["wavenet/postprocessing/postprocess2"] = p["wavenet/postprocessing/postprocess2"] * 10.0
    m.load_numpy_params(p)
    ckpt, cond, out = str(tmp_path / "model.ckpt-0"), str(tmp_path / "lc.npy"), str(tmp_path / "out.wav")
    torch.save(m.state_dict(), ckpt)
    lc = (np.random.RandomState(4).randn(3, 4) * 2).astype(np.float32)
    np.save(cond, lc)
    small = ",".join("%s=%d" % (k, getattr(hp, k)) for k in ("quantization_channels", "skip_channels", "residual_channels",
                                                            "dilation_channels", "dilations_depth", "dilations_length"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate_wavenet.py"), ckpt, "--samples", "12", "--save_every", "5",
                        "--lc_channels", "4", "--local_condition", cond, "--lc_hold", "5", "--hparams", small, "--seed", "7",
                        "--wav_out_path", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with wave.open(out, "rb") as f:
        pcm = np.frombuffer(f.readframes(f.getnframes()), "<i2").astype(np.float32) / 32767.0
    got = mu_law_encode(pcm[None], Q)[0]        # 16-bit samples are far finer than 64 mu-law steps
    # the script's own sequence of random numbers: the seed's last sample, then one block of uniforms per chunk
    rng = np.random.default_rng(7)
    seed = [Q // 2] * (m.rf - 1) + [int(rng.integers(Q))]
    un = np.concatenate([rng.random((1, k)) for k in (5, 5, 2)], axis=1)
    want = m.generate(np.asarray(seed, np.int32), 12, uniforms=un, local_conditions=lc[None], hold=5, t0=-m.rf).cpu().numpy()[0]
    assert got.shape == want.shape and np.array_equal(got, want), (got[-12:], want[-12:])
    assert len(set(want[-12:].tolist())) > 1
    # the script refuses what it cannot honour, before it builds a model
    import argparse
    import generate_wavenet
    args = dict(checkpoint=ckpt, hparams=small, gc_channels=None, lc_channels=4, local_condition=cond, lc_hold=5, samples=12,
                fast_generation=True, temperature=1.0)
    for over, text in ((dict(samples=16), "fewer than --samples"), (dict(fast_generation=False), "incremental generator only"),
                       (dict(temperature=0.9), "incremental generator only"), (dict(lc_hold=0), "--lc_hold must be at least 1"),
                       (dict(lc_channels=0), "--local_condition needs --lc_channels")):
        with pytest.raises(ValueError, match=text):
            generate_wavenet.main(argparse.Namespace(**dict(args, **over)))
