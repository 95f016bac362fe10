"""Sampling temperature and argmax in the WaveNet generator's draw (ns_wavenet_generate_params.temperature / argmax,
SimpleWaveNet.generate(temperature=)): the per-layer kernel draw for draw against a float64 sliding window with
generate_wavenet.py's scale_prediction, every engine against the definition applied to its own temperature-1
distribution, argmax, the serial draw branch of the MFMA kernel, the refusals, the Synthesizer and the script."""
import functools
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _hp(**over):
    from nspeech_amd import hparams as hparams_mod
    hp = hparams_mod.load("wavenet")
    small = dict(dilations_depth=2, dilations_length=3, residual_channels=16, dilation_channels=16, skip_channels=32,
                 quantization_channels=64)
    small.update(over)
    for k, v in small.items():
        setattr(hp, k, v)
    return hp


def _audio(N, T, seed):
    rng = np.random.RandomState(seed)
    t = np.arange(T) / 16000.0
    return np.stack([0.6 * np.sin(2 * np.pi * rng.uniform(100, 900) * t + rng.uniform(0, 6)) + 0.05 * rng.randn(T)
                     for _ in range(N)]).astype(np.float32)


def _sharpen(m, by):
    """Scale the last layer so that the distributions have structure (test_wavenet_gpu.py does the same)."""
    p = m.numpy_params()
    p["wavenet/postprocessing/postprocess2"] = p["wavenet/postprocessing/postprocess2"] * by
    m.load_numpy_params(p)
    return p


def _scale(p, T):
    """generate_wavenet.py's scale_prediction on every row of float64 p [B, Q]."""
    from generate_wavenet import scale_prediction
    return np.stack([scale_prediction(row, T) for row in np.asarray(p, np.float64)])


def _inv_cdf(p, u):
    """The draw of oracle.wavenet_oracle.generate: the first j with u * c[-1] < c[j]."""
    c = np.cumsum(p)
    return int(min(np.searchsorted(c, u * c[-1], side="right"), len(p) - 1))


# ------------------------------------------------------------------ 1. fp32, per-layer kernel, against float64
N_DRAW, N_ARGMAX = 12, 8
UN_SEED = 7             # with it every u * c[-1] below lies at least 4e-4 from a CDF step at T = 0.5, 1 and 1.5 (the tests assert
                        # 1e-4 on the reference's values; seeds 1 to 6 came within 1.5e-4 to 4e-5 or met a step's distribution
                        # that peaks below 4 / Q, and were passed over)
CHAIN = dict(residual_channels=32, dilation_channels=32, skip_channels=64, dilations_length=4)
MARGIN, GAP = 1e-4, 1e-3


def _fp32_inputs(rf, Q):
    from nspeech_amd.models.wavenet import mu_law_encode
    seeds = mu_law_encode(_audio(2, rf + 7, seed=5), Q)
    un = np.random.default_rng(UN_SEED).random((2, N_DRAW)).astype(np.float32)      # the kernel reads float32 uniforms
    return seeds, un


def _window_draws(pt, hpv, seed_ids, uniforms, T):
    """Sliding-window generation of one waveform in float64: predict_proba on the last rf samples, scale_prediction at
    T, the inverse CDF at the given uniform.  Returns the waveform, the least distance of a u * c[-1] to a CDF step and
    the least peak probability of a step's temperature-1 distribution."""
    from generate_wavenet import scale_prediction
    from oracle import wavenet_oracle as O
    rf = O.receptive_field(hpv)
    wave_, margin, peak = [int(v) for v in seed_ids], np.inf, np.inf
    for u in uniforms:
        pr = O.predict_proba(pt, hpv, torch.tensor(wave_[-rf:])).numpy()
        peak = min(peak, pr.max())
        w = scale_prediction(pr, T)
        c = np.cumsum(w)
        margin = min(margin, np.abs(c - float(u) * c[-1]).min())
        wave_.append(_inv_cdf(w, float(u)))
    return np.asarray(wave_, np.int32), margin, peak


def _window_argmax(pt, hpv, seed_ids, n):
    """The same window with the largest float64 logit taken; also the least gap between the top two logits."""
    from oracle import wavenet_oracle as O
    rf = O.receptive_field(hpv)
    wave_, gap = [int(v) for v in seed_ids], np.inf
    for _ in range(n):
        lg = O.network(pt, hpv, torch.tensor(wave_[-rf:])[None])[0, -1].double().numpy()
        top = np.sort(lg)[-2:]
        gap = min(gap, top[1] - top[0])
        wave_.append(int(np.argmax(lg)))
    return np.asarray(wave_, np.int32), gap


@functools.lru_cache(maxsize=None)
def _fp32_model():
    from nspeech_amd.models import create_model
    hp = _hp(**CHAIN)
    m = create_model("simple_wavenet", hp, device="cuda:0", dtype="fp32", seed=8)
    p = _sharpen(m, 12.0)
    pt = {k: torch.tensor(v, dtype=torch.float64) for k, v in p.items()}
    return hp, m, pt


@functools.lru_cache(maxsize=None)
def _fp32_reference(T):
    hp, m, pt = _fp32_model()
    seeds, un = _fp32_inputs(m.rf, hp.quantization_channels)
    out = [_window_draws(pt, hp.values(), seeds[b], un[b], T) for b in range(2)]
    return np.stack([o[0] for o in out]), min(o[1] for o in out), min(o[2] for o in out)


@pytest.mark.parametrize("T", [0.5, 1.5])
def test_per_layer_kernel_draws_what_the_tempered_oracle_draws(dev, T):
    """The eight-layer network of the engine tests below in fp32, its last layer scaled by 12: every step's float64
    distribution peaks above 4 / Q (4.2 / Q the least), and the temperature decides 19 of the 24 draws at either T."""
    hp, m, pt = _fp32_model()
    seeds, un = _fp32_inputs(m.rf, hp.quantization_channels)
    ref, margin, peak = _fp32_reference(T)
    plain, margin1, _ = _fp32_reference(1.0)
    print("T = %g: least distance of a draw to a CDF step %.3e (T = 1: %.3e), least peak %.2f / Q"
          % (T, margin, margin1, peak * hp.quantization_channels))
    assert margin >= MARGIN and margin1 >= MARGIN, (margin, margin1)     # fp32 logits differ from float64 ones by ~1e-6: a closer u could flip
    assert peak > 4.0 / hp.quantization_channels, peak
    assert (ref != plain).any()              # the temperature decides at least one draw
    got = m.generate(seeds, N_DRAW, uniforms=un, temperature=T).cpu().numpy()
    assert m.last_engine == 0
    assert np.array_equal(got, ref), (got[:, -N_DRAW:], ref[:, -N_DRAW:])
    one = m.generate(seeds, N_DRAW, uniforms=un).cpu().numpy()
    assert np.array_equal(one, plain) and not np.array_equal(one, got)


def test_per_layer_kernel_argmax_is_the_oracles(dev):
    hp, m, pt = _fp32_model()
    seeds, un = _fp32_inputs(m.rf, hp.quantization_channels)
    out = [_window_argmax(pt, hp.values(), seeds[b], N_ARGMAX) for b in range(2)]
    gap = min(o[1] for o in out)
    print("least gap between the top two logits %.3e" % gap)
    assert gap > GAP, gap
    got = m.generate(seeds, N_ARGMAX, uniforms=un[:, :N_ARGMAX], temperature=0).cpu().numpy()
    assert np.array_equal(got, np.stack([o[0] for o in out]))


# ------------------------------------------------------------------ 2. every engine
ENGINES = ["engine 1", "engine 2", "engine 2 with conditions", "engine 3", "per-layer kernel, bf16"]


@functools.lru_cache(maxsize=None)
def _bf16_model(kind):
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.models import create_model
    if kind == "small":
        hp = _hp(**CHAIN)
        m = create_model("simple_wavenet", hp, device="cuda:0", dtype="bf16", seed=8)
    elif kind == "conditioned":      # use_biases and a small local condition at the chain's widths, eight layers
        hp = _hp(quantization_channels=64, skip_channels=64, residual_channels=32, dilation_channels=32, dilations_depth=2,
                 dilations_length=4, use_biases=True, lc_channels=3)
        m = create_model("wavenet", hp, device="cuda:0", dtype="bf16", seed=8)
        rng = np.random.RandomState(11)
        p = m.numpy_params()
        for k in p:
            if k.endswith("_bias"):
                p[k] = (rng.randn(*p[k].shape) * 0.3).astype(np.float32)
        m.load_numpy_params(p)
    else:                            # wavenet.yaml as shipped: 50 layers, R = Dc = 32, S = 512, Q = 256
        hp = hparams_mod.load("wavenet")
        m = create_model("simple_wavenet", hp, device="cuda:0", dtype="bf16", seed=8)
        assert m.rf == 5117
    _sharpen(m, 10.0)
    return hp, m


def _engine_case(name):
    """-> (model, seeds [B, n_seed], generate's keywords, the engine generate must report)."""
    rng = np.random.RandomState(4)
    if name == "engine 3":
        hp, m = _bf16_model("shipped")
        return m, rng.randint(0, m.Q, size=(1, m.rf + 5)), {}, 3
    if name == "engine 2 with conditions":
        hp, m = _bf16_model("conditioned")
        B, n_seed, hold = 3, m.rf + 4, 3
        lc = rng.randn(B, (n_seed + 24) // hold + 1, 3).astype(np.float32)
        return m, rng.randint(0, m.Q, size=(B, n_seed)), dict(engine=2, local_conditions=lc, hold=hold), 2
    hp, m = _bf16_model("small")
    seeds = rng.randint(0, m.Q, size=(3, m.rf + 5))
    kw, eng = {"engine 1": (dict(engine=1), 1), "engine 2": (dict(engine=2), 2), "per-layer kernel, bf16": (dict(fast=False), 0)}[name]
    return m, seeds, kw, eng


def _one(m, seeds, un, kw, eng, **more):
    ids = m.generate(seeds, 1, uniforms=un, **dict(kw, **more)).cpu().numpy()
    assert m.last_engine == eng, (m.last_engine, eng)
    assert np.array_equal(ids[:, :-1], seeds)
    return ids[:, -1], m.last_probs.clone().view(len(seeds), -1)


def _check_tempered(m, seeds, kw, eng, temps=(0.7, 1.5)):
    B, Q = len(seeds), m.Q
    un = np.random.default_rng(2).random((B, 1)).astype(np.float32)
    _, p1 = _one(m, seeds, un, kw, eng)
    p1 = p1.cpu().numpy().astype(np.float64)
    assert (p1.max(1) > 4.0 / Q).all(), p1.max(1)            # distributions with structure, not the uniform one
    for T in temps:
        ids, pT = _one(m, seeds, un, kw, eng, temperature=T)
        pT = pT.cpu().numpy().astype(np.float64)
        err = np.abs(pT - _scale(p1, T)).max()
        tv = 0.5 * np.abs(pT - p1).sum(1)
        print("T = %g: max |p_T - scale(p_1, T)| = %.3e, total variation from p_1 %s" % (T, err, tv))
        assert err < 1e-5, (T, err)
        assert (tv > 1e-2).all(), (T, tv)
        for b in range(B):          # the draw is the inverse CDF of the kernel's own distribution at the given uniform
            assert abs(int(ids[b]) - _inv_cdf(pT[b], float(un[b, 0]))) <= 1, (T, b)


def _check_argmax(m, seeds, kw, eng):
    B = len(seeds)
    ua, ub = (np.random.default_rng(s).random((B, 1)).astype(np.float32) for s in (2, 9))
    assert not np.array_equal(ua, ub)
    _, p1 = _one(m, seeds, ua, kw, eng)
    ia, pa = _one(m, seeds, ua, kw, eng, temperature=0)
    ib, pb = _one(m, seeds, ub, kw, eng, temperature=0)
    assert np.array_equal(ia, pa.argmax(1).cpu().numpy()), (ia, pa.argmax(1))
    assert np.array_equal(ia, ib)                            # the uniforms play no part
    assert torch.equal(pa, p1) and torch.equal(pb, p1)       # last_probs: the temperature-1 distribution, bit for bit


@pytest.mark.parametrize("name", ENGINES)
def test_every_engine_applies_the_definition_to_its_own_logits(dev, name):
    _check_tempered(*_engine_case(name))


@pytest.mark.parametrize("name", ENGINES)
def test_every_engine_takes_the_argmax_at_temperature_zero(dev, name):
    _check_argmax(*_engine_case(name))


# ------------------------------------------------------------------ 3. a run of draws
def test_a_run_of_tempered_draws(dev):
    hp, m = _bf16_model("small")
    rng = np.random.RandomState(6)
    seeds = rng.randint(0, m.Q, size=(3, m.rf + 5))
    un = rng.rand(3, 24)
    runs = {}
    for name, kw in (("engine 1", dict(engine=1)), ("engine 2", dict(engine=2)), ("per-layer", dict(fast=False))):
        ids = m.generate(seeds, 24, uniforms=un, temperature=0.7, **kw).cpu().numpy()
        assert np.array_equal(ids[:, :m.rf + 5], seeds), name
        assert ids.min() >= 0 and ids.max() < m.Q, name
        runs[name] = ids[:, m.rf + 5:]
    plain = m.generate(seeds, 24, uniforms=un, engine=1).cpu().numpy()[:, m.rf + 5:]
    assert not np.array_equal(plain, runs["engine 1"])
    # identical operands, different summation order: a draw can only differ where u falls within ~1e-6 of a CDF step
    differ = (runs["engine 1"] != runs["per-layer"]).mean()
    assert differ < 0.02, differ


# ------------------------------------------------------------------ 5. the serial branch of the MFMA kernel
def test_serial_draw_branch_of_the_mfma_kernel(dev):
    """The MFMA kernel walks the CDF on one thread when Q > 512.  The launcher takes Q up to 1024 and the chain's
    post-processing products want Q / 8 to divide 512, so Q = 1024 is the one such size engine 2 accepts (engine 3 is
    Q = 256 only): one tempered sample and one argmax sample there, on a three-layer network.  Its last layer is scaled
    by 100: Glorot's bound for a [64, 1024] kernel is a third of the [64, 64] one's and three layers add up to less than
    eight, so that 10 leaves every distribution within 1.3 / Q of the uniform one."""
    from nspeech_amd.models import create_model
    hp = _hp(quantization_channels=1024, skip_channels=64, residual_channels=32, dilation_channels=32, dilations_depth=1,
             dilations_length=3)
    m = create_model("simple_wavenet", hp, device="cuda:0", dtype="bf16", seed=8)
    _sharpen(m, 100.0)
    seeds = np.random.RandomState(4).randint(0, 1024, size=(2, m.rf + 3))
    _check_tempered(m, seeds, dict(engine=2), 2, temps=(0.7,))
    _check_argmax(m, seeds, dict(engine=2), 2)


# ------------------------------------------------------------------ 6. refusals
def test_refusals(dev, monkeypatch):
    from nspeech_amd import ops
    from nspeech_amd._lib import NSError
    hp, m = _bf16_model("small")
    seeds = np.zeros((1, m.rf), np.int32)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            m.generate(seeds, 2, temperature=bad)
    real = ops.wavenet_generate
    for bad in (-0.5, float("nan")):         # the C entry point itself: NS_ERR_BAD_ARG (-1) and a message
        monkeypatch.setattr(ops, "wavenet_generate", lambda *a, _bad=bad, **k: real(*a, **dict(k, temperature=_bad)))
        with pytest.raises(NSError, match=r"ns_wavenet_generate failed \(-1\): ns_wavenet_generate: temperature"):
            m.generate(seeds, 2)
    monkeypatch.setattr(ops, "wavenet_generate", real)
    assert m.generate(seeds, 2).shape == (1, m.rf + 2)


# ------------------------------------------------------------------ 7. the Synthesizer
TACO_SMALL = dict(embedding_dim=32, encoder_conv_channels=64, encoder_lstm_units=32, attention_dim=64, decoder_lstm_units=64,
                  postnet_conv_channels=64, expand_conv_channels=64, expand_lstm_units=32, batch_size=2, batch_group_size=2,
                  max_iters=3)


def test_synthesizer_hands_the_temperature_to_the_vocoder(dev):
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.models.wavenet import mu_law_decode, mu_law_encode
    from nspeech_amd.synthesizer import Synthesizer
    whp = _hp(lc_channels=80, use_biases=True, dilations_depth=1, dilations_length=4, residual_channels=32, dilation_channels=32,
              skip_channels=64)
    hp = hparams_mod.load("taco2")
    for k, v in TACO_SMALL.items():
        setattr(hp, k, v)
    hparams_mod.set_hparams(hp)
    synth = Synthesizer(hp, dtype="bf16").load(None, "taco2")
    synth.load_vocoder(None, whp)
    v = synth.vocoder
    _sharpen(v, 10.0)
    text = "Hello, World."
    T, hop = hp.max_iters * hp.outputs_per_step, 250
    assert T * hop < 5000
    wav, mel, _ = synth.synthesize(text, vocoder="wavenet", temperature=0.6, seed=3)
    silence = int(mu_law_encode(np.zeros(1, np.float32), v.Q)[0])
    ids = v.generate(np.full((1, v.rf), silence, np.int32), T * hop, seed=3, local_conditions=mel[None], hold=hop, t0=-v.rf,
                     temperature=0.6)
    want = mu_law_decode(ids[0, v.rf:].cpu().numpy(), v.Q)
    full = synth._wavenet_vocode(mel, seed=3, temperature=0.6)
    assert full.shape == (T * hop,) and np.array_equal(full, want)
    assert len(wav) > 0 and np.array_equal(wav, want[:len(wav)])
    assert not np.array_equal(full, synth._wavenet_vocode(mel, seed=3))             # the temperature-1 wave is another one
    plain = synth.synthesize(text, vocoder="wavenet", seed=3)[0]
    assert len(plain) != len(wav) or not np.array_equal(plain, wav)
    # argmax: the random stream plays no part
    texts = ["Hello, World.", "Yes."]
    a = synth.synthesize_batch(texts, vocoder="wavenet", temperature=0, seed=1)
    b = synth.synthesize_batch(texts, vocoder="wavenet", temperature=0, seed=8)
    assert len(a) == 2 and all(len(x[0]) > 0 and np.array_equal(x[0], y[0]) for x, y in zip(a, b))
    # Griffin-Lim takes and ignores it, as it does the seed
    g0, g1 = synth.synthesize(text), synth.synthesize(text, temperature=0.6)
    assert np.array_equal(g0[0], g1[0])


# ------------------------------------------------------------------ 8. generate_wavenet.py
def test_cli_keeps_the_incremental_generator_at_any_temperature(dev, tmp_path):
    from nspeech_amd.models import create_model
    from nspeech_amd.models.wavenet import mu_law_encode
    hp = _hp(quantization_channels=64, skip_channels=64, residual_channels=32, dilation_channels=32, dilations_depth=2,
             dilations_length=4, lc_channels=4)
    Q = hp.quantization_channels
    m = create_model("wavenet", hp, device="cuda:0", dtype="bf16", seed=5)
    _sharpen(m, 10.0)
    ckpt, cond, out = str(tmp_path / "model.ckpt-0"), str(tmp_path / "lc.npy"), str(tmp_path / "out.wav")
    torch.save(m.state_dict(), ckpt)
    lc = (np.random.RandomState(4).randn(3, 4) * 2).astype(np.float32)
    np.save(cond, lc)
    small = ",".join("%s=%d" % (k, getattr(hp, k)) for k in ("quantization_channels", "skip_channels", "residual_channels",
                                                            "dilation_channels", "dilations_depth", "dilations_length"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate_wavenet.py"), ckpt, "--samples", "12", "--lc_channels", "4",
                        "--local_condition", cond, "--lc_hold", "5", "--hparams", small, "--seed", "7", "--wav_out_path", out,
                        "--incremental_temperature", "true", "--temperature", "0.8"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with wave.open(out, "rb") as f:
        pcm = np.frombuffer(f.readframes(f.getnframes()), "<i2").astype(np.float32) / 32767.0
    got = mu_law_encode(pcm[None], Q)[0]            # 16-bit samples are far finer than 64 mu-law steps
    # the script's own sequence of random numbers: the seed's last sample, then the uniforms of its one chunk
    rng = np.random.default_rng(7)
    seed = [Q // 2] * (m.rf - 1) + [int(rng.integers(Q))]
    un = rng.random((1, 12))
    kw = dict(uniforms=un, local_conditions=lc[None], hold=5, t0=-m.rf)
    want = m.generate(np.asarray(seed, np.int32), 12, temperature=0.8, **kw).cpu().numpy()[0]
    assert got.shape == want.shape and np.array_equal(got, want), (got[-12:], want[-12:])
    assert len(set(want[-12:].tolist())) > 1
    assert not np.array_equal(want, m.generate(np.asarray(seed, np.int32), 12, **kw).cpu().numpy()[0])
