"""The resumable WaveNet generator (ns_wavenet_generate_span, ops.wavenet_generate(span=), generate_stream,
Synthesizer.synthesize_stream, generate_wavenet.py --stream_chunk): on every single-workgroup kernel a series of spans
leaves what the one call leaves, bit for bit - ids, queues, last_probs, last_ends and the unwritten tail behind a stop -
wherever the boundaries lie, and the layers above hand out exactly the one call's waveform.

The models are test_wavenet_endpoint_gpu.py's six cases restated at dilations 1 2 4 8 twice, so that the largest ring (8
rows) is longer than the small chunks and a span leaves every ring half-turned (dilations_depth = 2 blocks of
dilations_length = 4 layers: models.wavenet.dilations; the other way round the largest dilation would be 2).  Two sets
of weights: postprocess2 times 10 where the draws must depend on the state the spans hand over (a wrong ring row or
condition row then changes the codes; more than one distinct code is asserted), and the freshly initialised ones for
the scripted end-point rows, which need that file's near-uniform distributions (u = 0 draws code 0, u = 1 - 2^-24
draws code Q - 1; asserted)."""
import argparse
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
Q = 64
N = 60                                       # drawn samples of a scripted row
U_SILENT, U_LOUD = np.float32(0.0), np.float32(1) - np.float32(2.0 ** -24)
THRESHOLD = 10 ** -2.0                       # find_endpoint's -40 dB
ENGINES = ["per-layer fp32", "per-layer bf16", "engine 1, R = 16", "engine 1, R = 32", "engine 2", "engine 2 with conditions"]
CHAIN = dict(residual_channels=32, dilation_channels=32, skip_channels=64)
HOLD = 3


def _hp(**over):
    from nspeech_amd import hparams as hparams_mod
    hp = hparams_mod.load("wavenet")
    small = dict(dilations_depth=2, dilations_length=4, residual_channels=16, dilation_channels=16, skip_channels=32,
                 quantization_channels=Q)
    small.update(over)
    for k, v in small.items():
        setattr(hp, k, v)
    return hp


@functools.lru_cache(maxsize=None)
def _model(kind):
    """-> (model, its freshly initialised parameters, the same with postprocess2 times 10 and the biases given values)."""
    from nspeech_amd.models import create_model
    if kind == "fp32":
        m = create_model("simple_wavenet", _hp(), device="cuda:0", dtype="fp32", seed=8)
    elif kind == "r16":
        m = create_model("simple_wavenet", _hp(), device="cuda:0", dtype="bf16", seed=8)
    elif kind == "r32":
        m = create_model("simple_wavenet", _hp(**CHAIN), device="cuda:0", dtype="bf16", seed=8)
    else:
        assert kind == "conditioned"
        m = create_model("wavenet", _hp(use_biases=True, lc_channels=3, **CHAIN), device="cuda:0", dtype="bf16", seed=8)
    assert max(m.dil) == 8 and m.L == 8
    fresh = m.numpy_params()
    sharp = dict(fresh)
    rng = np.random.RandomState(6)
    for k in sharp:
        if k.endswith("_bias"):
            sharp[k] = (rng.randn(*sharp[k].shape) * 0.1).astype(np.float32)
    sharp["wavenet/postprocessing/postprocess2"] = sharp["wavenet/postprocessing/postprocess2"] * 10.0
    return m, fresh, sharp


def _case(name, B, n, sharp):
    """-> (model, seeds [B, rf + 3], generate's keywords, the engine generate must report)."""
    kind, kw, eng = {"per-layer fp32": ("fp32", {}, 0), "per-layer bf16": ("r16", dict(fast=False), 0),
                     "engine 1, R = 16": ("r16", dict(engine=1), 1), "engine 1, R = 32": ("r32", dict(engine=1), 1),
                     "engine 2": ("r32", dict(engine=2), 2), "engine 2 with conditions": ("conditioned", dict(engine=2), 2)}[name]
    m, fresh, sharpened = _model(kind)
    m.load_numpy_params(sharpened if sharp else fresh)
    rng = np.random.RandomState(4)
    seeds = rng.randint(0, Q, size=(B, m.rf + 3)).astype(np.int32)
    if kind == "conditioned":
        kw = dict(kw, local_conditions=(0.3 * rng.randn(B, (m.rf + 3 + n) // HOLD + 1, 3)).astype(np.float32), hold=HOLD)
    return m, seeds, kw, eng


def _one_call(m, seeds, n, **kw):
    """generate() and what it left: ids, the final queues, last_probs, last_ends - host copies."""
    from nspeech_amd import ops
    real, seen = ops.wavenet_generate, []

    def spy(*a, **k):
        seen.append(a[14])                   # queues
        return real(*a, **k)
    ops.wavenet_generate = spy
    try:
        ids = m.generate(seeds, n, **kw)
    finally:
        ops.wavenet_generate = real
    return (ids.cpu().numpy(), seen[0].cpu().numpy().copy(), m.last_probs.cpu().numpy().copy(), m.last_ends.cpu().numpy().copy())


# ------------------------------------------------------------------ 1. spans equal one call
@pytest.mark.parametrize("name", ENGINES)
def test_spans_equal_one_call(dev, name):
    from nspeech_amd import ops
    B, n = 3, 40
    m, seeds, kw, eng = _case(name, B, n, sharp=True)
    n_seed, total = seeds.shape[1], seeds.shape[1] + n
    un = np.random.RandomState(9).rand(B, n).astype(np.float32)
    ids, queues, probs, ends = _one_call(m, seeds, n, uniforms=un, **kw)
    assert m.last_engine == eng and ends.tolist() == [n] * B
    assert np.array_equal(ids[:, :n_seed], seeds) and probs.any() and queues.any()
    assert all(len(set(row[n_seed:].tolist())) > 1 for row in ids), ids[:, n_seed:]       # the draws depend on the state
    # generate_stream at every chunk size: 1, sizes that leave the rings of 8 half-turned, on and off multiples of hold = 3,
    # and the whole waveform as one span
    for chunk in (1, 3, 5, 7, 8, 16, 40):
        m.last_engine = None
        stream = m.generate_stream(seeds, n, chunk, uniforms=un, **kw)
        pieces = list(stream)
        assert [p.shape for p in pieces] == [(B, min(chunk, n - j)) for j in range(0, n, chunk)], chunk
        assert all(p.dtype == np.int32 for p in pieces)
        assert np.array_equal(np.concatenate(pieces, axis=1), ids[:, n_seed:]), (name, chunk)
        assert np.array_equal(stream.ids.cpu().numpy(), ids), (name, chunk)
        assert np.array_equal(stream.queues.cpu().numpy(), queues), (name, chunk)
        assert np.array_equal(m.last_probs.cpu().numpy(), probs), (name, chunk)
        assert m.last_engine == eng and stream.last_engine == eng and m.last_ends.cpu().tolist() == [n] * B
        assert stream.drawn == n and next(stream, None) is None
    # a hand-made series through ops.wavenet_generate(span=): [1, 5) draws nothing and ends inside the seed, then a
    # boundary in the middle of the draws, a span of one step, and the rest
    real, calls = ops.wavenet_generate, []

    def spy(*a, **k):
        calls.append((a, dict(k)))
        return real(*a, **k)
    ops.wavenet_generate = spy
    try:
        stream = m.generate_stream(seeds, n, n, uniforms=un, **kw)
    finally:
        ops.wavenet_generate = real
    list(stream)
    (a, k), = calls
    assert k["span"][:2] == (1, total) and k["span"][2] is None
    stream.ids[:, n_seed:] = 0
    stream.queues.zero_()
    m.last_probs.zero_()
    for t0, t1 in ((1, 5), (5, n_seed + 9), (n_seed + 9, n_seed + 10), (n_seed + 10, total)):
        real(*a, **dict(k, span=(t0, t1, None)))
        if t1 == 5:
            assert not stream.ids[:, n_seed:].any().item() and stream.queues.any().item()
    assert np.array_equal(stream.ids.cpu().numpy(), ids)
    assert np.array_equal(stream.queues.cpu().numpy(), queues)
    assert np.array_equal(m.last_probs.cpu().numpy(), probs)


# ------------------------------------------------------------------ 2. the end-point rule's pair is carried
def _script(window, hop, n=N):
    """silent [6, n] (True = a silent sample): test_wavenet_endpoint_gpu.py's rows (a) .. (f)."""
    s = np.zeros((6, n), bool)
    s[1, 11:] = True                                   # (b) silent from a j that is no multiple of hop
    assert 11 % hop
    s[2, :window - 1] = True                           # (c) window - 1 silent, one loud, silent to the end
    s[2, window:] = True
    s[3, :] = True                                     # (d) silent from j = 0: x = 0 is never tested, end = 2 hop
    s[4, n - window:] = True                           # (e) silent only from x = n - window on: the strict bound
    s[5, -(-(n - window - hop) // hop) * hop:] = True  # (f) from x = n - window - hop, taken up to a multiple of hop
    return s


def _find_endpoints(ids_full, n_seed, window, hop, monkeypatch):
    """audio.find_endpoint on the decoded samples of the unstopped run, row by row -> (ends, drawn, rule)."""
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.models.wavenet import mu_law_decode
    from nspeech_amd.utils import audio
    hparams_mod.load("taco2")
    with monkeypatch.context() as mp:
        mp.setattr(audio, "endpoint_rule", lambda *a, **k: (window, hop, np.power(10.0, -40 * 0.05)))
        rule = audio.endpoint_rule()
        ends = [audio.find_endpoint(mu_law_decode(row[n_seed:], Q)) for row in ids_full]
    n = ids_full.shape[1] - n_seed
    return np.asarray(ends), np.asarray([e - hop + window if e < n else n for e in ends]), rule


@pytest.mark.parametrize("window,hop", [(6, 2), (7, 2)])
@pytest.mark.parametrize("name", ENGINES)
def test_the_rule_is_carried_across_spans(dev, monkeypatch, name, window, hop):
    m, seeds, kw, eng = _case(name, 6, N, sharp=False)
    n_seed = seeds.shape[1]
    silent = _script(window, hop)
    un = np.where(silent, U_SILENT, U_LOUD).astype(np.float32)
    full = m.generate(seeds, N, uniforms=un, **kw).cpu().numpy()
    assert np.array_equal(full[:, n_seed:], np.where(silent, 0, Q - 1)), name       # the codes came out as scripted
    ends, drawn, rule = _find_endpoints(full, n_seed, window, hop, monkeypatch)
    x_f, x_c = -(-(N - window - hop) // hop) * hop, -(-window // hop) * hop
    assert ends.tolist() == [N, 12 + hop, x_c + hop, 2 * hop, N, x_f + hop], ends
    ids, queues, probs, ends_one = _one_call(m, seeds, N, uniforms=un, endpoint=rule, **kw)
    assert np.array_equal(ends_one, ends)
    for b in range(6):
        k = n_seed + int(drawn[b])
        assert np.array_equal(ids[b, :k], full[b, :k]) and not ids[b, k:].any(), b
    # chunks of 1, of 5, and one whose first span ends exactly on the sample that fires row (d): j = hop + window - 1
    for chunk in (1, 5, hop + window):
        stream = m.generate_stream(seeds, N, chunk, uniforms=un, endpoint=rule, **kw)
        was_fired = np.zeros(6, bool)
        pieces = []
        for piece in stream:
            pieces.append(piece)
            assert (stream.fired >= was_fired).all()                   # fired is never cleared
            # a row fires in the span that draws its last sample, and is seen then
            assert np.array_equal(stream.fired, (drawn < N) & (drawn <= stream.drawn)), (chunk, stream.drawn, stream.fired)
            assert np.array_equal(stream.ends, np.where(stream.fired, ends, N))
            was_fired = stream.fired.copy()
        assert stream.drawn == N                                      # rows (a) and (e) run to the end
        assert np.array_equal(np.concatenate(pieces, axis=1), ids[:, n_seed:]), (name, chunk)
        assert np.array_equal(stream.ids.cpu().numpy(), ids), (name, chunk)              # the zero tails included
        assert np.array_equal(stream.queues.cpu().numpy(), queues), (name, chunk)        # a stopped row's rings stay put
        assert np.array_equal(m.last_ends.cpu().numpy(), ends) and m.last_ends.dtype == torch.int64
        assert np.array_equal(m.last_probs.cpu().numpy(), probs) and m.last_engine == eng
        assert stream.carry.cpu().numpy()[:, 1].tolist() == (drawn < N).astype(int).tolist()


@pytest.mark.parametrize("name", ENGINES)
def test_the_stream_ends_when_every_row_has_fired(dev, name):
    from nspeech_amd import ops
    window, hop = 6, 2
    m, seeds, kw, eng = _case(name, 6, N, sharp=False)
    n_seed = seeds.shape[1]
    un = np.zeros((6, N), np.float32)                                  # every row silent: all fire at j = hop + window - 1
    ids, queues, probs, ends = _one_call(m, seeds, N, uniforms=un, endpoint=(window, hop, THRESHOLD), **kw)
    assert ends.tolist() == [2 * hop] * 6 and not ids[:, n_seed:].any() and not probs.any()
    real, spans = ops.wavenet_generate, []

    def spy(*a, **k):
        spans.append(k["span"][:2])
        return real(*a, **k)
    for chunk, yielded in ((1, 8), (5, 10), (8, 8), (9, 9)):
        del spans[:]
        ops.wavenet_generate = spy
        try:
            stream = m.generate_stream(seeds, N, chunk, uniforms=un, endpoint=(window, hop, THRESHOLD), **kw)
            pieces = list(stream)
        finally:
            ops.wavenet_generate = real
        assert sum(p.shape[1] for p in pieces) == yielded == stream.drawn and stream.fired.all()
        # one span was launched ahead of the chunk that showed the last stop, none behind it
        assert len(spans) == len(pieces) + 1 and spans[0][0] == 1 and spans[-1][1] == n_seed + yielded + chunk - 1
        assert np.array_equal(stream.ids.cpu().numpy(), ids) and np.array_equal(stream.queues.cpu().numpy(), queues)
        assert m.last_ends.cpu().tolist() == [2 * hop] * 6 and not m.last_probs.any().item()


# ------------------------------------------------------------------ 3. what a stream refuses
def test_engine_3_and_an_empty_chunk_are_refused(dev, monkeypatch):
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd import ops
    from nspeech_amd.models import create_model
    m, _, _ = _model("r32")
    seeds = np.zeros((1, m.rf), np.int32)

    def launched(*a, **k):
        raise AssertionError("a kernel was launched")
    with monkeypatch.context() as mp:
        mp.setattr(ops, "wavenet_generate", launched)
        with pytest.raises(ValueError, match="engine 3"):
            m.generate_stream(seeds, 4, 2, engine=3)
        for chunk in (0, -1):
            with pytest.raises(ValueError, match="chunk"):
                m.generate_stream(seeds, 4, chunk)
    # wavenet.yaml as shipped (S = 512, Q = 256, no conditions): where generate() may pick engine 3, a stream stays at 2
    big = create_model("simple_wavenet", hparams_mod.load("wavenet"), device="cuda:0", dtype="bf16", seed=8)
    assert big.S == 512 and big.Q == 256
    pieces = list(big.generate_stream(np.zeros((1, big.rf), np.int32), 4, 3))
    assert big.last_engine == 2 and [p.shape for p in pieces] == [(1, 3), (1, 1)]


# ------------------------------------------------------------------ 4. the Synthesizer
TACO_SMALL = dict(embedding_dim=32, encoder_conv_channels=64, encoder_lstm_units=32, attention_dim=64, decoder_lstm_units=64,
                  postnet_conv_channels=64, expand_conv_channels=64, expand_lstm_units=32, batch_size=2, batch_group_size=2,
                  max_iters=17)
T_SAMPLES = 17 * 5 * 250                     # 85 frames of 250 samples: more than window + hop = 20000


@functools.lru_cache(maxsize=None)
def _synth():
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.synthesizer import Synthesizer
    whp = _hp(lc_channels=80, use_biases=True, dilations_depth=1, dilations_length=4, **CHAIN)
    hp = hparams_mod.load("taco2")
    for k, v in TACO_SMALL.items():
        setattr(hp, k, v)
    hparams_mod.set_hparams(hp)
    synth = Synthesizer(hp, dtype="bf16").load(None, "taco2")
    synth.load_vocoder(None, whp)
    assert hp.max_iters * hp.outputs_per_step * synth._vocoder_hop == T_SAMPLES
    return synth, synth.vocoder.numpy_params()


def _silent_vocoder(synth, fresh):
    """postprocess2's bias raised at the code of zero amplitude: at temperature 0 every sample is that code."""
    from nspeech_amd.models.wavenet import mu_law_encode
    from nspeech_amd import hparams as hparams_mod
    hparams_mod.set_hparams(synth.hparams)
    silence = int(mu_law_encode(np.zeros(1, np.float32), Q)[0])
    p = dict(fresh)
    bias = p["wavenet/postprocessing/postprocess2_bias"].copy()
    bias[silence] = 30.0
    p["wavenet/postprocessing/postprocess2_bias"] = bias
    synth.vocoder.load_numpy_params(p)
    return silence


def test_synthesize_stream_of_a_silent_vocoder(dev):
    synth, fresh = _synth()
    silence = _silent_vocoder(synth, fresh)
    rf = synth.vocoder.rf
    one = synth.synthesize("Hello, World.", vocoder="wavenet", temperature=0)
    assert one[0].shape == (8000,) and synth.vocoder.last_ends.tolist() == [8000]
    stream = synth.synthesize_stream("Hello, World.", chunk_samples=2500, temperature=0)
    assert np.array_equal(stream.mel, one[1]) and np.array_equal(stream.lin, one[2])
    pieces = list(stream)
    # 12000 trailing silent samples are held back: the chunks that end at 12500, 15000 and 17500 hand out 500, 2500 and
    # 2500, the one in which the rule fires (20000 drawn) the rest up to the end point
    assert [len(p) for p in pieces] == [500, 2500, 2500, 2500] and all(p.dtype == np.float32 for p in pieces)
    assert np.array_equal(np.concatenate(pieces), one[0])
    # the generator drew what the one call draws - up to the end of the window that fired - not T * hop
    codes = stream.codes
    assert codes.drawn == 20000 and synth.vocoder.last_ends.tolist() == [8000] and synth.vocoder.last_engine == 2
    ids = codes.ids.cpu().numpy()[0]
    assert (ids[:rf + 20000] == silence).all() and not ids[rf + 20000:].any() and len(ids) == rf + T_SAMPLES
    # uncut on request: every sample, as drawn
    uncut = list(synth.synthesize_stream("Hello, World.", chunk_samples=2500, temperature=0, stop_at_endpoint=False))
    assert [len(p) for p in uncut] == [2500] * 8 + [1250]
    assert sum(len(p) for p in uncut) == T_SAMPLES and np.array_equal(np.concatenate(uncut)[:8000], one[0])
    # the default chunk is 20 hops
    assert len(next(iter(synth.synthesize_stream("Hello, World.", temperature=0, stop_at_endpoint=False)))) == 5000


def test_synthesize_stream_of_a_loud_vocoder(dev):
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.synthesizer import Synthesizer
    synth, fresh = _synth()
    hparams_mod.set_hparams(synth.hparams)
    synth.vocoder.load_numpy_params(fresh)
    one = synth.synthesize("Hello, World.", vocoder="wavenet", temperature=1, seed=3)
    assert one[0].shape == (T_SAMPLES,)
    stream = synth.synthesize_stream("Hello, World.", chunk_samples=2500, temperature=1, seed=3)
    pieces = list(stream)
    assert len(pieces) > 1 and np.array_equal(np.concatenate(pieces), one[0])
    assert np.array_equal(stream.mel, one[1]) and np.array_equal(stream.lin, one[2])
    assert len(set(np.concatenate(pieces).tolist())) > Q // 2
    # the refusal of synthesize(vocoder="wavenet")
    with pytest.raises(ValueError, match="load_vocoder"):
        Synthesizer(synth.hparams).synthesize_stream("Hello, World.")


# ------------------------------------------------------------------ 5. generate_wavenet.py --stream_chunk
def _read(path):
    with wave.open(path, "rb") as f:
        return np.frombuffer(f.readframes(f.getnframes()), "<i2").copy()


def _small(hp):
    return ",".join("%s=%d" % (k, getattr(hp, k)) for k in ("quantization_channels", "skip_channels", "residual_channels",
                                                            "dilation_channels", "dilations_depth", "dilations_length"))


def test_cli_stream_chunk_writes_the_file_of_the_plain_run(dev, tmp_path):
    from nspeech_amd.models import create_model
    from nspeech_amd.models.wavenet import mu_law_encode
    hp = _hp(lc_channels=4, dilations_depth=2, dilations_length=4, **CHAIN)
    m = create_model("wavenet", hp, device="cuda:0", dtype="bf16", seed=5)
    p = m.numpy_params()
    p["wavenet/postprocessing/postprocess2"] = p["wavenet/postprocessing/postprocess2"] * 10.0
    m.load_numpy_params(p)
    ckpt, cond = str(tmp_path / "model.ckpt-0"), str(tmp_path / "lc.npy")
    torch.save(m.state_dict(), ckpt)
    np.save(cond, (np.random.RandomState(4).randn(3, 4) * 2).astype(np.float32))
    files = []
    for more in ([], ["--stream_chunk", "5"]):
        out = str(tmp_path / ("out%d.wav" % len(more)))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "generate_wavenet.py"), ckpt, "--samples", "12", "--lc_channels", "4",
                            "--local_condition", cond, "--lc_hold", "5", "--hparams", _small(hp), "--seed", "7",
                            "--wav_out_path", out] + more, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        files.append(_read(out))
        # the file is rewritten behind the chunks of 5 and 5, and at the end
        assert r.stdout.count("Updated wav file") == (3 if more else 1), r.stdout
    assert len(files[0]) == m.rf + 12 and np.array_equal(files[0], files[1])
    assert len(set(mu_law_encode(files[1][None, -12:].astype(np.float32) / 32767.0, Q)[0].tolist())) > 1


def test_cli_stream_chunk_is_cut_at_the_end_point(dev, tmp_path, capsys):
    """A model whose logits are all zero draws code 0 at temperature 0 - silent - so the rule (16000, 4000) fires with
    sample 19999 and the end point is 8000: the stream of 5000-sample chunks ends with the fourth and the file is cut."""
    import generate_wavenet
    from nspeech_amd.models import create_model
    hp = _hp(dilations_depth=1, dilations_length=4, **CHAIN)
    m = create_model("simple_wavenet", hp, device="cuda:0", dtype="bf16", seed=5)
    p = m.numpy_params()
    p["wavenet/postprocessing/postprocess2"] = p["wavenet/postprocessing/postprocess2"] * 0.0
    m.load_numpy_params(p)
    ckpt, out = str(tmp_path / "model.ckpt-0"), str(tmp_path / "out.wav")
    torch.save(m.state_dict(), ckpt)
    args = argparse.Namespace(checkpoint=ckpt, hparams=_small(hp), gc_channels=None, lc_channels=None, local_condition=None, lc_hold=1,
                              samples=21000, fast_generation=True, temperature=0.0, incremental_temperature=True, precision="bf16",
                              seed=0, wav_seed=None, save_every=None, stop_at_endpoint=True, stream_chunk=5000, wav_out_path=out)
    waveform = generate_wavenet.main(args)
    assert len(waveform) == m.rf + 8000 and not any(waveform[m.rf:])
    text = capsys.readouterr().out
    assert "End point at sample 8000 of 21000" in text and text.count("Updated wav file") == 4       # 3 partial, 1 final
    pcm = _read(out)
    assert len(pcm) == m.rf + 8000 and (pcm[m.rf:] == -32767).all()
