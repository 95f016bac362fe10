"""The utterance front end on the device (csrc/frontend.hip): ns_resample against audio._resample_reference run on the
CPU - equal bits, no tolerance: the same IEEE operations in the same order -, ns_frame_power against direct float64
sums, the device trim bounds against trim_wav / trim_silence, and the device chain (load_wav_device ->
trim_bounds_device -> features; DataFeeder(device_cache=True)) against the host chain it replaces."""
import os
import sys
import wave

import numpy as np
import pytest
import torch

import flac_writer as FW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
GUARD_VALUE = -12345.0


def _hp():
    from nspeech_amd import hparams
    hp = hparams.load("taco2")
    assert hp.sample_rate == 20000
    return hp


def _speech(seed, seconds, sr):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench.synthetic_speech(np.random.default_rng(seed), seconds, sr)


def _abi_resample(xt, sr_in, sr_out, stream):
    """ns_resample through the C ABI on `stream`, the output followed by guard words; returns (y, guard) as NumPy."""
    from nspeech_amd import _lib as L, ops
    from nspeech_amd.utils import audio as A
    n_out = int(xt.numel() * (float(sr_out) / float(sr_in)))
    win, delta, num_table = A._get_resample_tables(sr_in, sr_out, xt.device)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        buf = torch.full((n_out + GUARD,), GUARD_VALUE, dtype=torch.float32, device=xt.device)
        p = L.struct("ns_resample_params")
        p.x, p.x_dtype, p.n_in = ops.ptr(xt), L.NS_F32 if xt.dtype == torch.float32 else L.NS_F64, xt.numel()
        p.y, p.n_out, p.sr_in, p.sr_out = ops.ptr(buf), n_out, sr_in, sr_out
        p.win, p.delta, p.nwin, p.num_table = ops.ptr(win), ops.ptr(delta), win.numel(), num_table
        L.call("ns_resample", p, stream.cuda_stream)
    stream.synchronize()
    out = buf.cpu().numpy()
    return out[:n_out], out[n_out:]


@pytest.mark.parametrize("sr_in,sr_out", [(8000, 20000), (16000, 20000), (22050, 20000), (44100, 20000), (48000, 20000),
                                          (20000, 22050)])
def test_resample_equals_the_reference_bit_for_bit(dev, sr_in, sr_out):
    """Every combination of {Gaussian noise, PCM16-quantised synthetic speech} x {1, 50, one second, ten seconds of
    samples} x {float32, float64 input}, through the C ABI on a non-default stream, guard words behind n_out intact;
    and the NumPy-in / NumPy-out `resample` on the one-second clips."""
    from nspeech_amd.utils import audio as A
    rng = np.random.default_rng(sr_in + sr_out)
    full = 10 * sr_in
    noise64 = 0.25 * rng.standard_normal(full)
    speech = np.round(_speech(sr_in % 97, 10, sr_in).astype(np.float64) * 32767.0).clip(-32768, 32767) / 32768.0
    assert np.array_equal(speech, speech.astype(np.float32).astype(np.float64))
    signals = {("noise", "float32"): noise64.astype(np.float32), ("noise", "float64"): noise64,
               ("speech", "float32"): speech.astype(np.float32), ("speech", "float64"): speech}
    stream = torch.cuda.Stream(device=dev)
    checked = 0
    for (kind, dtype), sig in signals.items():
        assert str(sig.dtype) == dtype
        for n in (1, 50, sr_in, full):
            x = np.ascontiguousarray(sig[:n])
            n_out = int(n * (float(sr_out) / float(sr_in)))
            # one sample at a rate above the target's gives no output at all; the reference cannot form the maximum of
            # its empty tap counts, and an empty result has only one value
            want = A._resample_reference(x, sr_in, sr_out, device="cpu") if n_out else np.zeros(0, np.float32)
            got, guard = _abi_resample(torch.from_numpy(x).to(dev), sr_in, sr_out, stream)
            assert got.shape == want.shape == (int(n * (float(sr_out) / float(sr_in))),), (kind, dtype, n)
            same = np.array_equal(got, want)
            print("%d -> %d %s %s n=%d: n_out %d, equal %s, differing samples %d" %
                  (sr_in, sr_out, kind, dtype, n, want.size, same, int((got != want).sum())))
            assert same, (kind, dtype, n)
            assert np.all(guard == np.float32(GUARD_VALUE)), (kind, dtype, n)
            if n == sr_in:
                assert np.array_equal(A.resample(x, sr_in, sr_out), want), (kind, dtype, n)
            checked += 1
    assert checked == 16


def test_resample_device_keeps_the_result_on_the_device(dev):
    from nspeech_amd.utils import audio as A
    x = (0.1 * np.random.default_rng(3).standard_normal(30000)).astype(np.float32)
    y = A.resample_device(torch.from_numpy(x).to(dev), 22050, 20000)
    assert y.is_cuda and y.dtype == torch.float32
    assert np.array_equal(y.cpu().numpy(), A._resample_reference(x, 22050, 20000, device="cpu"))
    assert A.resample_device(torch.zeros(0, device=dev), 22050, 20000).numel() == 0


def _direct_power(x, frame_length, hop):
    y = np.pad(np.asarray(x, np.float64), frame_length // 2, mode="reflect")
    return np.array([np.sum(y[f * hop:f * hop + frame_length] ** 2) / frame_length for f in range(1 + len(x) // hop)])


@pytest.mark.parametrize("frame_length,hop", [(1024, 512), (2048, 512)])
def test_frame_power_against_direct_float64_sums(dev, frame_length, hop):
    """Relative error <= 1e-12: all terms are non-negative, so a float64 sum of at most 2048 of them in any order is
    within 2048 x 2^-53 = 2.3e-13 of the exact one."""
    from nspeech_amd.datasets import process as P
    rng = np.random.default_rng(frame_length)
    for n in (frame_length // 2 + 1, frame_length, 5000, 5120, 76000, 200000):
        x = (0.3 * rng.standard_normal(n) * np.linspace(0.001, 1.0, n)).astype(np.float32)
        got = P.frame_power_device(torch.from_numpy(x).to(dev), frame_length, hop)
        want = _direct_power(x, frame_length, hop)
        assert got.shape == want.shape and got.dtype == np.float64
        rel = np.abs(got - want).max() / want.max()
        each = (np.abs(got - want) / want).max()
        print("frame_power %d / %d, n = %d: %d frames, max relative error %.3g (per frame %.3g)" % (frame_length, hop, n, want.size, rel, each))
        assert each <= 1e-12, (n, each)


def _padded_speech(seed):
    """Three seconds of synthetic speech between 9 000 and 7 000 samples of N(0, 0.002) noise, at 20 kHz."""
    rng = np.random.default_rng(seed)
    body = _speech(seed, 3, 20000)
    return np.concatenate([rng.normal(0, 0.002, 9000), body, rng.normal(0, 0.002, 7000)]).astype(np.float32)


def _host_power(wav, frame_length, hop):
    """The frame powers as the host code forms them (differences of one running sum)."""
    y = np.pad(np.asarray(wav, np.float64), frame_length // 2, mode="reflect")
    sq = np.concatenate([[0.0], np.cumsum(y * y)])
    starts = np.arange(1 + (len(y) - frame_length) // hop) * hop
    return np.maximum((sq[starts + frame_length] - sq[starts]) / frame_length, 0.0)


def _trim_wav_margin_db(wav, top_db=25):
    mse = _host_power(wav, 1024, 512)
    db = 10.0 * np.log10(np.maximum(1e-10, mse)) - 10.0 * np.log10(max(1e-10, float(mse.max())))
    return float(np.abs(db + top_db).min())


def _trim_silence_margin_db(wav, threshold):
    with np.errstate(divide="ignore"):
        return float(np.abs(20.0 * np.log10(np.sqrt(_host_power(wav, 2048, 512)) / threshold)).min())


def _trim_cases():
    cases = [("speech between noise, seed %d" % s, _padded_speech(s)) for s in range(4)]
    cases.append(("all silence", np.zeros(30000, np.float32)))
    cases.append(("no silence", _speech(9, 2, 20000)))
    return cases


def test_trim_bounds_device_takes_trim_wavs_slice(dev):
    """Condition on the inputs, asserted on the host values first: every frame is at least 1e-3 dB away from the
    threshold (the host forms frame sums as differences of a running sum, the kernel adds directly; the worst-case
    rounding of the former on a 10 s clip is about 1e-4 dB)."""
    from nspeech_amd.datasets import process as P
    for name, wav in _trim_cases():
        margin = _trim_wav_margin_db(wav)
        want = P.trim_wav(wav)
        start, end = P.trim_bounds_device(torch.from_numpy(wav).to(dev))
        print("trim_wav %s: margin %.4g dB, %d -> %d samples, device bounds (%d, %d)" % (name, margin, wav.size, want.size, start, end))
        assert margin >= 1e-3, (name, margin)
        assert end - start == want.size and np.array_equal(wav[start:end], want), name
        if name.startswith("speech"):
            assert 0 < start < 9000 and wav.size - 7000 < end < wav.size, (name, start, end)
        else:
            assert (start, end) == (0, wav.size), name


def test_trim_silence_bounds_device_take_trim_silences_slice(dev):
    from nspeech_amd.datasets import process as P
    threshold = 0.02
    for name, wav in _trim_cases():
        margin = _trim_silence_margin_db(wav, threshold)
        want = P.trim_silence(wav, threshold)
        start, end = P.trim_silence_bounds_device(torch.from_numpy(wav).to(dev), threshold)
        print("trim_silence %s: margin %.4g dB, %d -> %d samples, device bounds (%d, %d)" % (name, margin, wav.size, want.size, start, end))
        assert margin >= 1e-3, (name, margin)
        assert end - start == want.size and np.array_equal(wav[start:end], want), name
        if name.startswith("speech"):
            assert 0 < start and end < wav.size, (name, start, end)
        elif name == "all silence":
            assert want.size == 0
        else:
            assert start == 0 and want.size > wav.size - 1024


def _write_wav_stereo(path, sr, seed):
    """PCM16 stereo WAV: 1.5 s of synthetic speech between 0.3 s and 0.2 s of faint noise, the second channel a scaled copy
    plus its own noise."""
    rng = np.random.default_rng(seed)
    body = _speech(seed, 1.5, sr)
    left = np.concatenate([rng.normal(0, 0.002, int(0.3 * sr)), body, rng.normal(0, 0.002, int(0.2 * sr))])
    right = 0.7 * left + rng.normal(0, 0.001, left.size)
    pcm = np.round(np.clip(np.stack([left, right], 1), -1, 1) * 32767).astype("<i2")
    with wave.open(path, "wb") as f:
        f.setnchannels(2)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes(pcm.tobytes())


def _write_flac_mono(path, sr, seed):
    rng = np.random.default_rng(seed)
    body = _speech(seed, 1.2, sr)
    x = np.concatenate([rng.normal(0, 0.002, int(0.25 * sr)), body, rng.normal(0, 0.002, int(0.25 * sr))])
    pcm = np.round(np.clip(x, -1, 1) * 32767).astype(np.int64)[:, None]
    frames, pos = [], 0
    while pos < len(pcm):
        size = min(4096, len(pcm) - pos)
        frames.append(dict(size=size, subframes=[dict(type="fixed", order=2, porder=3 if size == 4096 else 0)]))
        pos += size
    with open(path, "wb") as f:
        f.write(FW.encode(pcm, 16, sr, frames))


def test_device_chain_equals_the_host_chain_per_utterance(dev, tmp_path):
    from nspeech_amd.datasets import process as P
    from nspeech_amd.utils import audio as A
    _hp()
    wav_path, flac_path = str(tmp_path / "a.wav"), str(tmp_path / "b.flac")
    _write_wav_stereo(wav_path, 22050, 1)
    _write_flac_mono(flac_path, 16000, 2)
    for path in (wav_path, flac_path):
        host = A.load_wav(path)
        got = A.load_wav_device(path)
        assert got.is_cuda and got.dtype == torch.float32 and torch.equal(got, torch.from_numpy(host).to(dev)), path
        idx, wav, lin, mel, n_frames = P.process_utterance(path)
        didx, dwav, dlin, dmel, dn = P.process_utterance_device(path)
        assert didx == idx and dn == n_frames and dwav.is_cuda and dlin.is_cuda and dmel.is_cuda
        assert 0 < wav.size < host.size, "the fixture has silent ends to trim"
        assert torch.equal(dwav.cpu(), torch.from_numpy(np.ascontiguousarray(wav))), path
        assert torch.equal(dlin.cpu(), torch.from_numpy(np.ascontiguousarray(lin))), path
        assert torch.equal(dmel.cpu(), torch.from_numpy(np.ascontiguousarray(mel))), path
    host = A.load_wav(wav_path, offset=0.25, duration=0.8)
    got = A.load_wav_device(wav_path, offset=0.25, duration=0.8)
    assert host.size == int(int(0.8 * 22050) * (20000.0 / 22050.0)) and torch.equal(got.cpu(), torch.from_numpy(host))


def _corpus(tmp_path):
    lj, libre = str(tmp_path / "lj"), str(tmp_path / "libre")
    os.makedirs(os.path.join(lj, "wavs"))
    os.makedirs(libre)
    texts = ["Hello world.", "A short one.", "The quick brown fox.", "Speech from a file."]
    with open(os.path.join(lj, "metadata.csv"), "w") as f:
        for i, t in enumerate(texts):
            _write_wav_stereo(os.path.join(lj, "wavs", "utt%d.wav" % i), 22050, 10 + i)
            f.write("utt%d|%s|%s\n" % (i, t, t))
    with open(os.path.join(libre, "corpus.csv"), "w") as f:
        for i in range(2):
            _write_flac_mono(os.path.join(libre, "%d.flac" % i), 16000, 20 + i)
            f.write("7-1-%d,%d.flac,a reading of some text,train\n" % (i, i))
    return lj, libre


def test_datafeeder_device_front_end(dev, tmp_path, monkeypatch):
    """With device_cache and neither loader nor features the feeder runs the device chain on its own stream and caches
    the host chain's features bit for bit; no device-wide synchronise enters its thread."""
    from nspeech_amd.datasets.datafeeder import DataFeeder
    from nspeech_amd.utils import audio as A
    hp = _hp()
    hp.batch_size, hp.batch_group_size = 2, 3
    lj, libre = _corpus(tmp_path)
    host = DataFeeder(hp, ljspeech=lj, librispeech=libre, prefetch=False)
    assert host.front_end == "host"
    host.next_batch()
    assert len(host.cache) == 6

    def no_device_wide_sync(*a, **k):
        raise AssertionError("torch.cuda.synchronize() inside the feeder")
    fd = DataFeeder(hp, ljspeech=lj, librispeech=libre, device_cache=True)
    assert fd.front_end == "device"
    monkeypatch.setattr(torch.cuda, "synchronize", no_device_wide_sync)
    try:
        inputs, lengths, mel, lin = fd.next_batch()
    finally:
        fd.stop()
        monkeypatch.undo()
    assert torch.is_tensor(mel) and mel.is_cuda and mel.shape[0] == 2
    torch.cuda.synchronize()
    assert set(fd.cache) == set(host.cache)
    for path, (hmel, hlin) in host.cache.items():
        dmel, dlin = fd.cache[path]
        assert dmel.is_cuda and dlin.is_cuda
        assert torch.equal(dmel.cpu(), torch.from_numpy(hmel)) and torch.equal(dlin.cpu(), torch.from_numpy(hlin)), path

    with_loader = DataFeeder(hp, ljspeech=lj, device_cache=True, loader=A.load_wav, prefetch=False)
    assert with_loader.front_end == "host"
    with_loader.next_batch()
    for path, (dmel, dlin) in with_loader.cache.items():
        assert torch.equal(dmel.cpu(), torch.from_numpy(host.cache[path][0])), path
    assert DataFeeder(hp, ljspeech=lj, features=A.spectrogram_and_mel, device_cache=True, prefetch=False).front_end == "host"
    assert DataFeeder(hp, ljspeech=lj, prefetch=False).front_end == "host"
