"""Griffin-Lim with the momentum update on the GPU (both kernel forms of ns_griffin_lim) against the float64 reference of
tests/griffin_lim_ref.py, on consistent raw magnitudes |STFT(y)| of speech-like signals.

Bounds: the project's own for Griffin-Lim (tests/test_audio_gpu.py), relative to the reference's peak - 2e-4 up to one
iteration, 5e-3 above.  Rounding the reference's state to float32 after every transform moves it by at most 3.8e-5 of
the peak on these inputs (30 iterations), so the fp32 kernel chain has room; and every case of two or more iterations
first shows that the float64 PLAIN result lies further from the momentum reference than the bound (8.8e-3 of the peak
at the least), so a kernel that ignores `momentum` cannot pass."""
import ctypes as C

import numpy as np
import pytest
import torch

import griffin_lim_ref as R
from test_wavenet_hold_gpu import TACO_SMALL

pytestmark = pytest.mark.gpu

GENERIC = (1024, 200, 800)                      # n_fft / hop / win of the one-workgroup-per-frame form
TEXTS = ["Hello, World.", "Dr. Jones arrived at 9 o'clock.", "Yes."]


@pytest.fixture()
def audio(dev):
    from nspeech_amd import hparams
    from nspeech_amd.utils import audio as A
    keep = hparams.get_hparams()
    hp = hparams.load("taco2")
    yield A, hp
    hparams.set_hparams(keep)


@pytest.fixture()
def generic(audio):
    """num_freq 513 at 16 kHz: n_fft 1024, hop 200, win 800 - not the wave-per-frame kernel's size."""
    A, hp = audio
    hp.num_freq, hp.sample_rate = 513, 16000
    assert A._stft_parameters() == GENERIC
    return A, hp


def _gl(A, S, iters, momentum=None):
    kw = {} if momentum is None else dict(momentum=momentum)
    return A.griffin_lim_gpu(np.array(S, dtype=np.float32), iters=iters, raw_magnitude=True, **kw).cpu().numpy()   # (a copy: the shared magnitudes are read-only)


def _check(got, seed, T, iters, a, geom=()):
    ref = R.reference(seed, T, iters, a, *geom)
    peak = np.abs(ref).max()
    tol = 2e-4 if iters <= 1 else 5e-3
    err = np.abs(got - ref).max() / peak
    print("seed %d T %d momentum %g iters %d: error %.3g of the peak (bound %g)" % (seed, T, a, iters, err, tol))
    assert got.shape == ref.shape and np.isfinite(got).all()
    if iters >= 2:
        away = np.abs(R.reference(seed, T, iters, 0.0, *geom) - ref).max() / peak
        assert away > tol, away
    assert err < tol, (seed, T, iters, a, err)


@pytest.mark.parametrize("iters", [1, 2, 5, 30])
@pytest.mark.parametrize("a", [0.5, 0.99])
def test_wave_kernel_two_clips_of_41_frames(audio, a, iters):
    """T = 41 is not a multiple of the four frames of a workgroup: the surplus waves leave beside the history loads."""
    A, hp = audio
    got = _gl(A, np.stack([R.magnitudes(6, 41), R.magnitudes(7, 41)]), iters, a)
    assert got.shape == (2, 40 * 250 + 1000)
    _check(got[0], 6, 41, iters, a)
    _check(got[1], 7, 41, iters, a)


@pytest.mark.parametrize("seed,T,iters", [(9, 5, 1), (9, 5, 2), (9, 5, 5), (9, 5, 30), (10, 1, 1), (10, 1, 2), (10, 1, 5)])
@pytest.mark.parametrize("a", [0.5, 0.99])
def test_wave_kernel_few_frames_and_one_frame(audio, a, seed, T, iters):
    A, hp = audio
    _check(_gl(A, R.magnitudes(seed, T), iters, a), seed, T, iters, a)


@pytest.mark.parametrize("iters", [1, 2, 5, 30])
@pytest.mark.parametrize("a", [0.5, 0.99])
def test_generic_kernel(generic, a, iters):
    A, hp = generic
    _check(_gl(A, R.magnitudes(11, 25, *GENERIC), iters, a), 11, 25, iters, a, GENERIC)


@pytest.mark.parametrize("form", ["wave", "generic"])
def test_bit_identities(audio, form):
    A, hp = audio
    geom = ()
    if form == "generic":
        hp.num_freq, hp.sample_rate = 513, 16000
        geom = GENERIC
    S = np.stack([R.magnitudes(6, 41, *geom), R.magnitudes(7, 41, *geom)])
    for iters in (0, 1, 5):
        assert np.array_equal(_gl(A, S, iters, 0.0), _gl(A, S, iters)), iters             # off = the call without it
    plain1 = _gl(A, S, 1)
    for a in (0.5, 0.99):
        assert np.array_equal(_gl(A, S, 1, a), plain1), a                                # no history in iteration 1
    both = _gl(A, S, 5, 0.99)
    assert not np.array_equal(both, _gl(A, S, 5))
    for i in range(2):
        assert np.array_equal(both[i], _gl(A, S[i], 5, 0.99)), i                         # rows = the single clips
    assert np.array_equal(both, _gl(A, S, 5, 0.99))                                      # and the call repeats itself


def _direct(A, S, iters, momentum, fill):
    """ns_griffin_lim as griffin_lim_gpu calls it, on a work area (and an output) the caller filled with `fill`."""
    from nspeech_amd import _lib as L, ops
    n_fft, hop, win = A._stft_parameters()
    tb = A._get_tables()
    st = torch.as_tensor(np.asarray(S)).to("cuda", torch.float32).contiguous()
    N, T, F = st.shape
    Lout = (T - 1) * hop + win
    wav = torch.full((N, Lout), fill, dtype=torch.float32, device="cuda")
    p = L.struct("ns_griffin_lim_params")
    p.spec, p.N, p.T = ops.ptr(st), N, T
    p.n_fft, p.hop, p.win, p.iters = n_fft, hop, win, iters
    p.power, p.ref_level_db, p.min_level_db = 1.5, 20.0, 100.0
    p.window, p.twiddle, p.wav = ops.ptr(tb["window"]), ops.ptr(tb["twiddle"]), ops.ptr(wav)
    p.raw_magnitude, p.momentum = 1, momentum
    nbytes = L.lib().ns_griffin_lim_work_bytes
    nbytes.restype = C.c_size_t
    work = torch.full(((nbytes(C.byref(p)) + 3) // 4,), fill, dtype=torch.float32, device="cuda")
    p.work = ops.ptr(work)
    L.call("ns_griffin_lim", p, ops.stream())
    return wav.cpu().numpy()


@pytest.mark.parametrize("form", ["wave", "generic"])
def test_a_work_area_full_of_nan_is_harmless(audio, form):
    """The first iteration only stores the history: nothing the caller left in the work area is ever read."""
    A, hp = audio
    geom = ()
    if form == "generic":
        hp.num_freq, hp.sample_rate = 513, 16000
        geom = GENERIC
    S = np.stack([R.magnitudes(6, 41, *geom), R.magnitudes(7, 41, *geom)])
    got = _direct(A, S, 5, 0.99, float("nan"))
    assert np.isfinite(got).all()
    assert np.array_equal(got, _gl(A, S, 5, 0.99))
    _check(got[0], 6, 41, 5, 0.99, geom)


def test_convergence_on_the_device(audio):
    """Thirty iterations with momentum reach what sixty plain ones reach - judged on the GPU's own waveforms."""
    A, hp = audio
    S = R.magnitudes(6, 41)
    S64 = S.astype(np.float64)
    sc_ref = R.spectral_convergence(R.reference(6, 41, 30, 0.99), S64)
    sc_mom = R.spectral_convergence(_gl(A, S, 30, 0.99), S64)
    sc_plain = R.spectral_convergence(_gl(A, S, 60, 0.0), S64)
    print("SC: GPU (0.99, 30) %.5f, reference %.5f, GPU (0, 60) %.5f" % (sc_mom, sc_ref, sc_plain))
    assert abs(sc_mom - sc_ref) <= 0.01 * sc_ref
    assert sc_mom <= 1.05 * sc_plain


def test_the_hparam_reaches_the_vocoder_functions(audio):
    from oracle import audio_oracle as AO
    from test_audio_oracle import HP, _speechlike
    A, hp = audio
    spec = AO.spectrogram(_speechlike(30 * 250 + 1000, 6), dict(HP, min_level_db=-100)).T[:31].copy()     # [T, F] in [0, 1]
    off = A.inv_spectrogram_tensorflow(spec)
    assert np.array_equal(off, A.griffin_lim_gpu(spec, momentum=0.0).cpu().numpy())
    hp.griffin_lim_momentum = 0.99
    on = A.inv_spectrogram_tensorflow(spec)
    assert np.array_equal(on, A.griffin_lim_gpu(spec, momentum=0.99).cpu().numpy())
    assert np.isfinite(on).all() and not np.array_equal(on, off)
    assert np.array_equal(A.inv_spectrogram(spec.T), A.inv_preemphasis(on))
    hp.griffin_lim_momentum = 0.0
    assert np.array_equal(A.inv_spectrogram_tensorflow(spec), off)


def test_synthesize_batch_follows_the_hparam(dev):
    """The small Tacotron-2 of tests/test_synth_batch_gpu.py: with griffin_lim_momentum set, every row of
    synthesize_batch is the single-clip functions under the same hparam, and synthesize follows it as well."""
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.synthesizer import Synthesizer, pad_text_batch
    from nspeech_amd.utils import audio as A
    from nspeech_amd.utils.text import text_to_sequence
    keep = hparams_mod.get_hparams()
    try:
        hp = hparams_mod.load("taco2")
        for k, v in TACO_SMALL.items():
            setattr(hp, k, v)
        hp.parse("griffin_lim_momentum=0.99,griffin_lim_iters=30")
        hparams_mod.set_hparams(hp)
        synth = Synthesizer(hp, dtype="bf16").load(None, "taco2")
        got = synth.synthesize_batch(TEXTS)
        m = synth.model
        names = [x.strip() for x in hp.cleaners.split(",")]
        inputs, lengths = pad_text_batch([text_to_sequence(t, names) for t in TEXTS])
        m.initialize(inputs, lengths, np.zeros(3, np.int32))
        lin = m.linear_outputs.clone()
        m.check_status()
        for i in range(3):
            raw = A.griffin_lim_gpu(lin[i].contiguous(), iters=30, momentum=0.99).cpu().numpy()
            assert np.array_equal(A.inv_spectrogram_tensorflow(lin[i].contiguous()).cpu().numpy(), raw)
            want = A.inv_preemphasis(raw)
            want = want[:A.find_endpoint(want)]
            assert len(want) > 0 and np.isfinite(want).all()
            assert np.array_equal(got[i][0], want), (i, len(got[i][0]), len(want))
        wav, _, lin1 = synth.synthesize(TEXTS[2])
        want = A.inv_preemphasis(A.griffin_lim_gpu(m.linear_outputs[0].contiguous(), iters=30, momentum=0.99).cpu().numpy())
        assert np.array_equal(wav, want[:A.find_endpoint(want)])
    finally:
        hparams_mod.set_hparams(keep)
