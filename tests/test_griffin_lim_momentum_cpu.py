"""The momentum update of Griffin-Lim without a GPU: the float64 reference itself (tests/griffin_lim_ref.py), what the
update buys in iterations, the C ABI as the binding sees it (the new field, the work area, the refusals - all before any
launch) and the hparam."""
import ctypes as C

import numpy as np
import pytest

import griffin_lim_ref as R
from oracle import audio_oracle as AO

SIGNALS = [(6, 41), (7, 41), (1234, 101)]          # (seed, frames)


def test_reference_without_momentum_is_the_oracle():
    S = R.magnitudes(6, 41).astype(np.float64)
    for iters in (0, 1, 5):
        assert np.array_equal(R.griffin_lim(S, R.N_FFT, R.HOP, R.WIN, iters, 0.0), AO.griffin_lim_tf(S, R.N_FFT, R.HOP, R.WIN, iters))
    # the first iteration has no history: any momentum gives the plain one
    assert np.array_equal(R.griffin_lim(S, R.N_FFT, R.HOP, R.WIN, 1, 0.99), AO.griffin_lim_tf(S, R.N_FFT, R.HOP, R.WIN, 1))


def test_reference_float32_state_drift_is_far_inside_the_gpu_bound():
    S = R.magnitudes(6, 41).astype(np.float64)
    ref = R.reference(6, 41, 30, 0.99)
    drift = np.abs(R.griffin_lim(S, R.N_FFT, R.HOP, R.WIN, 30, 0.99, float32_state=True) - ref).max() / np.abs(ref).max()
    print("float32-state drift at (0.99, 30): %.3g of the peak" % drift)
    assert drift < 5e-4                                  # a tenth of the 5e-3 the GPU tests allow


@pytest.mark.parametrize("seed,T", SIGNALS)
def test_momentum_reaches_in_half_the_iterations_what_the_plain_update_reaches(seed, T):
    S = R.magnitudes(seed, T).astype(np.float64)
    sc = {(a, it): R.spectral_convergence(R.reference(seed, T, it, a), S) for a, it in ((0.0, 30), (0.0, 60), (0.99, 20), (0.99, 30))}
    print("seed %d T %d: " % (seed, T) + ", ".join("SC(%g, %d) = %.4f" % (a, it, v) for (a, it), v in sc.items()))
    assert sc[(0.99, 30)] <= 1.05 * sc[(0.0, 60)]
    assert sc[(0.99, 20)] < sc[(0.0, 30)]


# ---------------------------------------------------------------- the C ABI, through the loaded library, no device
def _params(**over):
    """A call that would be valid: the pointers point into host buffers that a refused call never reads."""
    from nspeech_amd import _lib
    buf = (C.c_float * 16)()
    p = _lib.struct("ns_griffin_lim_params")
    p.spec = p.window = p.twiddle = p.wav = p.work = C.addressof(buf)
    p.N, p.T, p.n_fft, p.hop, p.win, p.iters = 2, 41, 2048, 250, 1000, 5
    p.power, p.ref_level_db, p.min_level_db, p.raw_magnitude = 1.5, 20.0, 100.0, 1
    for k, v in over.items():
        setattr(p, k, v)
    p._keep = buf
    return p


def _work_bytes(p):
    from nspeech_amd import _lib
    fn = _lib.lib().ns_griffin_lim_work_bytes
    fn.restype = C.c_size_t
    return fn(C.byref(p))


def test_momentum_is_the_last_field_and_a_zeroed_struct_means_off():
    from nspeech_amd import _lib
    p = _lib.struct("ns_griffin_lim_params")
    assert p._fields_[-1] == ("momentum", C.c_float)
    assert [f[0] for f in p._fields_][-3:] == ["work", "raw_magnitude", "momentum"]
    assert p.momentum == 0.0


@pytest.mark.parametrize("N,T,n_fft,win", [(2, 41, 2048, 1000), (1, 1, 2048, 1000), (1, 25, 1024, 800), (32, 797, 2048, 1000),
                                           (3, 7, 4096, 999)])
def test_work_bytes(N, T, n_fft, win):
    F = n_fft // 2 + 1
    today = 4 * (((N * T * F + 1) & ~1) + 2 * N * T * win) + 256
    off = _work_bytes(_params(N=N, T=T, n_fft=n_fft, win=win, momentum=0.0))
    on = _work_bytes(_params(N=N, T=T, n_fft=n_fft, win=win, momentum=0.99))
    assert off == today
    assert today < on <= today + 8 * N * T * (n_fft // 2 + 2)
    assert on == today + 16 * N * T * (n_fft // 4 + 1)                  # the formula the header states
    assert _work_bytes(_params(N=N, T=T, n_fft=n_fft, win=win, momentum=0.5)) == on


@pytest.mark.parametrize("bad", [1.0, -0.1, float("nan"), 1.5, float("inf")])
def test_momentum_outside_the_unit_interval_is_refused_with_a_message(bad):
    from nspeech_amd import _lib
    lib = _lib.lib()
    assert lib.ns_griffin_lim(C.byref(_params(momentum=bad)), C.c_void_p(0)) == -1          # NS_ERR_BAD_ARG
    assert lib.ns_last_error().decode().startswith("ns_griffin_lim: momentum")
    with pytest.raises(_lib.NSError, match="momentum"):
        _lib.call("ns_griffin_lim", _params(momentum=bad), 0)


def test_nothing_to_do_is_a_success_without_a_launch():
    from nspeech_amd import _lib
    assert _lib.lib().ns_griffin_lim(C.byref(_params(N=0, momentum=0.99)), C.c_void_p(0)) == 0
    assert _lib.lib().ns_griffin_lim(C.byref(_params(T=0, momentum=0.5)), C.c_void_p(0)) == 0


# ---------------------------------------------------------------- the hparam
def test_hparam_default_is_off_and_an_override_takes():
    from nspeech_amd import hparams
    keep = hparams.get_hparams()
    try:
        hp = hparams.load("taco2")
        assert hp.griffin_lim_momentum == 0.0 and isinstance(hp.griffin_lim_momentum, float)
        hp.parse("griffin_lim_momentum=0.99,griffin_lim_iters=30")
        assert hp.griffin_lim_momentum == 0.99 and hp.griffin_lim_iters == 30
        assert hparams.load("taco1").griffin_lim_momentum == 0.0
    finally:
        hparams.set_hparams(keep)
