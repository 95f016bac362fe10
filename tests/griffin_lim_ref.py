"""Float64 reference of Griffin-Lim with the momentum update (ns_griffin_lim, include/nspeech_hip.h) on the oracle's
TF-convention transforms, and the figures the momentum tests share: the test signals' raw magnitudes and the spectral
convergence of a waveform against them."""
import functools

import numpy as np

from oracle import audio_oracle as AO
from test_audio_oracle import _speechlike

N_FFT, HOP, WIN = 2048, 250, 1000


def griffin_lim(S, n_fft, hop, win, iters, momentum=0.0, float32_state=False):
    """Zero initial phase, E_prev = 0, then `iters` x { E = STFT(y); A = E - b E_prev; E_prev = E;
    y = ISTFT(S A / max(1e-8, |A|)) } with b = momentum / (1 + momentum).  momentum = 0 is AO.griffin_lim_tf, operation
    for operation.  float32_state rounds y and E to float32 after every transform (what a float32 chain keeps between
    its steps): the distance to the unrounded result estimates the drift such a chain may show."""
    r32 = (lambda a: a.astype(np.float32).astype(np.float64)) if float32_state else (lambda a: a)
    c64 = (lambda a: a.astype(np.complex64).astype(np.complex128)) if float32_state else (lambda a: a)
    beta = momentum / (1.0 + momentum)
    Sc = np.asarray(S).astype(np.complex128)
    y = r32(AO.tf_istft(Sc, n_fft, hop, win))
    prev = None
    for _ in range(iters):
        est = c64(AO.tf_stft(y, n_fft, hop, win))
        a = est if (prev is None or beta == 0.0) else est - beta * prev
        prev = est
        angles = a / np.maximum(1e-8, np.abs(a))
        y = r32(AO.tf_istft(Sc * angles, n_fft, hop, win))
    return y


def spectral_convergence(y, S, n_fft=N_FFT, hop=HOP, win=WIN):
    """|| g |STFT(y)| - S || / || S || with the least-squares gain g (the un-normalised inverse transform leaves a
    constant round-trip gain on y, which is not what the iterations are judged by)."""
    m = np.abs(AO.tf_stft(np.asarray(y, np.float64), n_fft, hop, win))
    g = (m * S).sum() / (m * m).sum()
    return float(np.linalg.norm(g * m - S) / np.linalg.norm(S))


@functools.lru_cache(maxsize=None)
def magnitudes(seed, T, n_fft=N_FFT, hop=HOP, win=WIN):
    """Consistent raw magnitudes |STFT(y)| [T, n_fft/2+1] float32 of a speech-like signal (read-only: shared)."""
    S = np.abs(AO.tf_stft(_speechlike((T - 1) * hop + win, seed), n_fft, hop, win)).astype(np.float32)
    assert S.shape == (T, n_fft // 2 + 1)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def reference(seed, T, iters, momentum, n_fft=N_FFT, hop=HOP, win=WIN):
    """griffin_lim of magnitudes(seed, T) in float64, computed once per setting (read-only: shared)."""
    y = griffin_lim(magnitudes(seed, T, n_fft, hop, win).astype(np.float64), n_fft, hop, win, iters, momentum)
    y.setflags(write=False)
    return y
