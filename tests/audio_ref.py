"""Float64 contract of the audio kernels (csrc/audio.hip), stated from the parameter blocks of include/nspeech_hip.h:
every function takes the geometry (n_fft, hop, win), the tables as the caller supplies them and plain arrays - never the
hparams.  tests/test_audio_ref_cpu.py proves this module (independent formulations, planted errors, the conditions that
keep a bound from hiding a failure); tests/test_audio_contract_gpu.py holds every kernel form to it.  Both take their
cases from the tables at the end of this file.

Every transform has a `dt` argument.  dt = float64 is the reference.  dt = float32 is the EMULATION: the same
formulation with scipy.fft on float32 / complex64 data (single precision throughout) and the state rounded to float32
between the steps.  It is not a model of the kernels - they use other FFT factorizations - and it is used for one thing
only: its distance from the reference sizes the bounds (transform_delta, inverse_bound), next to a derived floor.

`plant` selects a deliberately wrong variant of a function (PLANTS); only the CPU module passes it."""
import functools
import math
from collections import namedtuple

import numpy as np
import scipy.fft

from test_audio_oracle import _speechlike

EPS = 2.0 ** -23                                  # float32 machine epsilon
FLT_MIN = float(np.finfo(np.float32).tiny)
f32, f64 = np.float32, np.float64

PLANTS = ("edge_pad", "preemph_neighbour", "window_at_start", "drop_fourth", "next_clip", "norm_by_window",
          "dc_nyquist_kept", "swap_bins", "no_momentum", "gt_zero")


def _cd(dt):
    return np.complex64 if dt == f32 else np.complex128


# ----------------------------------------------------------------------------------------------------------- the tables
def window_table(win):
    """Periodic Hann(win) as the caller supplies it: float32 of the float64 values."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)).astype(f32)


def twiddle_table(n_fft):
    """twiddle[m] = (cos, -sin)(2 pi m / n_fft), m < n_fft / 2: float32 [n_fft / 2, 2] of the float64 values."""
    a = 2.0 * np.pi * np.arange(n_fft // 2) / n_fft
    return np.stack([np.cos(a), -np.sin(a)], 1).astype(f32)


def mel_table(n_mels, n_fft, seed=0):
    """An arbitrary non-negative basis [n_mels, n_fft/2+1] float32: overlapping random bumps, about half the entries 0."""
    F = n_fft // 2 + 1
    rng = np.random.default_rng(1000 + seed)
    B = rng.uniform(0.0, 2.0 / math.sqrt(F), (n_mels, F)) * (rng.uniform(size=(n_mels, F)) < 0.5)
    return B.astype(f32)


@functools.lru_cache(maxsize=None)
def signal(L, seed):
    """The speech-like signal of the audio tests at a 0.5 peak plus white noise of sigma 0.05 (float32, read-only).  The
    noise floor is part of the input: without it the near-empty bins of a large transform make the feature intervals of
    feature_interval() wide (tests/test_audio_ref_cpu.py asserts the shares)."""
    y = _speechlike(L, seed).astype(f64)
    y = 0.5 * y / max(np.abs(y).max(), 1e-30) + np.random.default_rng(seed + 77).normal(0.0, 0.05, L)
    y = y.astype(f32)
    y.setflags(write=False)
    return y


# ------------------------------------------------------------------------------------------------------ filters, pointwise
def preemphasis(x, coef, dt=f64):
    """ns_preemphasis, inverse = 0: y[n] = x[n] - c x[n-1], zero initial state; c is the float32 the block carries."""
    x = np.asarray(x, dt)
    y = x.copy()
    y[1:] = x[1:] - dt(f32(coef)) * x[:-1]
    return y


def inv_preemphasis(x, coef):
    """ns_preemphasis, inverse = 1: y[n] = x[n] + c y[n-1], zero initial state (float64, one sample after the other)."""
    c, acc = float(f32(coef)), 0.0
    y = np.empty(len(x), f64)
    for i, v in enumerate(np.asarray(x, f64)):
        acc = v + c * acc
        y[i] = acc
    return y


def inv_preemphasis_blocked_f32(x, coef):
    """A float32 evaluation of the inverse filter in another association than the sample-after-sample one: tiles of 2048,
    blocks of 8 samples run in sequence, the blocks' affine maps (c^8, partial) combined by a Hillis-Steele scan, a carry
    from tile to tile - the association the kernel documents.  Only its distance from float64 is used (a bound)."""
    c = f32(coef)
    x = np.asarray(x, f32)
    n = len(x)
    y = np.empty(n, f32)
    c8 = f32(1.0)
    for _ in range(8):
        c8 = f32(c8 * c)
    carry = f32(0.0)
    for base in range(0, n, 2048):
        tile = np.zeros(2048, f32)
        m = min(2048, n - base)
        tile[:m] = x[base:base + m]
        tile = tile.reshape(256, 8)
        loc = np.empty((256, 8), f32)
        acc = np.zeros(256, f32)
        for j in range(8):
            acc = (tile[:, j] + c * acc).astype(f32)
            loc[:, j] = acc
        A, B = np.full(256, c8, f32), acc.copy()
        off = 1
        while off < 256:
            pa, pb = np.ones(256, f32), np.zeros(256, f32)
            pa[off:], pb[off:] = A[:-off], B[:-off]
            B = ((A * pb).astype(f32) + B).astype(f32)
            A = (A * pa).astype(f32)
            off *= 2
        ins = np.full(256, carry, f32)
        ins[1:] = ((A[:-1] * carry).astype(f32) + B[:-1]).astype(f32)
        pw = c
        out = np.empty((256, 8), f32)
        for j in range(8):
            out[:, j] = (loc[:, j] + (pw * ins).astype(f32)).astype(f32)
            pw = f32(pw * c)
        y[base:base + m] = out.reshape(-1)[:m]
        carry = f32(f32(A[255] * carry) + B[255])
    return y


def pointwise(x, mode, min_level_db):
    """ns_audio_pointwise: 0 amp_to_db, 1 db_to_amp, 2 normalize, 3 denormalize (float64 of the float32 inputs)."""
    x = np.asarray(x, f64)
    mn = float(f32(min_level_db))
    if mode == 0:
        return 20.0 * np.log10(np.maximum(float(f32(1e-5)), x))
    if mode == 1:
        return np.power(10.0, x * 0.05)
    if mode == 2:
        return np.clip((x - mn) / -mn, 0.0, 1.0)
    return np.clip(x, 0.0, 1.0) * -mn + mn


def pointwise_tolerance(x, mode, min_level_db):
    """Per element, from the number formats alone.
    0: log10f is good to 2 ulps, the product with 20 rounds once: 4 ulps of the result.
    1: the exponent e = x * 0.05f carries two roundings (the constant, the product), 2^-23 |e| at the most, which the
       power turns into a RELATIVE error ln(10) 2^-23 |e|; powf itself is good to 2 ulps: (4 + 2 ln(10) |e|) ulps.
    2: x - min rounds once (exact near the lower clamp: Sterbenz), the quotient once: 4 ulps of the unclipped result,
       which is exactly 1 once it is clipped.
    3: clip(x) * -min + min cancels near x = 1, so the roundings are ulps of the OPERANDS: 2 ulps of |min|."""
    x = np.asarray(x, f64)
    mn = abs(float(min_level_db))
    ref = pointwise(x, mode, min_level_db)
    if mode == 0:
        return 4 * EPS * np.abs(ref) + 2.0 ** -149
    if mode == 1:
        return (4 + 2 * math.log(10.0) * np.abs(x * 0.05)) * EPS * ref
    if mode == 2:
        return 4 * EPS * np.minimum(1.0, np.abs((x - float(f32(min_level_db))) / mn)) + 2.0 ** -149
    return np.full(x.shape, 2 * EPS * mn)


# ----------------------------------------------------------------------------------------------------------- transforms
def stft_center(y, n_fft, hop, win, window, preemph=0.0, dt=f64, plant=None):
    """The transform behind ns_spectrogram: pre-emphasis (fused in the kernel; 0 = none), reflect padding by n_fft / 2,
    frames every hop, the window centred in the n_fft frame at (n_fft - win) // 2.  [T, n_fft/2+1], T = 1 + L // hop."""
    y = np.asarray(y, dt)
    L, h = len(y), n_fft // 2
    assert L > h
    if plant == "preemph_neighbour":              # the filter run over the padded signal: x[i] - c x[i+1] where reflected
        yy = np.pad(y, h + 1, mode="reflect")
        yp = yy[1:-1] - dt(f32(preemph)) * yy[:-2]
    else:
        yp = np.pad(preemphasis(y, preemph, dt), h, mode="edge" if plant == "edge_pad" else "reflect")
    w = np.zeros(n_fft, dt)
    lpad = 0 if plant == "window_at_start" else (n_fft - win) // 2
    w[lpad:lpad + win] = np.asarray(window, dt)
    T = 1 + L // hop
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    return scipy.fft.rfft(yp[idx] * w, axis=1)


def tf_stft(y, n_fft, hop, win, window, dt=f64, T=None):
    """ns_stft_tf: frames of win samples every hop, windowed, zero-padded at the END to n_fft.  T = 1 + (L - win) // hop."""
    y = np.asarray(y, dt)
    T = 1 + (len(y) - win) // hop if T is None else T
    idx = np.arange(T)[:, None] * hop + np.arange(win)[None, :]
    return scipy.fft.rfft(y[idx] * np.asarray(window, dt), n=n_fft, axis=1)


def inverse_frames(S, n_fft, dt=f64, plant=None):
    """irfft of every row of S [T, n_fft/2+1]: the imaginary parts of DC and Nyquist are ignored.  The planted variant
    is what a half-size complex inverse (the merge of bins k and n_fft/2 - k) gives when it does not drop them."""
    S = np.asarray(S).astype(_cd(dt))
    S0 = S.copy()
    S0[:, 0] = S0[:, 0].real
    S0[:, -1] = S0[:, -1].real
    fr = scipy.fft.irfft(S0, n=n_fft, axis=1)
    if plant == "dc_nyquist_kept":
        b, d = S[:, 0].imag, S[:, -1].imag
        fr = fr.copy()
        fr[:, 0::2] -= ((b + d) / n_fft)[:, None]
        fr[:, 1::2] += ((b - d) / n_fft)[:, None]
    return fr.astype(dt)


def overlap_add(frames, hop, plant=None, nxt=None):
    """y[pos] = the sum of frames[f][pos - f hop] over the frames f < T that cover pos.  frames [T, win]."""
    T, win = frames.shape
    y = np.zeros((T - 1) * hop + win, frames.dtype)
    for t in range(T):
        fr = frames[t]
        if plant == "drop_fourth":                # only the three most recent covering frames of every sample
            pos = t * hop + np.arange(win)
            fr = np.where(np.minimum(pos // hop, T - 1) - t < 3, fr, 0)
        y[t * hop:t * hop + win] += fr
    if plant == "next_clip" and nxt is not None and win > hop:      # the frame index not clamped to T - 1
        y[T * hop:] += nxt[0][:win - hop]
    return y


def tf_istft(S, n_fft, hop, win, window, dt=f64, plant=None):
    """ns_istft, center = 0: irfft[:win] x window, overlap-add, no window-sum normalisation; [(T-1) hop + win]."""
    return overlap_add(inverse_frames(S, n_fft, dt, plant)[:, :win] * np.asarray(window, dt), hop, plant)


def istft_center(S, n_fft, hop, win, window, dt=f64, plant=None):
    """ns_istft, center = 1: the window centred in the n_fft frame, overlap-add, divided by the summed squared window
    where that exceeds FLT_MIN (elsewhere the sum stays as it is), n_fft / 2 trimmed at both ends; [(T-1) hop]."""
    w = np.asarray(window, dt)
    T = S.shape[0]
    lpad = (n_fft - win) // 2
    y = overlap_add(inverse_frames(S, n_fft, dt, plant)[:, lpad:lpad + win] * w, hop, plant)
    ws = overlap_add(np.tile(w if plant == "norm_by_window" else w * w, (T, 1)), hop)
    nz = ws > (0.0 if plant == "gt_zero" else FLT_MIN)
    y[nz] = y[nz] / ws[nz]
    shift = n_fft // 2 - lpad
    return y[shift:shift + (T - 1) * hop]


# --------------------------------------------------------------------------------------------------------------- features
def feature(m, ref_level_db, min_level_db):
    """_normalize(_amp_to_db(m) - ref_level_db): clip((20 log10(max(1e-5, m)) - ref - min) / -min, 0, 1)."""
    mn = float(f32(min_level_db))
    db = 20.0 * np.log10(np.maximum(float(f32(1e-5)), m)) - float(f32(ref_level_db))
    return np.clip((db - mn) / -mn, 0.0, 1.0)


def spectrogram(y, n_fft, hop, win, window, preemph, mel_basis, ref_level_db, min_level_db, dt=f64, plant=None):
    """ns_spectrogram: stft [T, F] complex, lin = feature(|stft|, ref, min), mel = feature(mel_basis . |stft|, 0, min)."""
    X = stft_center(y, n_fft, hop, win, window, preemph, dt, plant)
    mag = np.abs(X)
    melmag = mag @ np.asarray(mel_basis, dt).T
    return dict(stft=X, mag=mag, melmag=melmag, lin=feature(mag.astype(f64), ref_level_db, min_level_db),
                mel=feature(melmag.astype(f64), 0.0, min_level_db))


def transform_delta(ref, emu, n_fft):
    """Per frame: max(4 x the emulation's distance, 8 eps log2(n_fft) max |X|).  The second term is the classical FFT
    rounding bound eps log2 N ||x||_2 <= eps log2 N max |X| with headroom (8) for twiddles read from a float32 table."""
    return np.maximum(4 * np.abs(emu - ref).max(1), 8 * EPS * math.log2(n_fft) * np.abs(ref).max(1))


def feature_interval(m, delta, ref_level_db, min_level_db):
    """Where a feature of a magnitude known to within delta may lie: feature() is monotone in m, so
    [f(max(0, m - delta)), f(m + delta)] in the order its sign gives, widened by the roundings of the float32 dB chain
    (log10f 2 ulps, x 20, - ref, - min, x 1 / -min: 4 ulps of |dB| + |ref| + |min|, in units of |min|) and 2 ulps of the
    result.  Exact at both clamps, honest at near-empty bins."""
    a = feature(np.maximum(0.0, m - delta), ref_level_db, min_level_db)
    b = feature(m + delta, ref_level_db, min_level_db)
    db = np.abs(20.0 * np.log10(np.maximum(1e-5, m + delta)))
    wide = 4 * EPS * (db + abs(ref_level_db) + abs(min_level_db)) / abs(min_level_db) + 2 * EPS
    return np.minimum(a, b) - wide, np.maximum(a, b) + wide


def spectrogram_bounds(ref, emu, n_fft, mel_basis, ref_level_db, min_level_db):
    """delta per frame of the transform, and the intervals of lin and mel.  The magnitude adds one rounding of sqrtf;
    the mel sum goes through |basis| and adds the worst case of its float32 accumulation (F / 64 terms per lane and the
    six steps of the wave reduction, + 1 for the fused multiply)."""
    delta = transform_delta(ref["stft"], emu["stft"], n_fft)
    B = np.abs(np.asarray(mel_basis, f64))
    F = n_fft // 2 + 1
    dmag = delta[:, None] + EPS * ref["mag"]
    dmel = dmag @ B.T + (F / 64 + 7) * EPS * (ref["mag"] @ B.T)
    return dict(delta=delta, lin=feature_interval(ref["mag"], dmag, ref_level_db, min_level_db),
                mel=feature_interval(ref["melmag"], dmel, 0.0, min_level_db))


# ------------------------------------------------------------------------------------------------------------ Griffin-Lim
def gl_magnitude(spec, raw_magnitude, power, ref_level_db, min_level_db, dt=f64):
    """raw_magnitude 1: spec as it is.  0: (10^((clip(spec, 0, 1) * -min + min + ref) / 20))^power."""
    spec = np.asarray(spec, dt)
    if raw_magnitude:
        return spec
    mn, rf = dt(f32(min_level_db)), dt(f32(ref_level_db))
    db = np.clip(spec, 0, 1) * -mn + mn + rf
    return np.power(np.power(dt(10.0), db * dt(0.05)), dt(f32(power))).astype(dt)


def griffin_lim(S, n_fft, hop, win, window, iters, momentum=0.0, dt=f64, float32_state=False, plant=None):
    """ns_griffin_lim on magnitudes S [N, T, F]: y0 = ISTFT(S) (zero phase), E_prev = 0, then `iters` x { E = STFT(y);
    A = E - b E_prev (from the second iteration on); E_prev = E; y = ISTFT(S A / max(1e-8, |A|)) }, b = a / (1 + a) with
    a the float32 the block carries; TF-convention transforms.  Returns [N, (T-1) hop + win].  float32_state (dt float64
    only) rounds y and E to float32 after every transform, as tests/griffin_lim_ref.py does."""
    r32 = (lambda a: a.astype(f32).astype(f64)) if float32_state else (lambda a: a)
    c64 = (lambda a: a.astype(np.complex64).astype(np.complex128)) if float32_state else (lambda a: a)
    S = np.asarray(S, dt)
    N = S.shape[0]
    w = np.asarray(window, dt)
    a = float(f32(momentum))
    beta = dt(0.0 if plant == "no_momentum" else a / (1.0 + a))

    def ola_all(frames):
        return [r32(overlap_add(frames[n], hop, plant, frames[n + 1] if n + 1 < N else None)) for n in range(N)]

    y = ola_all([inverse_frames(S[n], n_fft, dt)[:, :win] * w for n in range(N)])
    prev = [None] * N
    for _ in range(iters):
        frames = []
        for n in range(N):
            E = c64(tf_stft(y[n], n_fft, hop, win, w, dt))
            A = E if (prev[n] is None or beta == 0) else E - beta * prev[n]
            prev[n] = E
            if plant == "swap_bins":
                A = A[:, ::-1]
            ang = A / np.maximum(dt(1e-8), np.abs(A))
            frames.append(inverse_frames(S[n] * ang, n_fft, dt)[:, :win] * w)
        y = ola_all(frames)
    return np.stack(y)


def inverse_bound(ref, emu, n_fft, iters, project):
    """For the inverse transforms and Griffin-Lim, relative to the reference's peak: the smaller of the project's
    existing bound and max(4 x the emulation's distance, the transform floor 8 eps log2(n_fft) times 2 (1 + iters))."""
    peak = np.abs(ref).max()
    return min(project, max(4 * np.abs(emu - ref).max() / peak, 8 * EPS * math.log2(n_fft) * 2 * (1 + iters)))


def gl_project_bound(iters):
    return 2e-4 if iters <= 1 else 5e-3           # tests/test_audio_gpu.py


ISTFT_PROJECT_BOUND = 2e-5                        # tests/test_audio_gpu.py


def gl_form(n_fft, hop, win, window_addr, work_addr):
    """The selection rule as include/nspeech_hip.h states it."""
    wave = (n_fft == 2048 and hop % 2 == 0 and win % 2 == 0 and win <= 4 * hop and win <= 1024
            and window_addr % 8 == 0 and work_addr % 8 == 0)
    return "wave" if wave else "generic"


def gl_work_floats(N, T, n_fft, win, momentum):
    """ns_griffin_lim_work_bytes() / 4, from the header's formula."""
    F = n_fft // 2 + 1
    return (4 * (((N * T * F + 1) & ~1) + 2 * N * T * win) + 256 + (16 * N * T * (n_fft // 4 + 1) if momentum > 0 else 0)) // 4


# ------------------------------------------------------------------------------------------------------------------ cases
GEOMETRIES = [      # (n_fft, hop, win), why - the transforms and the features
    ((64, 16, 64), "the smallest transform: a quarter of the 256 threads have a butterfly; win = n_fft, no centring"),
    ((64, 7, 24), "odd hop, n_fft - win = 40: most of the frame is zero padding"),
    ((128, 7, 27), "the small models' n_fft; odd win, odd n_fft - win: the centring offset rounds down"),
    ((256, 64, 64), "hop = win: one frame covers a sample, the window sum is 0 where Hann is 0; one butterfly per thread"),
    ((512, 50, 200), "four covering frames exactly; two butterflies per thread"),
    ((1024, 200, 800), "the second tested geometry of the suite"),
    ((2048, 250, 1000), "the shipped geometry"),
    ((4096, 400, 1600), "the largest transform, the largest LDS request"),
    ((4096, 1024, 4096), "the largest window: win = n_fft at the upper end"),
]

SpecCase = namedtuple("SpecCase", "geom L preemph n_mels ref_db min_db outs scale seed why")
IstftCase = namedtuple("IstftCase", "geom T center source why")
StftTfCase = namedtuple("StftTfCase", "geom T extra why")
GlCase = namedtuple("GlCase", "form geom T N iters momentum raw power min_db misalign why")


def spec_lengths(n_fft, hop):
    """n_fft/2 + 1 (the shortest admitted: the reflection reaches the other end), and one either side of a multiple of
    hop, raised to that minimum where 6 hop is shorter.  At most ten frames."""
    lo = n_fft // 2 + 1
    out = []
    for L in (lo, 6 * hop - 1, 6 * hop, 6 * hop + 1):
        L = max(L, lo)
        if L not in out:
            out.append(L)
    return out


def _spec_cases():
    cases = []
    for i, (g, why) in enumerate(GEOMETRIES):
        n_mels = (5, 7, 13, 6)[i % 4]             # none a multiple of the four waves of a workgroup
        for j, L in enumerate(spec_lengths(g[0], g[1])):
            seed = {0: 4, 80: 85}.get(10 * i + j, 10 * i + j)     # (two draws leave a frame too many near-empty bins)
            cases.append(SpecCase(g, L, 0.97, n_mels, 20.0, -100.0, "lin+mel+stft", 1.0, seed, why))
    big, small = GEOMETRIES[6][0], GEOMETRIES[2][0]
    cases += [
        SpecCase(big, 1501, 0.97, 80, 20.0, -100.0, "lin", 1.0, 91, "lin_out alone"),
        SpecCase(big, 1499, 0.97, 80, 20.0, -100.0, "mel", 1.0, 92, "mel_out alone; the shipped 80 mel rows"),
        SpecCase(small, 65, 0.5, 3, 20.0, -100.0, "mel", 1.0, 93, "mel_out alone with fewer rows than waves; another coefficient"),
        SpecCase(small, 71, 0.0, 5, 0.0, -100.0, "lin+stft", 1.0, 94, "no pre-emphasis (preemph == 0 never reads the neighbour); ref_level_db 0"),
        SpecCase(big, 1500, 0.97, 7, 20.0, -100.0, "lin+mel+stft", 1e-4, 95, "a quiet signal: a visible share on the lower clamp (and the 1e-5 floor)"),
        SpecCase(big, 1500, 0.97, 7, 0.0, 100.0, "lin+mel+stft", 1.0, 96, "the shipped min_level_db = +100: a visible share on the upper clamp"),
        SpecCase(GEOMETRIES[0][0], 96, 0.97, 5, 0.0, 100.0, "lin+mel+stft", 3.0, 97, "min_level_db = +100 at the smallest transform"),
    ]
    return cases


SPEC_CASES = _spec_cases()
QUIET_CASES = {95: "lower", 96: "upper", 97: "upper"}       # seed -> the clamp the case must show

STFT_TF_CASES = [StftTfCase(g, T, extra, why) for g, why in GEOMETRIES
                 for T, extra in ((1, 0), (6, 0), (6, 3))]  # L = (T-1) hop + win + extra: exact, and a few samples longer

ISTFT_CASES = [IstftCase(g, T, center, source, why) for g, why in GEOMETRIES for center in (0, 1)
               for T, source in ((6, "stft"), (5, "random"), (1, "random"))]
ISTFT_CASES += [IstftCase((256, 64, 64), 5, 1, "tiny_window", "window[0] = 1e-20: a window sum of 1e-40, positive and under FLT_MIN - not divided by")]

_WAVE = [((2048, 250, 1000), "the shipped geometry: win = 4 hop exactly"),
         ((2048, 300, 1000), "win no multiple of hop: the fourth slot covers only part of the frame"),
         ((2048, 256, 1024), "win = 1024, the form's upper end: every lane of every load has a sample"),
         ((2048, 1000, 1000), "hop = win: one covering frame, three empty slots"),
         ((2048, 2, 6), "a tiny window: one lane pair holds the frame, three covering frames")]
_GENERIC = [((2048, 250, 1000), "window at a 4-byte offset declines the wave form: both forms meet one reference on one input"),
            ((2048, 200, 1000), "five frames cover a sample: win > 4 hop"),
            ((2048, 250, 999), "odd win"),
            ((64, 16, 64), "M = 32: log2 M odd, radix-2 tail; a thread in eight has a radix-4 butterfly"),
            ((64, 7, 24), "odd hop, short window in the smallest transform"),
            ((128, 7, 27), "M = 64: pure radix-4 (no tail); the small models' n_fft; odd win"),
            ((512, 13, 200), "sixteen covering frames"),
            ((512, 50, 200), "M = 256: pure radix-4, one butterfly per four threads"),
            ((4096, 400, 1600), "M = 2048: radix-2 tail, two butterflies per thread"),
            ((4096, 1024, 4096), "the largest window")]
#            T  N iters momentum
_GL_RUNS = [(1, 1, 0, 0.0), (3, 3, 1, 0.0), (4, 1, 3, 0.0), (5, 3, 3, 0.99), (9, 1, 2, 0.99), (9, 3, 3, 0.0)]


def _gl_cases():
    cases = []
    for g, why in _WAVE:
        cases += [GlCase("wave", g, T, N, it, a, 1, 1.0, -100.0, False, why) for T, N, it, a in _GL_RUNS]
    for g, why in _GENERIC:
        mis = g == (2048, 250, 1000)
        for T, N, it, a in _GL_RUNS:
            if g == (512, 13, 200):
                T, N = 20, 1
            cases.append(GlCase("generic", g, T, N, it, a, 1, 1.0, -100.0, mis, why))
    for form, g, mis in (("wave", (2048, 250, 1000), False), ("generic", (1024, 200, 800), False)):
        for power in (1.0, 1.5):
            for mn in (-100.0, 100.0):
                cases.append(GlCase(form, g, 5, 1, 1, 0.0, 0, power, mn, mis, "raw_magnitude = 0: the magnitude conversion, power %g, min_level_db %+g" % (power, mn)))
    seen, out = set(), []
    for c in cases:                               # (512, 13, 200) folds its runs onto T = 20, N = 1
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


GL_CASES = _gl_cases()

POINTWISE_N = (1, 255, 257, 4096 * 256 + 5)
PREEMPH_N = (1, 7, 8, 9, 2047, 2048, 2049, 4097)
PREEMPH_N_LOOP = 1024 * 256 + 3
PREEMPH_COEFS = (0.97, 0.0, -0.97, 0.999)


def case_id(c):
    g = "%d-%d-%d" % c.geom
    if isinstance(c, SpecCase):
        return "%s-L%d-%s-s%d" % (g, c.L, c.outs, c.seed)
    if isinstance(c, IstftCase):
        return "%s-T%d-c%d-%s" % (g, c.T, c.center, c.source)
    if isinstance(c, StftTfCase):
        return "%s-T%d+%d" % (g, c.T, c.extra)
    return "%s-%s-T%d-N%d-i%d-a%g%s%s" % (c.form, g, c.T, c.N, c.iters, c.momentum, "" if c.raw else "-p%g-m%+g" % (c.power, c.min_db),
                                          "-off4" if c.misalign else "")


# ------------------------------------------------------------------------------------------- inputs and references per case
def spec_inputs(c):
    n_fft, hop, win = c.geom
    y = (signal(c.L, c.seed).astype(f64) * c.scale).astype(f32)
    return dict(wav=y, window=window_table(win), twiddle=twiddle_table(n_fft), mel_basis=mel_table(c.n_mels, n_fft, c.seed))


@functools.lru_cache(maxsize=None)
def spec_reference(c):
    """(reference, bounds) of a spectrogram case; computed once, shared, not to be written to."""
    n_fft, hop, win = c.geom
    x = spec_inputs(c)
    args = (x["wav"], n_fft, hop, win, x["window"], c.preemph, x["mel_basis"], c.ref_db, c.min_db)
    ref, emu = spectrogram(*args), spectrogram(*args, dt=f32)
    return ref, spectrogram_bounds(ref, emu, n_fft, x["mel_basis"], c.ref_db, c.min_db)


def stft_tf_inputs(c):
    n_fft, hop, win = c.geom
    return dict(wav=signal((c.T - 1) * hop + win + c.extra, 300 + c.T + c.extra), window=window_table(win), twiddle=twiddle_table(n_fft))


@functools.lru_cache(maxsize=None)
def stft_tf_reference(c):
    n_fft, hop, win = c.geom
    x = stft_tf_inputs(c)
    ref = tf_stft(x["wav"], n_fft, hop, win, x["window"], T=c.T)
    return ref, transform_delta(ref, tf_stft(x["wav"], n_fft, hop, win, x["window"], dt=f32, T=c.T), n_fft)


def istft_inputs(c):
    n_fft, hop, win = c.geom
    w = window_table(win)
    F = n_fft // 2 + 1
    if c.source == "stft":                        # the first T frames of the transform the inverse belongs to
        y = signal(max((c.T - 1) * hop + (0 if c.center else win), n_fft // 2 + 1), 400 + c.T)
        S = (stft_center(y, n_fft, hop, win, w) if c.center else tf_stft(y, n_fft, hop, win, w))[:c.T]
    else:                                         # random, DC and Nyquist with imaginary parts as large as the rest
        rng = np.random.default_rng(500 + c.T + n_fft + hop)
        S = rng.normal(size=(c.T, F)) + 1j * rng.normal(size=(c.T, F))
    if c.source == "tiny_window":
        w = w.copy()
        w[0] = 1e-20
    assert S.shape == (c.T, F)
    return dict(spec=S.astype(np.complex64), window=w, twiddle=twiddle_table(n_fft))


@functools.lru_cache(maxsize=None)
def istft_reference(c, plant=None):
    """(reference, relative bound); an empty reference (center = 1, T = 1) has the bound 0."""
    n_fft, hop, win = c.geom
    x = istft_inputs(c)
    fn = istft_center if c.center else tf_istft
    ref = fn(x["spec"], n_fft, hop, win, x["window"], plant=plant)
    if plant is not None or ref.size == 0:
        return ref, 0.0
    return ref, inverse_bound(ref, fn(x["spec"], n_fft, hop, win, x["window"], dt=f32), n_fft, 0, ISTFT_PROJECT_BOUND)


def gl_inputs(c):
    """spec [N, T, F] float32: consistent magnitudes |STFT(y)| of N different signals (raw_magnitude 1), or their
    normalised dB feature at ref 20 / min -100, a spectrogram in [0, 1] with real dynamics (raw_magnitude 0)."""
    n_fft, hop, win = c.geom
    w = window_table(win)
    S = np.stack([np.abs(tf_stft(signal((c.T - 1) * hop + win, 600 + 7 * n + c.T), n_fft, hop, win, w)) for n in range(c.N)])
    if not c.raw:
        S = feature(S, 20.0, -100.0)
    return dict(spec=S.astype(f32), window=w, twiddle=twiddle_table(n_fft))


@functools.lru_cache(maxsize=None)
def gl_reference(c, plant=None, momentum=None, float32_state=False):
    n_fft, hop, win = c.geom
    x = gl_inputs(c)
    S = gl_magnitude(x["spec"], c.raw, c.power, 20.0, c.min_db)
    return griffin_lim(S, n_fft, hop, win, x["window"], c.iters, c.momentum if momentum is None else momentum,
                       float32_state=float32_state, plant=plant)


@functools.lru_cache(maxsize=None)
def gl_bound(c):
    """Relative to each clip's reference peak.  raw_magnitude 1: inverse_bound().  raw_magnitude 0: the kernels form the
    magnitudes with the fast __powf (exp2(y log2 x), about 2^-21 |y log2 x| relative), which the emulation's powf does
    not show: the project's own bound (2e-4 up to one iteration, tests/test_audio_gpu.py) is the one in force."""
    n_fft, hop, win = c.geom
    if not c.raw:
        return gl_project_bound(c.iters)
    x = gl_inputs(c)
    ref = gl_reference(c)
    emu = griffin_lim(x["spec"], n_fft, hop, win, x["window"], c.iters, c.momentum, dt=f32)
    return min(inverse_bound(ref[n], emu[n], n_fft, c.iters, gl_project_bound(c.iters)) for n in range(c.N))


def is_momentum_case(c):
    return c.momentum > 0 and c.iters >= 2
