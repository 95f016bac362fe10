"""Every kernel of csrc/audio.hip (ns_spectrogram, ns_stft_tf, ns_istft, both forms of ns_griffin_lim with their three
momentum variants, ns_audio_pointwise, ns_preemphasis) against the float64 contract of tests/audio_ref.py (itself proven
by tests/test_audio_ref_cpu.py), called through _lib.struct / _lib.call with this module's own tables - never through
utils.audio, whose hparams reach two geometries.  The case tables, with one line per case on what it is for, are at the
end of tests/audio_ref.py.  A case a launcher refuses fails; nothing is skipped.

Every case: each output lies between sentinel margins (MARGIN floats on either side) and is prefilled with the
sentinel; the work areas (ns_griffin_lim_work_bytes(), T * win floats for ns_istft) are prefilled with NaN and followed
by a guard tail; the call runs twice on the same buffers and the second result, which must equal the first bit for bit
(it starts from what the first left in the work area), is the one compared; every element is compared; afterwards the
margins and tails still hold the sentinel and every input is bit-identical.

Tolerances - none is taken from a kernel's output, none is looser than what tests/test_audio_gpu.py holds the same
quantity to (the CPU module asserts that per case):
  transforms  per frame delta = max(4 x the distance of the float32 emulation from float64, 8 eps log2(n_fft) max |X| of
              the frame).  The second term - the classical FFT rounding bound eps log2 N ||x||_2 <= eps log2 N max |X|,
              with headroom for float32 table twiddles - decided in every case: the emulation lies 0.2e-7 to 2.1e-7 of
              max |X| from float64 (4 x that is 0.15 of the floor at the most; 0.58 for ns_istft).  About 1e-5 of the peak at n_fft 2048 where the suite had 2e-4.
  features    lin_out and mel_out are monotone in the magnitude: a value must lie in [f(max(0, m - d)), f(m + d)],
              d = delta + one rounding of sqrtf (through |basis| and the worst case of the float32 sum for mel), widened
              by the roundings of the float32 dB chain (audio_ref.feature_interval).  Exact at both clamps.
  inverses    relative to the reference's peak (per clip): min(the project's bound, max(4 x the emulation's distance,
              the transform floor 8 eps log2(n_fft) x 2 (1 + iters))); the project's bounds are 2e-5 for ns_istft and
              2e-4 up to one iteration / 5e-3 above for Griffin-Lim.  With raw_magnitude = 0 the kernels form the
              magnitudes with the fast __powf, which the emulation does not show: there the project's 2e-4 is in force.
  pointwise   from the number formats (audio_ref.pointwise_tolerance): 4 ulps of the result for modes 0 and 2, 2 ulps
              of |min_level_db| for mode 3 (it cancels near 1), (4 + 2 ln(10) |x| / 20) ulps relative for mode 1.
  filters     forward: one ulp of |x[n]| + |c x[n-1]| (a product and a sum, or one fused step).  Inverse: 4 x the
              distance from float64 of a float32 evaluation in the kernel's association (blocks of 8, scanned), of the
              peak - which is 0 at coef 0, where the kernel must be exact.

Found by this module: no kernel was found wrong.  All 352 cases met every bound at the first run on the MI355X, nothing
outside an output's or a work area's extent was written, no input was touched and every second call repeated the first
bit for bit.  What the header did not say and now does: the accepted ranges and refusals, the two Griffin-Lim forms and
the rule that picks one (the 8-byte alignment of `window` and `work` included), that ns_istft ignores the imaginary
parts of DC and Nyquist (in its full-size complex transform they cannot reach the real part; the statement binds any
later half-size form) and stores the undivided sum where the window sum is FLT_MIN or less, the extents, and the
in-place inverse filter.  Its "Radix-2 ... one workgroup per frame" sentence described one of three transforms.

Worst error / bound per kernel and form on the MI355X over all cases (every test prints its own, `pytest -s`); the
module takes 2.2 s of wall time there, 352 tests, none above 0.25 s:
  ns_spectrogram    stft_out 0.029   lin_out 0.068   mel_out 0.044   (of the interval's half towards the error)
  ns_stft_tf        0.025
  ns_istft          center 0: 0.012   center 1: 0.423 (256-64-64, hop = win: the quotient by a small window sum)
  ns_griffin_lim    wave form:    plain 0.036   momentum 0.031   raw_magnitude 0: 0.004 (of the project's 2e-4)
                    generic form: plain 0.121   momentum 0.106   raw_magnitude 0: 0.004
                    (both worst generic figures at 512-13-200, sixteen covering frames)
  ns_audio_pointwise   mode 0: 0.526   1: 0.279   2: 0.219   3: 0.160
  ns_preemphasis    forward 0.941 (one ulp of the operands is all it is allowed)   inverse 0.451, exact at coef 0
The transforms sit at 1 / 35 of delta and below: the derived floor carries the factor 8 for table twiddles, and the
kernels' error is that of the float32 emulation (1e-7 to 3e-7 of max |X|)."""
import ctypes as C

import numpy as np
import pytest
import torch

import audio_ref as R

pytestmark = pytest.mark.gpu

MARGIN = 64                                       # floats on either side of an output (256 bytes: alignment is kept)
GUARD = 4096                                      # floats behind a work area
SENTINEL = -1234.5
f32, f64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------- buffers
class Out:
    """n floats between two margins, all prefilled with the sentinel."""

    def __init__(self, n, tail=MARGIN, fill=SENTINEL):
        self.n, self.tail = n, tail
        self.buf = torch.full((MARGIN + n + tail,), SENTINEL, dtype=torch.float32, device="cuda")
        self.buf[MARGIN:MARGIN + n] = fill
        self.ptr = self.buf.data_ptr() + 4 * MARGIN

    def get(self):
        return self.buf[MARGIN:MARGIN + self.n].cpu().numpy()

    def intact(self):
        return bool((self.buf[:MARGIN] == SENTINEL).all()) and bool((self.buf[MARGIN + self.n:] == SENTINEL).all())


class In:
    """A device copy of a host array, `off` floats behind an aligned address; compared bit for bit afterwards."""

    def __init__(self, a, off=0):
        self.host = np.ascontiguousarray(a)
        flat = torch.from_numpy(self.host.view(f32).reshape(-1).copy())
        self.buf = torch.zeros(off + flat.numel(), dtype=torch.float32, device="cuda")
        self.buf[off:] = flat.cuda()
        self.off = off
        self.ptr = self.buf.data_ptr() + 4 * off

    def unchanged(self):
        return np.array_equal(self.buf[self.off:].cpu().numpy().view(np.uint32), self.host.view(np.uint32).reshape(-1))


def _twice(entry, p, outs):
    """Run the call twice; returns the second results, which must be the first bit for bit."""
    from nspeech_amd import _lib, ops
    _lib.call(entry, p, ops.stream())
    first = [o.get() for o in outs]
    _lib.call(entry, p, ops.stream())
    second = [o.get() for o in outs]
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), entry + ": the second call differs from the first"
    return second


def _geometry(p, c_geom):
    p.n_fft, p.hop, p.win = c_geom


# ------------------------------------------------------------------------------------------------------- ns_spectrogram
@pytest.mark.parametrize("c", R.SPEC_CASES, ids=R.case_id)
def test_spectrogram(dev, c):
    from nspeech_amd import _lib
    n_fft, hop, win = c.geom
    F, T = n_fft // 2 + 1, 1 + c.L // hop
    x = R.spec_inputs(c)
    ref, b = R.spec_reference(c)
    ins = {k: In(v) for k, v in x.items()}
    outs = {"lin": Out(T * F), "mel": Out(T * c.n_mels), "stft": Out(2 * T * F)}
    want = c.outs.split("+")
    p = _lib.struct("ns_spectrogram_params")
    p.wav, p.L, p.preemph, p.T = ins["wav"].ptr, c.L, c.preemph, T
    _geometry(p, c.geom)
    p.window, p.twiddle, p.mel_basis, p.n_mels = ins["window"].ptr, ins["twiddle"].ptr, ins["mel_basis"].ptr, c.n_mels
    p.ref_level_db, p.min_level_db = c.ref_db, c.min_db
    p.lin_out = outs["lin"].ptr if "lin" in want else None
    p.mel_out = outs["mel"].ptr if "mel" in want else None
    p.stft_out = outs["stft"].ptr if "stft" in want else None
    got = dict(zip(want, _twice("ns_spectrogram", p, [outs[k] for k in want])))
    assert all(o.intact() for o in outs.values()) and all(i.unchanged() for i in ins.values())
    for k in outs:
        if k not in want:
            assert (outs[k].get() == SENTINEL).all(), k + " was not asked for"
    fig = []
    if "stft" in want:
        X = got["stft"].astype(f64).reshape(T, F, 2)
        X = X[:, :, 0] + 1j * X[:, :, 1]
        assert np.isfinite(got["stft"]).all()
        r = (np.abs(X - ref["stft"]).max(1) / b["delta"]).max()
        fig.append("stft %.3f" % r)
        assert r <= 1.0, ("stft", r)
    for k, n in (("lin", F), ("mel", c.n_mels)):
        if k in want:
            v = got[k].astype(f64).reshape(T, n)
            lo, hi = b[k]
            assert np.isfinite(v).all()
            r = np.maximum((v - ref[k]) / (hi - ref[k]), (ref[k] - v) / (ref[k] - lo)).max()
            fig.append("%s %.3f (worst |error| %.2g)" % (k, r, np.abs(v - ref[k]).max()))
            assert ((lo <= v) & (v <= hi)).all(), (k, r)
    print("spectrogram %s: error / bound  %s" % (R.case_id(c), "  ".join(fig)))


# ------------------------------------------------------------------------------------------------------------ ns_stft_tf
@pytest.mark.parametrize("c", R.STFT_TF_CASES, ids=R.case_id)
def test_stft_tf(dev, c):
    from nspeech_amd import _lib
    n_fft, hop, win = c.geom
    F = n_fft // 2 + 1
    x = R.stft_tf_inputs(c)
    ref, delta = R.stft_tf_reference(c)
    ins = {k: In(v) for k, v in x.items()}
    out = Out(2 * c.T * F)
    p = _lib.struct("ns_stft_tf_params")
    p.wav, p.L, p.T = ins["wav"].ptr, len(x["wav"]), c.T
    _geometry(p, c.geom)
    p.window, p.twiddle, p.out = ins["window"].ptr, ins["twiddle"].ptr, out.ptr
    got, = _twice("ns_stft_tf", p, [out])
    assert out.intact() and all(i.unchanged() for i in ins.values()) and np.isfinite(got).all()
    X = got.astype(f64).reshape(c.T, F, 2)
    r = (np.abs(X[:, :, 0] + 1j * X[:, :, 1] - ref).max(1) / delta).max()
    print("stft_tf %s: error / bound %.3f" % (R.case_id(c), r))
    assert r <= 1.0, r


# -------------------------------------------------------------------------------------------------------------- ns_istft
@pytest.mark.parametrize("c", R.ISTFT_CASES, ids=R.case_id)
def test_istft(dev, c):
    from nspeech_amd import _lib
    n_fft, hop, win = c.geom
    x = R.istft_inputs(c)
    ref, bound = R.istft_reference(c)
    ins = {k: In(v) for k, v in x.items()}
    out = Out(len(ref))
    work = Out(c.T * win, tail=GUARD, fill=float("nan"))
    p = _lib.struct("ns_istft_params")
    p.spec, p.T, p.center = ins["spec"].ptr, c.T, c.center
    _geometry(p, c.geom)
    p.window, p.twiddle, p.wav, p.work = ins["window"].ptr, ins["twiddle"].ptr, out.ptr, work.ptr
    got, frames = _twice("ns_istft", p, [out, work])
    assert out.intact() and work.intact() and all(i.unchanged() for i in ins.values())
    assert np.isfinite(got).all() and np.isfinite(frames).all()          # every windowed frame was written
    if len(ref) == 0:
        print("istft %s: no output" % R.case_id(c))
        return
    r = np.abs(got - ref).max() / np.abs(ref).max()
    print("istft %s: error %.3g of the peak, bound %.3g: %.3f" % (R.case_id(c), r, bound, r / bound))
    assert r <= bound, (r, bound)


# --------------------------------------------------------------------------------------------------------- ns_griffin_lim
@pytest.mark.parametrize("c", R.GL_CASES, ids=R.case_id)
def test_griffin_lim(dev, c):
    from nspeech_amd import _lib
    n_fft, hop, win = c.geom
    Lout = (c.T - 1) * hop + win
    x = R.gl_inputs(c)
    ref, bound = R.gl_reference(c), R.gl_bound(c)
    ins = {k: In(v, off=1 if (k == "window" and c.misalign) else 0) for k, v in x.items()}
    out = Out(c.N * Lout)
    p = _lib.struct("ns_griffin_lim_params")
    p.spec, p.N, p.T, p.iters = ins["spec"].ptr, c.N, c.T, c.iters
    _geometry(p, c.geom)
    p.power, p.ref_level_db, p.min_level_db = c.power, 20.0, c.min_db
    p.window, p.twiddle, p.wav = ins["window"].ptr, ins["twiddle"].ptr, out.ptr
    p.raw_magnitude, p.momentum = c.raw, c.momentum
    nbytes = _lib.lib().ns_griffin_lim_work_bytes
    nbytes.restype = C.c_size_t
    nb = nbytes(C.byref(p))
    assert nb == 4 * R.gl_work_floats(c.N, c.T, n_fft, win, c.momentum)
    work = Out(nb // 4, tail=GUARD, fill=float("nan"))
    p.work = work.ptr
    # the header's rule, on the addresses of this call, puts the case where the table says
    assert R.gl_form(n_fft, hop, win, ins["window"].ptr, work.ptr) == c.form
    got, = _twice("ns_griffin_lim", p, [out])
    assert out.intact() and work.intact() and all(i.unchanged() for i in ins.values()) and np.isfinite(got).all()
    got = got.reshape(c.N, Lout)
    r = max(np.abs(got[n] - ref[n]).max() / np.abs(ref[n]).max() for n in range(c.N))
    print("griffin_lim %s: error %.3g of the peak, bound %.3g: %.3f" % (R.case_id(c), r, bound, r / bound))
    assert r <= bound, (r, bound)


# ----------------------------------------------------------------------------------------------------- ns_audio_pointwise
def _pointwise_input(mode, n):
    rng = np.random.default_rng(10 * mode + n % 97)
    if mode == 0:                                 # amplitudes over eight decades, and what max(1e-5, x) floors: 0 and below
        x = np.where(rng.uniform(size=n) < 0.15, -rng.uniform(0, 1, n) * (rng.uniform(size=n) < 0.5), 10.0 ** rng.uniform(-7, 3, n))
    elif mode == 1:
        x = rng.uniform(-120, 20, n)
    elif mode == 2:
        x = rng.uniform(-150, 150, n)             # both clamps at min_level_db = +-100
    else:
        x = rng.uniform(-0.5, 1.5, n)
    return x.astype(f32)


@pytest.mark.parametrize("min_db", [-100.0, 100.0])
@pytest.mark.parametrize("n", R.POINTWISE_N)
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_pointwise(dev, mode, n, min_db):
    from nspeech_amd import _lib
    x = _pointwise_input(mode, n)
    xin, out = In(x), Out(n)
    p = _lib.struct("ns_audio_pointwise_params")
    p.x, p.y, p.n, p.mode, p.min_level_db = xin.ptr, out.ptr, n, mode, min_db
    got, = _twice("ns_audio_pointwise", p, [out])
    assert out.intact() and xin.unchanged() and np.isfinite(got).all()
    ref, tol = R.pointwise(x, mode, min_db), R.pointwise_tolerance(x, mode, min_db)
    if mode in (2, 3):                            # the inputs reach both clamps
        lo, hi = (0.0, 1.0) if mode == 2 else sorted((min_db, 0.0))
        assert n < 255 or ((ref == lo).any() and (ref == hi).any())
    r = (np.abs(got - ref) / tol).max()
    print("pointwise mode %d n %d min %+g: error / bound %.3f" % (mode, n, min_db, r))
    assert r <= 1.0, r


# --------------------------------------------------------------------------------------------------------- ns_preemphasis
def _preemph(x_ptr, y_ptr, n, coef, inverse, outs):
    from nspeech_amd import _lib
    p = _lib.struct("ns_preemphasis_params")
    p.x, p.y, p.n, p.coef, p.inverse = x_ptr, y_ptr, n, coef, inverse
    return _twice("ns_preemphasis", p, outs)


@pytest.mark.parametrize("coef", R.PREEMPH_COEFS)
@pytest.mark.parametrize("n", R.PREEMPH_N + (R.PREEMPH_N_LOOP,))
def test_preemphasis_forward(dev, n, coef):
    x = R.signal(n, 40 + n % 7)
    xin, out = In(x), Out(n)
    got, = _preemph(xin.ptr, out.ptr, n, coef, 0, [out])
    assert out.intact() and xin.unchanged()
    ref = R.preemphasis(x, coef)
    prev = np.concatenate([[0.0], np.abs(x[:-1].astype(f64))])
    tol = R.EPS * (np.abs(x.astype(f64)) + abs(float(f32(coef))) * prev)
    r = (np.abs(got - ref) / np.maximum(tol, 2.0 ** -149)).max()
    print("preemphasis forward n %d coef %g: error / bound %.3f" % (n, coef, r))
    assert r <= 1.0, r


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("coef", R.PREEMPH_COEFS)
@pytest.mark.parametrize("n", R.PREEMPH_N)
def test_preemphasis_inverse(dev, n, coef, in_place):
    from nspeech_amd import _lib, ops
    x = R.signal(n, 40 + n % 7)
    ref = R.inv_preemphasis(x, coef)
    bound = 4 * np.abs(R.inv_preemphasis_blocked_f32(x, coef) - ref).max()
    if in_place:                                  # y == x: one call (a second one would filter the result again)
        out = Out(n)
        out.buf[MARGIN:MARGIN + n] = torch.from_numpy(x.copy()).cuda()
        p = _lib.struct("ns_preemphasis_params")
        p.x, p.y, p.n, p.coef, p.inverse = out.ptr, out.ptr, n, coef, 1
        _lib.call("ns_preemphasis", p, ops.stream())
        got = out.get()
    else:
        xin, out = In(x), Out(n)
        got, = _preemph(xin.ptr, out.ptr, n, coef, 1, [out])
        assert xin.unchanged()
    assert out.intact() and np.isfinite(got).all()
    err = np.abs(got - ref).max()
    print("preemphasis inverse n %d coef %g%s: error %.3g, bound %.3g (peak %.3g)" % (n, coef, " in place" if in_place else "", err, bound, np.abs(ref).max()))
    assert err <= bound, (err, bound)


def test_in_place_inverse_is_the_out_of_place_one(dev):
    x = R.signal(4097, 3)
    xin, a, b = In(x), Out(4097), Out(4097)
    b.buf[MARGIN:MARGIN + 4097] = torch.from_numpy(x.copy()).cuda()
    _preemph(xin.ptr, a.ptr, 4097, 0.97, 1, [a])
    from nspeech_amd import _lib, ops
    p = _lib.struct("ns_preemphasis_params")
    p.x, p.y, p.n, p.coef, p.inverse = b.ptr, b.ptr, 4097, 0.97, 1
    _lib.call("ns_preemphasis", p, ops.stream())
    assert np.array_equal(a.get().view(np.uint32), b.get().view(np.uint32)) and b.intact()
