"""tests/audio_ref.py must not be wrong the way a kernel is.  No GPU.

The reference against independent formulations (scipy.signal.lfilter for both filters, a direct O(N^2) DFT over frames
indexed one sample at a time at n_fft 64, the oracle's librosa / TF restatements at every geometry, np.fft.irfft for
the DC / Nyquist rule, tests/griffin_lim_ref.py); ten planted errors, each beyond the bound of every case of
tests/test_audio_contract_gpu.py meant to catch it and inside the bound of a case that is not; the conditions that keep
a bound from hiding a failure, asserted for every case the GPU module runs; and the C ABI of the six parameter blocks
with the refusals the launchers document, through the loaded library and before any launch."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.signal

import audio_ref as R
import griffin_lim_ref as GR
from oracle import audio_oracle as AO

f32, f64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------- independent formulations
@pytest.mark.parametrize("coef", R.PREEMPH_COEFS)
def test_filters_against_lfilter(coef):
    c = float(f32(coef))
    for n in (1, 9, 2049):
        x = R.signal(n, 3)
        fwd, inv = scipy.signal.lfilter([1.0, -c], [1.0], x.astype(f64)), scipy.signal.lfilter([1.0], [1.0, -c], x.astype(f64))
        assert np.abs(R.preemphasis(x, coef) - fwd).max() <= 1e-15
        assert np.abs(R.inv_preemphasis(x, coef) - inv).max() <= 1e-12 * max(1.0, np.abs(inv).max())
        emu = R.inv_preemphasis_blocked_f32(x, coef)
        assert np.abs(emu - inv).max() <= 1e-5 * max(1.0, np.abs(inv).max())          # float32, not wrong
        assert coef != 0.0 or np.array_equal(emu, x)


def _dft_frames(frames, n_fft):
    k = np.arange(n_fft // 2 + 1)
    return frames @ np.exp(-2j * np.pi * np.outer(np.arange(n_fft), k) / n_fft)


@pytest.mark.parametrize("geom", [(64, 16, 64), (64, 7, 24)])
def test_transforms_against_a_direct_dft_with_scalar_framing(geom):
    n_fft, hop, win = geom
    w = R.window_table(win).astype(f64)
    for L in R.spec_lengths(n_fft, hop):
        y = R.signal(L, 5).astype(f64)
        c = float(f32(0.97))
        T = 1 + L // hop
        fr = np.zeros((T, n_fft))
        for t in range(T):
            for j in range(n_fft):
                wj = j - (n_fft - win) // 2
                if 0 <= wj < win:
                    i = t * hop + j - n_fft // 2
                    i = -i if i < 0 else i
                    i = 2 * (L - 1) - i if i >= L else i
                    assert 0 <= i < L
                    fr[t, j] = (y[i] - (c * y[i - 1] if i > 0 else 0.0)) * w[wj]
        got = R.stft_center(y, n_fft, hop, win, w, 0.97)
        assert got.shape == (T, n_fft // 2 + 1) and np.abs(got - _dft_frames(fr, n_fft)).max() <= 1e-12
    y = R.signal(5 * hop + win + 3, 6).astype(f64)
    fr = np.zeros((6, n_fft))
    for t in range(6):
        fr[t, :win] = y[t * hop:t * hop + win] * w
    S = R.tf_stft(y, n_fft, hop, win, w)
    assert S.shape == (6, n_fft // 2 + 1) and np.abs(S - _dft_frames(fr, n_fft)).max() <= 1e-12
    # the inverse: the Hermitian sum one bin at a time
    n = np.arange(n_fft)
    full = np.concatenate([S, np.conj(S[:, -2:0:-1])], 1)
    inv = (full @ np.exp(2j * np.pi * np.outer(np.arange(n_fft), n) / n_fft)).real / n_fft
    assert np.abs(R.inverse_frames(S, n_fft) - inv).max() <= 1e-12
    want = np.zeros(5 * hop + win)
    for t in range(6):
        want[t * hop:t * hop + win] += inv[t, :win] * w
    assert np.abs(R.tf_istft(S, n_fft, hop, win, w) - want).max() <= 1e-12


@pytest.mark.parametrize("geom", [g for g, _ in R.GEOMETRIES], ids=lambda g: "%d-%d-%d" % g)
def test_transforms_against_the_oracle(geom):
    """The oracle builds its own float64 window; the float32 table moves a result by a few 1e-8."""
    n_fft, hop, win = geom
    w = R.window_table(win)
    y = R.signal(max(6 * hop + 1, n_fft // 2 + 1), 8)
    a, b = R.stft_center(y, n_fft, hop, win, w, 0.97), AO.librosa_stft(AO.preemphasis(y, float(f32(0.97))), n_fft, hop, win).T
    assert a.shape == b.shape and np.abs(a - b).max() <= 1e-6 * np.abs(b).max()
    assert np.abs(R.istft_center(b, n_fft, hop, win, w) - AO.librosa_istft(b.T, n_fft, hop, win)).max() <= 1e-6 * max(1.0, np.abs(y).max())
    y = R.signal(5 * hop + win, 9)
    a, b = R.tf_stft(y, n_fft, hop, win, w), AO.tf_stft(y, n_fft, hop, win)
    assert a.shape == b.shape and np.abs(a - b).max() <= 1e-6 * np.abs(b).max()
    assert np.abs(R.tf_istft(b, n_fft, hop, win, w) - AO.tf_istft(b, n_fft, hop, win)).max() <= 1e-6
    S = np.abs(b)[None]
    for iters, a in ((0, 0.0), (2, 0.0), (3, 0.99)):
        got = R.griffin_lim(S, n_fft, hop, win, w, iters, a)[0]
        want = GR.griffin_lim(S[0], n_fft, hop, win, iters, float(f32(a)))
        assert np.abs(got - want).max() <= 2e-5 * np.abs(want).max(), (iters, a)      # (the phase step amplifies the table's 6e-8)


def test_dc_and_nyquist_rule_is_irfft():
    rng = np.random.default_rng(0)
    S = rng.normal(size=(3, 33)) + 1j * rng.normal(size=(3, 33))
    Z = S.copy()
    Z[:, 0], Z[:, -1] = Z[:, 0].real, Z[:, -1].real
    assert np.abs(R.inverse_frames(S, 64) - np.fft.irfft(S, n=64, axis=1)).max() <= 1e-15
    assert np.abs(R.inverse_frames(S, 64) - np.fft.irfft(Z, n=64, axis=1)).max() <= 1e-15
    assert np.abs(R.inverse_frames(S, 64, plant="dc_nyquist_kept") - R.inverse_frames(S, 64)).max() > 1e-3
    assert np.array_equal(R.inverse_frames(Z, 64, plant="dc_nyquist_kept"), R.inverse_frames(Z, 64))


def test_pointwise_and_magnitudes_against_the_oracle():
    x = np.linspace(-0.5, 1.5, 41).astype(f32)
    for mn in (-100.0, 100.0):
        hp = dict(min_level_db=mn)
        assert np.array_equal(R.pointwise(x * f32(100), 2, mn), AO.normalize((x * f32(100)).astype(f64), hp))
        assert np.array_equal(R.pointwise(x, 3, mn), AO.denormalize(x.astype(f64), hp))
        S = np.power(np.power(10.0, (AO.denormalize(x.astype(f64), hp) + 20.0) * 0.05), 1.5)
        assert np.allclose(R.gl_magnitude(x, 0, 1.5, 20.0, mn), S, rtol=1e-14)
    assert np.allclose(R.pointwise(np.abs(x), 0, -100.0), AO.amp_to_db(np.abs(x).astype(f64)), rtol=1e-6, atol=1e-5)     # (1e-5 as a float32)
    assert np.array_equal(R.gl_magnitude(x, 1, 1.5, 20.0, -100.0), x.astype(f64))
    assert np.array_equal(R.feature(np.abs(x).astype(f64), 20.0, -100.0), R.pointwise(R.pointwise(np.abs(x), 0, 0) - 20.0, 2, -100.0))


def test_tables():
    for n in (6, 27, 1000):
        assert np.array_equal(R.window_table(n), AO.hann_periodic(n).astype(f32)) and R.window_table(n)[0] == 0.0
    tw = R.twiddle_table(64)
    assert tw.shape == (32, 2) and tw.dtype == f32 and tuple(tw[0]) == (1.0, 0.0) and tw[16, 1] == -1.0
    assert np.abs(tw[:, 0] + 1j * tw[:, 1] - np.exp(-2j * np.pi * np.arange(32) / 64)).max() <= 2.0 ** -24


# ------------------------------------------------------------------------------------------------------- planted errors
def _spec_ratio(c, plant):
    """The planted transform's distance from the reference over the frame's delta, worst frame."""
    n_fft, hop, win = c.geom
    x = R.spec_inputs(c)
    ref, b = R.spec_reference(c)
    X = R.stft_center(x["wav"], n_fft, hop, win, x["window"], c.preemph, plant=plant)
    return float((np.abs(X - ref["stft"]).max(1) / b["delta"]).max())


def _stft_tf_ratio(c, plant):
    """ns_stft_tf pads by 0 samples, whatever the mode: the plant of the feature kernel's padding leaves it alone."""
    n_fft, hop, win = c.geom
    x = R.stft_tf_inputs(c)
    ref, delta = R.stft_tf_reference(c)
    y = np.pad(x["wav"], 0, mode="edge" if plant == "edge_pad" else "reflect")
    return float((np.abs(R.tf_stft(y, n_fft, hop, win, x["window"], T=c.T) - ref).max(1) / delta).max())


def _istft_ratio(c, plant):
    ref, bound = R.istft_reference(c)
    if ref.size == 0:
        return 0.0
    return float(np.abs(R.istft_reference(c, plant)[0] - ref).max() / np.abs(ref).max() / bound)


def _gl_ratio(c, plant):
    ref, bad, bound = R.gl_reference(c), R.gl_reference(c, plant), R.gl_bound(c)
    return float(max(np.abs(bad[n] - ref[n]).max() / np.abs(ref[n]).max() for n in range(c.N)) / bound)


def _covers4(c):
    return c.geom[2] > 3 * c.geom[1] and c.T >= 4


FAMILIES = {"spec": (R.SPEC_CASES, _spec_ratio), "stft_tf": (R.STFT_TF_CASES, _stft_tf_ratio),
            "istft": (R.ISTFT_CASES, _istft_ratio), "gl": (R.GL_CASES, _gl_ratio)}
#   plant: (families it is evaluated on, the cases meant to catch it)
PLANTED = {
    "edge_pad": (("spec", "stft_tf"), lambda c: isinstance(c, R.SpecCase)),
    "preemph_neighbour": (("spec",), lambda c: c.preemph != 0),
    "window_at_start": (("spec",), lambda c: c.geom[2] < c.geom[0]),
    "drop_fourth": (("istft", "gl"), _covers4),
    "next_clip": (("gl",), lambda c: c.N > 1 and c.geom[2] > c.geom[1]),
    "norm_by_window": (("istft",), lambda c: c.center == 1 and c.T >= 2),
    "dc_nyquist_kept": (("istft",), lambda c: c.source != "stft" and not (c.center == 1 and c.T == 1)),
    "swap_bins": (("gl",), lambda c: c.iters >= 1),
    "no_momentum": (("gl",), R.is_momentum_case),
    "gt_zero": (("istft",), lambda c: c.source == "tiny_window"),
}


def test_every_plant_is_listed():
    assert set(PLANTED) == set(R.PLANTS) and len(PLANTED) >= 8


@pytest.mark.parametrize("plant", sorted(PLANTED))
def test_planted_error_is_caught_where_meant_and_missed_elsewhere(plant):
    families, meant = PLANTED[plant]
    caught, missed, worst_miss = 0, 0, 0.0
    least = math.inf
    for fam in families:
        cases, ratio = FAMILIES[fam]
        for c in cases:
            r = ratio(c, plant)
            if meant(c):
                assert r > 1.0, (plant, R.case_id(c), r)
                caught, least = caught + 1, min(least, r)
            elif r <= 1.0:
                missed, worst_miss = missed + 1, max(worst_miss, r)
    print("%s: beyond the bound at all %d cases meant for it (the least %.3g x), inside it at %d others (%.3g x at the most)"
          % (plant, caught, least, missed, worst_miss))
    assert caught >= 1 and missed >= 1


# ------------------------------------------------------------------- the conditions, for every case the GPU module runs
@pytest.mark.parametrize("c", R.SPEC_CASES, ids=R.case_id)
def test_feature_intervals_are_narrow(c):
    """At most 5 % of a case's elements may have an interval wider than 2e-4 and at most 1 % one wider than 1e-3; the
    transform's delta is never looser than the 2e-4 of the peak the suite already holds it to; a clamp case shows its
    clamp."""
    ref, b = R.spec_reference(c)
    T, F = 1 + c.L // c.geom[1], c.geom[0] // 2 + 1
    assert ref["stft"].shape == (T, F) and ref["mel"].shape == (T, c.n_mels) and T <= 11
    assert (b["delta"] <= 2e-4 * np.abs(ref["stft"]).max()).all()
    for k in ("lin", "mel"):
        lo, hi = b[k]
        assert ((lo <= ref[k]) & (ref[k] <= hi)).all()
        wide = hi - lo
        s1, s2 = float((wide > 2e-4).mean()), float((wide > 1e-3).mean())
        print("%s %s: %.2f %% of the intervals wider than 2e-4, %.2f %% wider than 1e-3" % (R.case_id(c), k, 100 * s1, 100 * s2))
        assert s1 <= 0.05 and s2 <= 0.01, (k, s1, s2)
    clamp = R.QUIET_CASES.get(c.seed)
    if clamp:
        share = float((ref["lin"] == (0.0 if clamp == "lower" else 1.0)).mean())
        print("%s: %.1f %% of lin on the %s clamp" % (R.case_id(c), 100 * share, clamp))
        assert 0.05 <= share <= 0.95


@pytest.mark.parametrize("c", R.STFT_TF_CASES, ids=R.case_id)
def test_stft_tf_cases(c):
    n_fft, hop, win = c.geom
    ref, delta = R.stft_tf_reference(c)
    L = len(R.stft_tf_inputs(c)["wav"])
    assert ref.shape == (c.T, n_fft // 2 + 1) and (c.T - 1) * hop + win <= L < (c.T - 1) * hop + win + hop
    assert (delta <= 2e-4 * np.abs(ref).max()).all()


@pytest.mark.parametrize("c", R.ISTFT_CASES, ids=R.case_id)
def test_istft_cases(c):
    n_fft, hop, win = c.geom
    x = R.istft_inputs(c)
    ref, bound = R.istft_reference(c)
    assert ref.shape == ((c.T - 1) * hop + (0 if c.center else win),) and bound <= R.ISTFT_PROJECT_BOUND
    if c.source != "stft":
        assert (np.abs(x["spec"][:, [0, -1]].imag) > 1e-3).all()
    else:
        assert (x["spec"][:, [0, -1]].imag == 0).all()
    if c.center and hop == win and c.T > 1:       # the window sum is under FLT_MIN at every frame edge, and not 0 at one
        w = x["window"].astype(f64)
        assert (w[0] * w[0] <= R.FLT_MIN) and np.isfinite(ref).all()
    print("%s: bound %.3g of the peak" % (R.case_id(c), bound))


@pytest.mark.parametrize("c", R.GL_CASES, ids=R.case_id)
def test_griffin_lim_cases(c):
    n_fft, hop, win = c.geom
    ref, bound = R.gl_reference(c), R.gl_bound(c)
    assert ref.shape == (c.N, (c.T - 1) * hop + win) and np.isfinite(ref).all() and bound <= R.gl_project_bound(c.iters)
    peaks = np.abs(ref).max(1)
    assert (peaks > 0).all()
    # the selection rule of the header puts the case where the table says (an address of 4: four bytes off an 8-byte boundary)
    assert R.gl_form(n_fft, hop, win, 4 if c.misalign else 0, 0) == c.form
    assert R.gl_work_floats(c.N, c.T, n_fft, win, c.momentum) * 4 == _work_bytes(c)
    # rounding the state to float32 moves the reference by at most a tenth of the bound
    drift = max(np.abs(R.gl_reference(c, float32_state=True)[n] - ref[n]).max() / peaks[n] for n in range(c.N))
    print("%s: bound %.3g, float32-state drift %.3g of the peak" % (R.case_id(c), bound, drift))
    assert drift <= bound / 10
    if c.N > 1:                                   # three different clips
        assert not np.array_equal(ref[0], ref[1]) and not np.array_equal(ref[1], ref[2])
    if R.is_momentum_case(c):                     # a kernel that ignores momentum is further away than twice the bound
        plain = R.gl_reference(c, momentum=0.0)
        away = min(np.abs(plain[n] - ref[n]).max() / peaks[n] for n in range(c.N))
        print("    the plain result lies %.3g of the peak away" % away)
        assert away > 2 * bound, (away, bound)


def test_generic_form_runs_both_parities_with_iterations():
    par = {int(math.log2(c.geom[0] // 2)) % 2 for c in R.GL_CASES if c.form == "generic" and c.iters >= 1}
    assert par == {0, 1}
    assert {c.form for c in R.GL_CASES if not c.raw} == {"wave", "generic"}
    both = [c for c in R.GL_CASES if c.geom == (2048, 250, 1000) and c.raw]
    assert {(c.T, c.N, c.iters, c.momentum) for c in both if c.form == "wave"} == {(c.T, c.N, c.iters, c.momentum) for c in both if c.form == "generic"}
    for a, b in zip([c for c in both if c.form == "wave"], [c for c in both if c.form == "generic"]):
        assert np.array_equal(R.gl_inputs(a)["spec"], R.gl_inputs(b)["spec"])           # the same input, one reference


def test_pointwise_and_filter_tolerances_are_tight():
    x = np.linspace(-120, 20, 57).astype(f32)
    assert (R.pointwise_tolerance(x, 1, -100.0) / R.pointwise(x, 1, -100.0)).max() < 1e-5            # test_audio_gpu.py: 1e-5
    assert R.pointwise_tolerance(np.linspace(-150, 150, 61).astype(f32), 2, 100.0).max() < 1e-6     # 1e-6
    assert R.pointwise_tolerance(np.linspace(-0.5, 1.5, 41).astype(f32), 3, 100.0).max() < 1e-4     # 1e-4
    assert R.pointwise_tolerance(np.linspace(1e-6, 1e3, 99).astype(f32), 0, 0.0).max() < 2e-4       # 2e-4
    for coef in R.PREEMPH_COEFS:
        for n in R.PREEMPH_N:
            xs = R.signal(n, 40 + n % 7)
            ref = R.inv_preemphasis(xs, coef)
            d = 4 * np.abs(R.inv_preemphasis_blocked_f32(xs, coef) - ref).max()
            assert d <= 2e-4 * np.abs(ref).max()                                                   # 2e-4 of the peak


# ------------------------------------------------------------------------------------- the C ABI, through the library
BLOCKS = {
    "ns_spectrogram_params": ["wav", "L", "preemph", "n_fft", "hop", "win", "T", "window", "twiddle", "mel_basis", "n_mels",
                              "ref_level_db", "min_level_db", "lin_out", "mel_out", "stft_out"],
    "ns_griffin_lim_params": ["spec", "N", "T", "n_fft", "hop", "win", "iters", "power", "ref_level_db", "min_level_db", "window",
                              "twiddle", "wav", "work", "raw_magnitude", "momentum"],
    "ns_stft_tf_params": ["wav", "L", "n_fft", "hop", "win", "T", "window", "twiddle", "out"],
    "ns_istft_params": ["spec", "T", "n_fft", "hop", "win", "center", "window", "twiddle", "wav", "work"],
    "ns_audio_pointwise_params": ["x", "y", "n", "mode", "min_level_db"],
    "ns_preemphasis_params": ["x", "y", "n", "coef", "inverse"],
}


@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_parameter_block_fields(name):
    from nspeech_amd import _lib
    p = _lib.struct(name)
    assert [f[0] for f in p._fields_] == BLOCKS[name]
    kinds = dict(p._fields_)
    assert kinds["n"] is C.c_int64 if "n" in kinds else True
    for f in ("n_fft", "hop", "win", "T", "L", "N", "center", "iters", "mode", "inverse", "raw_magnitude", "n_mels"):
        assert kinds.get(f, C.c_int) is C.c_int, f


def _block(name, **over):
    """A call that would be valid at (2048, 250, 1000); the pointers are host memory that a refused call never reads."""
    from nspeech_amd import _lib
    buf = (C.c_float * 16)()
    p = _lib.struct(name)
    for f, kind in p._fields_:
        if kind is C.c_void_p:
            setattr(p, f, C.addressof(buf))
    vals = dict(n_fft=2048, hop=250, win=1000, T=5, N=1, L=2000, iters=1, n_mels=4, power=1.0, min_level_db=-100.0, raw_magnitude=1)
    for f, v in dict(vals, **over).items():
        if f in dict(p._fields_):
            setattr(p, f, v)
    p._keep = buf
    return p


def _work_bytes(c):
    from nspeech_amd import _lib
    fn = _lib.lib().ns_griffin_lim_work_bytes
    fn.restype = C.c_size_t
    return fn(C.byref(_block("ns_griffin_lim_params", n_fft=c.geom[0], hop=c.geom[1], win=c.geom[2], N=c.N, T=c.T, momentum=c.momentum)))


def _rc(entry, p):
    from nspeech_amd import _lib
    return getattr(_lib.lib(), entry)(C.byref(p), C.c_void_p(0))


TRANSFORMS = ["ns_spectrogram", "ns_griffin_lim", "ns_stft_tf", "ns_istft"]


@pytest.mark.parametrize("entry", TRANSFORMS)
def test_documented_refusals(entry):
    from nspeech_amd import _lib
    blk = entry + "_params"
    for n_fft in (32, 8192, 96, 1000, 0, -2048):
        assert _rc(entry, _block(blk, n_fft=n_fft, hop=4, win=16, L=9000)) == -1, n_fft
        assert _lib.lib().ns_last_error().decode().startswith(entry)
    assert _rc(entry, _block(blk, win=2049, hop=250, L=9000)) == -1                     # win > n_fft
    if entry in ("ns_griffin_lim", "ns_istft"):
        assert _rc(entry, _block(blk, hop=1001)) == -1                                  # hop > win
        assert _rc(entry, _block(blk, hop=0)) == -1
    if entry == "ns_spectrogram":
        assert _rc(entry, _block(blk, L=1024)) == -1                                    # L <= n_fft / 2
        assert _rc(entry, _block(blk, L=1025, T=0)) == 0
    if entry == "ns_stft_tf":
        assert _rc(entry, _block(blk, L=1999, T=5)) == -1                               # the last frame ends at 2000
        assert _rc(entry, _block(blk, L=2000, T=0)) == 0
        assert _rc(entry, _block(blk, L=2000, T=-1)) == -1                              # (the one entry that refuses T < 0)
        assert _rc(entry, _block(blk, hop=0)) == -1
    with pytest.raises(_lib.NSError, match=entry):
        _lib.call(entry, _block(blk, n_fft=96), 0)


@pytest.mark.parametrize("entry,over", [("ns_spectrogram", dict(T=0)), ("ns_spectrogram", dict(T=-1)), ("ns_griffin_lim", dict(T=0)),
                                        ("ns_griffin_lim", dict(N=0)), ("ns_griffin_lim", dict(N=-3)), ("ns_stft_tf", dict(T=0)),
                                        ("ns_istft", dict(T=0)), ("ns_istft", dict(T=-1)), ("ns_audio_pointwise", dict(n=0)),
                                        ("ns_preemphasis", dict(n=0)), ("ns_preemphasis", dict(n=-5, inverse=1))])
def test_nothing_to_do_is_a_success_without_a_launch(entry, over):
    """(A launch would read the host pointers of _block() on a machine with a GPU, and fail on one without.)"""
    assert _rc(entry, _block(entry + "_params", **over)) == 0


def test_pointwise_refuses_an_unknown_mode():
    assert _rc("ns_audio_pointwise", _block("ns_audio_pointwise_params", n=4, mode=4)) == -1
    assert _rc("ns_audio_pointwise", _block("ns_audio_pointwise_params", n=4, mode=-1)) == -1
