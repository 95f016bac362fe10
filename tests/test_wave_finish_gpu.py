"""ns_wave_finish (csrc/audio.hip): inv_preemphasis and find_endpoint of N clips in one launch, one workgroup per row.

The filter is held to ns_preemphasis(inverse=1) bit for bit and to the float64 recursion of oracle/audio_oracle.py within
the bound tests/test_audio_gpu.py holds that kernel to.  The end of a row is held to find_endpoint's rule on the kernel's
OWN output row, exactly: oracle.audio_oracle.find_endpoint restated on the test's (window, hop, threshold) - the maximum
and not its absolute value, a strict comparison made in double, a NaN in a window makes it loud, the window at 0 is
never tested, window need not be a multiple of hop.

The NaN case: with coef = 0 the row is y[n] = x[n] + 0 * y[n-1], and 0 * NaN is NaN - the filter (this one, the one of
ns_preemphasis and scipy's lfilter alike) carries a NaN to the end of the row.  So the kernel's own row is NaN from
index hop + 3 on, no later window is silent, and the rule gives L; a table that assumes y == x there would say 3 * hop.
The case still tells the two implementations apart: a kernel whose fmaxf drops the NaN answers 2 * hop."""
import numpy as np
import pytest
import torch

from oracle import audio_oracle as AO

pytestmark = pytest.mark.gpu

THRESHOLD = 0.01


def _rule(y, window, hop, threshold=THRESHOLD):
    """oracle.audio_oracle.find_endpoint on (window, hop) given as they are; the comparison in double."""
    threshold = np.float64(threshold)
    for x in range(hop, len(y) - window, hop):
        if np.max(y[x:x + window]) < threshold:
            return x + hop
    return len(y)


def _run(dev, x, coef, window, hop, threshold=THRESHOLD, pad=0, inplace=False):
    """x float32 [N, L] -> (y [N, L], ends [N], the whole y buffer [N, L + pad], the whole x buffer afterwards)"""
    from nspeech_amd import ops
    N, L = x.shape
    ld = L + pad
    xb = np.full((N, ld), 7.0, np.float32)
    xb[:, :L] = x
    xd = torch.from_numpy(xb).to(dev)
    yd = xd if inplace else torch.full((N, ld), -3.0, dtype=torch.float32, device=dev)
    ends = torch.full((N,), -1, dtype=torch.int64, device=dev)
    ops.wave_finish(xd, yd, N, L, ld, coef, window, hop, threshold, ends)
    yb = yd.cpu().numpy()
    return yb[:, :L], ends.cpu().numpy(), yb, xd.cpu().numpy()


@pytest.fixture(scope="module")
def A(dev):
    from nspeech_amd import hparams
    from nspeech_amd.utils import audio
    hparams.load("taco2")
    assert float(hparams.get_hparams().preemphasis) == 0.97
    return audio


# ------------------------------------------------------------------ filter
# 8 samples per thread, 2048 per tile; 4097 = two full tiles and one sample
@pytest.mark.parametrize("L", [1, 7, 8, 9, 2047, 2048, 2049, 4097])
def test_filter_rows_equal_inv_preemphasis(dev, A, L):
    N, window, hop = 3, 16, 4
    x = (np.random.RandomState(L).randn(N, L) * 0.3).astype(np.float32)
    y, ends, yb, xb = _run(dev, x, 0.97, window, hop, pad=5)
    assert (yb[:, L:] == -3.0).all() and (xb[:, L:] == 7.0).all() and np.array_equal(xb[:, :L], x)
    for i in range(N):
        assert np.array_equal(y[i], A.inv_preemphasis(x[i])), i              # the same bits as ns_preemphasis
        ref = AO.inv_preemphasis(x[i], 0.97)
        err = np.abs(y[i] - ref).max()
        print("L=%d row %d: max error against float64 %.3e (bound %.3e)" % (L, i, err, 2e-4 * np.abs(ref).max()))
        assert err < 2e-4 * np.abs(ref).max()
        assert ends[i] == _rule(y[i], window, hop)
    y2, ends2, yb2, _ = _run(dev, x, 0.97, window, hop, pad=5, inplace=True)
    assert np.array_equal(y2, y) and np.array_equal(ends2, ends) and (yb2[:, L:] == 7.0).all()


# ------------------------------------------------------------------ endpoint semantics (coef = 0: y == x while x is finite)
def _cases(window, hop):
    """name -> (x [L], the end expected at hop = 4 from the issue's table or None, where it does not apply)"""
    one = np.ones(64, np.float32)
    c = {}
    for L in (1, window, window + hop):
        c["zeros L=%d" % L] = (np.zeros(L, np.float32), L)
    c["zeros L=window+hop+1"] = (np.zeros(window + hop + 1, np.float32), 2 * hop)
    a = one.copy(); a[:window] = 0
    c["only [0, window) silent"] = (a, 64)
    a = one.copy(); a[44:44 + window] = 0
    c["only the last admissible window silent"] = (a, 48)
    a = one.copy(); a[44:44 + window - 1] = 0
    c["the same, its last sample loud"] = (a, 64)
    c["float32(0.01): below the double 0.01"] = (np.full(64, np.float32(0.01)), 2 * hop)
    c["nextafter(float32(0.01), 1)"] = (np.full(64, np.nextafter(np.float32(0.01), np.float32(1))), 64)
    c["-5: max, not abs"] = (np.full(64, -5.0, np.float32), 2 * hop)
    a = np.zeros(64, np.float32); a[hop + 3] = np.nan
    c["a NaN at hop + 3"] = (a, 64)             # the filter carries the NaN to the end of the row: see the docstring
    return c


@pytest.mark.parametrize("window,hop", [(16, 4), (19, 4)])
def test_endpoint_semantics(dev, window, hop):
    assert 44 < 64 - window <= 44 + hop         # x = 44 is the last admissible window of a 64-sample row
    for name, (x, table) in _cases(window, hop).items():
        y, ends, _, _ = _run(dev, x[None], 0.0, window, hop)
        L = len(x)
        assert np.array_equal(y[0], x, equal_nan=True) or name.startswith("a NaN"), name
        want = _rule(y[0], window, hop)
        hp = {"sample_rate": window}            # the oracle itself: int(window * 1.0), int(window / 4), 10^(-40 / 20)
        assert int(window / 4) == hop and AO.find_endpoint(y[0], hp, -40, 1.0) == want, name
        print("window %d hop %d  %-42s L=%-3d end %d (rule %d)" % (window, hop, name, L, ends[0], want))
        assert want == table, name
        assert ends[0] == want, name
    # the NaN case on finite ground: the row behind a NaN is NaN, what a NaN-dropping maximum would call silent
    y, ends, _, _ = _run(dev, _cases(window, hop)["a NaN at hop + 3"][0][None], 0.0, window, hop)
    assert np.isnan(y[0, hop + 3:]).all() and not np.isnan(y[0, :hop + 3]).any() and ends[0] == 64


def test_window_across_the_tile_boundary(dev):
    window, hop, L = 1024, 256, 6000
    x = np.ones(L, np.float32)
    x[1792:2816] = 0                            # silent exactly in the window at 1792, which spans sample 2048
    assert _rule(x, window, hop) == 2048
    y, ends, _, _ = _run(dev, x[None], 0.0, window, hop)
    assert np.array_equal(y[0], x) and ends[0] == 2048


# ------------------------------------------------------------------ finish_waves at the shipped hparams
def test_finish_waves_agrees_with_the_single_clip_functions(dev, A):
    L = 50000
    rng = np.random.RandomState(0)
    x = np.zeros((3, L), np.float32)
    x[0, :20000] = rng.uniform(-0.1, 0.1, 20000)
    x[2] = rng.uniform(-0.1, 0.1, L)
    xd = torch.from_numpy(x).to(dev)
    y, ends = A.finish_waves(xd)
    assert y.is_cuda and ends.is_cuda and y.dtype == torch.float32 and ends.dtype == torch.int64
    assert y.shape == (3, L) and ends.shape == (3,) and torch.equal(xd.cpu(), torch.from_numpy(x))
    yh, eh = y.cpu().numpy(), ends.cpu().numpy()
    for i in range(3):
        assert np.array_equal(yh[i], A.inv_preemphasis(x[i])), i
        assert eh[i] == A.find_endpoint(yh[i]), (i, eh[i])
    print("ends", eh.tolist())
    assert 20000 <= eh[0] <= 28000 and eh[1] == 8000 and eh[2] == 50000
    # an array and a single clip take the same road
    y1, e1 = A.finish_waves(x[0])
    assert y1.shape == (1, L) and np.array_equal(y1.cpu().numpy()[0], yh[0]) and int(e1[0]) == eh[0]
