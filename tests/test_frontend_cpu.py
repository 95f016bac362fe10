"""The utterance front end's C ABI without a GPU: ns_resample / ns_resample_out_len / ns_frame_power are exported, their
argument checks answer before any launch, and the order of the resampler's sum - the thing the kernel has to follow bit
for bit (tests/test_frontend_gpu.py) - is pinned by a scalar loop written here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from nspeech_amd import _lib

RATES = (8000, 16000, 20000, 22050, 44100, 48000)


def test_front_end_symbols_and_structs():
    lib = _lib.lib()
    for name in ("ns_resample", "ns_resample_out_len", "ns_frame_power"):
        assert name in _lib.FUNCS and hasattr(lib, name), name
    r = {f[0]: f[1] for f in _lib.struct("ns_resample_params")._fields_}
    assert list(r) == ["x", "x_dtype", "n_in", "y", "n_out", "sr_in", "sr_out", "win", "delta", "nwin", "num_table"]
    assert r["x"] is C.c_void_p and r["win"] is C.c_void_p and r["n_in"] is C.c_int64 and r["n_out"] is C.c_int64
    f = {f[0]: f[1] for f in _lib.struct("ns_frame_power_params")._fields_}
    assert list(f) == ["x", "n", "frame_length", "hop", "out", "n_frames"]
    assert f["n"] is C.c_int64 and f["n_frames"] is C.c_int64
    assert _lib.NS_F64 == 2


def test_resample_out_len_is_pythons_truncation():
    fn = _lib.lib().ns_resample_out_len
    fn.restype, fn.argtypes = C.c_int64, [C.c_int64, C.c_int, C.c_int]
    rng = np.random.default_rng(0)
    ns = [0, 1, 2, 3, 49, 50, 441, 16000, 20000, 22050, 48000, 10 ** 7] + [int(v) for v in rng.integers(0, 10 ** 7, size=300)]
    for a in RATES:
        for b in RATES:
            for n in ns:
                assert fn(n, a, b) == int(n * (float(b) / float(a))), (n, a, b)
    from nspeech_amd.utils import audio as A
    assert A.resample_out_len(2500, 22050, 20000) == 2267
    assert fn(10, 0, 20000) < 0 and fn(10, 20000, -1) < 0 and fn(-1, 20000, 20000) < 0


def _resample_params(n_in=100, sr_in=22050, sr_out=20000):
    p = _lib.struct("ns_resample_params")
    p.x, p.y, p.win, p.delta = 256, 512, 768, 1024          # non-null, never dereferenced: every case below fails first
    p.x_dtype, p.n_in, p.sr_in, p.sr_out = _lib.NS_F32, n_in, sr_in, sr_out
    p.n_out = int(n_in * (float(sr_out) / float(sr_in)))
    p.nwin, p.num_table = 32769, 512
    return p


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.lib()

    def refused(p, fn, word):
        rc = fn(C.byref(p), None) if p is not None else fn(None, None)
        msg = lib.ns_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    refused(None, lib.ns_resample, "null")
    for field in ("x", "y", "win", "delta"):
        p = _resample_params()
        setattr(p, field, None)
        refused(p, lib.ns_resample, "null pointer")
    for a, b in ((0, 20000), (22050, 0), (-22050, 20000)):
        refused(_bad_rates(a, b), lib.ns_resample, "rates must be positive")
    for wrong in (-1, 1):
        p = _resample_params()
        p.n_out += wrong
        refused(p, lib.ns_resample, "is not ns_resample_out_len")
    p = _resample_params()
    p.x_dtype = _lib.NS_BF16
    refused(p, lib.ns_resample, "x_dtype")
    # n_out == 0 succeeds without a launch (and without a GPU): nothing to compute, even with null buffers
    p = _resample_params(n_in=0)
    p.x = p.y = None
    assert p.n_out == 0 and lib.ns_resample(C.byref(p), None) == 0
    p = _resample_params(n_in=1, sr_in=48000, sr_out=20000)
    assert p.n_out == 0 and lib.ns_resample(C.byref(p), None) == 0

    q = _lib.struct("ns_frame_power_params")
    refused(None, lib.ns_frame_power, "null")
    refused(q, lib.ns_frame_power, "null")
    q.x, q.out, q.frame_length, q.hop = 256, 512, 1024, 512
    for n in (0, 1, 512):                                   # reflection by 512 needs more than 512 samples
        q.n, q.n_frames = n, 1 + n // 512
        refused(q, lib.ns_frame_power, "reflect")
    q.n, q.n_frames = 4000, 7                               # 1 + 4000 // 512 = 8
    refused(q, lib.ns_frame_power, "n_frames")
    q.n_frames, q.frame_length = 8, 1023
    refused(q, lib.ns_frame_power, "even")
    q.frame_length, q.hop = 1024, 0
    refused(q, lib.ns_frame_power, "hop")


def _bad_rates(a, b):
    p = _resample_params()
    p.sr_in, p.sr_out = a, b
    return p


def _scalar_resample(x, sr_orig, sr_new):
    """audio.resample as a per-sample float64 loop: the left wing's taps i = 0, 1, ... and then the right wing's into ONE
    accumulator, every tap w = win[k] + eta * delta[k]; acc = acc + w * x[..] with separately rounded operations (NumPy
    scalars never fuse) - the order ns_resample's kernel follows."""
    from nspeech_amd.utils import audio as A
    x = np.asarray(x, np.float64)
    ratio = float(sr_new) / float(sr_orig)
    n_out = int(x.shape[0] * ratio)
    win_np, num_table = A._kaiser_best()
    win = win_np * (ratio if ratio < 1 else 1.0)
    delta = np.zeros_like(win)
    delta[:-1] = win[1:] - win[:-1]
    scale = min(1.0, ratio)
    index_step = int(scale * num_table)
    inv = 1.0 / ratio
    nwin, n_orig = win.shape[0], x.shape[0]
    y = np.zeros(n_out, np.float64)
    for j in range(n_out):
        tr = np.float64(j) * inv
        n = int(tr)
        frac = np.float64(scale) * (tr - np.float64(n))
        acc = np.float64(0.0)
        for fr, count, sign, base in ((frac, n + 1, -1, n), (np.float64(scale) - frac, n_orig - n - 1, +1, n + 1)):
            idx = fr * np.float64(num_table)
            off = int(idx)
            eta = idx - np.float64(off)
            for i in range(min(count, (nwin - off) // index_step)):
                k = off + i * index_step
                w = win[k] + eta * delta[k]
                acc = acc + w * x[base + sign * i]
        y[j] = acc
    return y.astype(np.float32)


@pytest.mark.parametrize("sr_orig,n", [(22050, 2500), (48000, 4000), (16000, 2500), (44100, 2500)])
def test_reference_resampler_sums_in_the_scalar_loops_order(sr_orig, n):
    from nspeech_amd.utils import audio as A
    rng = np.random.default_rng(sr_orig)
    x = (0.3 * rng.standard_normal(n)).astype(np.float32)
    got = A._resample_reference(x, sr_orig, 20000, device="cpu")
    want = _scalar_resample(x, sr_orig, 20000)
    assert got.dtype == np.float32 and got.shape == (int(n * (20000.0 / sr_orig)),)
    assert np.array_equal(got, want)


def test_resample_kernel_has_no_fused_multiply_add():
    """ns_resample's taps are four separately rounded float64 operations; hipcc contracts a * b + c by default.  The
    kernel's assembly, compiled with the flags build.sh gives the file, holds v_mul_f64 / v_add_f64 and not one fma."""
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(os.path.dirname(here), "nspeech_amd", "csrc")
    sh = open(os.path.join(csrc, "build.sh")).read()
    base = re.search(r'^FLAGS="([^"]*)"', sh, flags=re.M).group(1).split()
    extra = re.search(r'frontend\.hip\)\s*echo "([^"]*)"', sh).group(1).split()
    assert "-ffp-contract=off" in extra
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    asm = subprocess.run([hipcc] + base + extra + ["-S", "--cuda-device-only", os.path.join(csrc, "frontend.hip"), "-o", "-"],
                         check=True, capture_output=True, text=True).stdout
    bodies = re.findall(r"^(_Z\d+resample_kernel\w*):[^\n]*\n(.*?)^\.Lfunc_end", asm, flags=re.S | re.M)
    assert len(bodies) == 2, [b[0] for b in bodies]         # float32 and float64 input
    for name, body in bodies:
        assert "v_mul_f64" in body and "v_add_f64" in body, name
        fused = re.findall(r"\bv_(?:fma|fmac|mad|mac)\w*_f(?:64|32)\w*", body)
        assert not fused, (name, fused)
