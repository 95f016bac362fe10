"""The host side of the WaveNet generator's sampling temperature: the identity the kernels rely on, the two fields of the
C struct, and how generate_wavenet.py routes --temperature with and without --incremental_temperature.  No device."""
import argparse
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


@pytest.mark.parametrize("T", [0.25, 0.7, 1.0, 2.0])
def test_scale_prediction_is_the_softmax_of_logits_over_t(T):
    """generate_wavenet.py:124-130 scales log(p); the kernels scale the exponent (lg - max) instead: the same
    distribution, softmax(lg / T), in float64."""
    from generate_wavenet import scale_prediction
    rng = np.random.RandomState(3)
    for Q in (64, 256):
        lg = rng.uniform(-40.0, 0.0, size=Q)
        hi, lo = rng.choice(Q, 2, replace=False)
        lg[hi], lg[lo] = 0.0, -40.0
        assert lg.max() - lg.min() == 40.0

        def softmax(x):
            e = np.exp(x - x.max())
            return e / e.sum()
        want = softmax(lg / T)
        got = scale_prediction(softmax(lg), T)
        # the kernels' own form: weights exp((lg - m) * (1 / T)), normalised by their sum
        w = np.exp((lg - lg.max()) * (1.0 / T))
        assert np.abs(got - want).max() < 1e-12 and np.abs(w / w.sum() - want).max() < 1e-12
        assert abs(got.sum() - 1.0) < 1e-12


def test_struct_carries_temperature_and_argmax_and_moves_no_member():
    """The two members fill the struct's two alignment gaps (behind w_dtype and behind engine), so cond_t0 stays the last
    member, as tests/test_wavenet_cond_abi_cpu.py pins it: the layout without them is the layout with them."""
    from nspeech_amd import _lib
    p = _lib.struct("ns_wavenet_generate_params")
    kinds = dict(p._fields_)
    assert kinds["temperature"] is ctypes.c_float and kinds["argmax"] is ctypes.c_int
    assert p.temperature == 0.0 and p.argmax == 0              # all-zero fields: the call as it was
    names = [f[0] for f in p._fields_]
    assert names[names.index("temperature") - 1] == "w_dtype" and names[names.index("argmax") - 1] == "engine"
    assert names[-1] == "cond_t0"
    T = type(p)
    assert T.temperature.offset == T.w_dtype.offset + 4 and T.argmax.offset == T.engine.offset + 4
    old = type("before", (ctypes.Structure,), {"_fields_": [f for f in p._fields_ if f[0] not in ("temperature", "argmax")]})
    assert ctypes.sizeof(old) == ctypes.sizeof(p)
    for n, _ in old._fields_:
        assert getattr(old, n).offset == getattr(T, n).offset, n


def _args(**over):
    a = dict(checkpoint="/nonexistent/model.ckpt-0", hparams="", gc_channels=None, lc_channels=None, local_condition=None, lc_hold=1,
             samples=4, fast_generation=True, temperature=1.0, precision="bf16", seed=0, wav_seed=None)
    a.update(over)
    return argparse.Namespace(**a)


def _no_model(monkeypatch):
    import generate_wavenet

    def refuse(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(generate_wavenet, "create_model", refuse)
    return generate_wavenet


def test_flag_without_fast_generation_is_refused_before_a_model_is_built(monkeypatch):
    gw = _no_model(monkeypatch)
    for T in (0.8, 1.0, 0.0):
        with pytest.raises(ValueError, match="--incremental_temperature"):
            gw.main(_args(incremental_temperature=True, fast_generation=False, temperature=T))


def test_namespace_without_the_flag_routes_as_before(monkeypatch, tmp_path):
    gw = _no_model(monkeypatch)
    cond = str(tmp_path / "lc.npy")
    np.save(cond, np.zeros((4, 4), np.float32))
    lc = dict(lc_channels=4, local_condition=cond)
    assert not hasattr(_args(), "incremental_temperature")
    for over in (dict(temperature=0.9), dict(fast_generation=False), dict(temperature=0.9, incremental_temperature=False)):
        with pytest.raises(ValueError, match="incremental generator only"):
            gw.main(_args(**dict(lc, **over)))
    # with the flag the same request passes the refusals and reaches the model
    with pytest.raises(AssertionError, match="a model was built"):
        gw.main(_args(incremental_temperature=True, temperature=0.9, **lc))
    with pytest.raises(AssertionError, match="a model was built"):
        gw.main(_args(incremental_temperature=True, temperature=0.0, **lc))
