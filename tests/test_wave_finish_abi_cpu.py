"""ns_wave_finish (include/nspeech_hip.h) as the binding sees it, without a GPU: the symbol, the struct's fields, and the
argument checks, which come before any launch - a refused call and a call with nothing to do touch no device."""
import ctypes as C

import pytest

from nspeech_amd import _lib


def _params(**over):
    """A call that would be valid: the three pointers point into host buffers that a refused call never reads."""
    buf = (C.c_float * 16)()
    end = (C.c_int64 * 4)()
    p = _lib.struct("ns_wave_finish_params")
    p.x, p.y, p.end = C.addressof(buf), C.addressof(buf), C.addressof(end)
    p.N, p.L, p.ld, p.coef, p.window, p.hop, p.threshold = 2, 8, 8, 0.97, 4, 1, 0.01
    for k, v in over.items():
        setattr(p, k, v)
    p._keep = (buf, end)
    return p


def _call(p):
    return _lib.lib().ns_wave_finish(C.byref(p), C.c_void_p(0))


def test_symbol_and_struct():
    assert "ns_wave_finish" in _lib.FUNCS and hasattr(_lib.lib(), "ns_wave_finish")
    p = _lib.struct("ns_wave_finish_params")
    fields = p._fields_
    assert [f[0] for f in fields] == ["x", "y", "N", "L", "ld", "coef", "window", "hop", "threshold", "end"]
    types = dict(fields)
    assert types["x"] is C.c_void_p and types["y"] is C.c_void_p and types["end"] is C.c_void_p
    assert types["N"] is C.c_int and types["coef"] is C.c_float and types["threshold"] is C.c_double
    assert all(types[k] is C.c_int64 for k in ("L", "ld", "window", "hop"))


@pytest.mark.parametrize("bad", [dict(x=None), dict(y=None), dict(end=None), dict(N=-1), dict(L=-1), dict(ld=7),
                                 dict(window=0), dict(hop=0), dict(window=-3), dict(hop=-1)],
                         ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_bad_arguments_are_refused_with_a_message(bad):
    lib = _lib.lib()
    assert _call(_params(**bad)) == -1                       # NS_ERR_BAD_ARG
    assert lib.ns_last_error().decode().startswith("ns_wave_finish")
    with pytest.raises(_lib.NSError, match="ns_wave_finish"):
        _lib.call("ns_wave_finish", _params(**bad), 0)


def test_null_params_block_is_refused():
    assert _lib.lib().ns_wave_finish(None, C.c_void_p(0)) == -1


def test_no_rows_is_a_success_without_a_launch():
    assert _call(_params(N=0)) == 0
    assert _call(_params(N=0, L=0, ld=0)) == 0
