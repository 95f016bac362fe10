"""ns_wavenet_gate's held-condition fields and ns_wavenet_hold_sum (include/nspeech_hip.h) as the binding sees them: the
fields are appended, so an all-zero tail is the call as it was.  No call is made: the entry points' own argument checks
are tests/test_wavenet_hold_gpu.py's, on real buffers."""
import ctypes

from nspeech_amd import _lib


def test_gate_fields_are_appended():
    p = _lib.struct("ns_wavenet_gate_params")
    names = [f[0] for f in p._fields_]
    assert names[-5:] == ["cond", "ld_cond", "cond_rows", "cond_hold", "cond_t0"] and names[-6] == "dz"
    fields = dict(p._fields_)
    assert fields["ld_cond"] is ctypes.c_int64 and fields["cond_rows"] is ctypes.c_int and fields["cond_hold"] is ctypes.c_int
    assert type(p).cond.offset > type(p).dz.offset
    assert "ns_wavenet_hold_sum" in _lib.FUNCS and hasattr(_lib.lib(), "ns_wavenet_hold_sum")
