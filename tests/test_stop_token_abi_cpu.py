"""ns_stop_token and its work-size function are exported and declared, the parameter block follows the header, and the
host-side argument checks return -1 with a message before anything is launched (so they run without a GPU)."""
import ctypes
import os
import re

import pytest

from nspeech_amd import _lib

FAKE = 0x1000       # a non-null address that is never dereferenced: every case below fails its check on the host


def _params(**over):
    p = _lib.struct("ns_stop_token_params")
    base = dict(N=2, S=3, D=64, h=FAKE, h_dtype=_lib.NS_F32, h_sn=4 * 64, h_ss=64, w=FAKE, b=FAKE, logits=None,
                out_steps=None, pos_weight=1.0, grad_scale=1.0, dh=None, dh_sn=4 * 64, dh_ss=64, dw=None, db=None,
                acc=None, threshold_logit=0.0, stop_steps=None, work=None)
    base.update(over)
    for k, v in base.items():
        setattr(p, k, v)
    return p


def test_entry_points_are_exported_and_declared():
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"\bint\s+ns_stop_token\s*\(\s*const\s+ns_stop_token_params\s*\*", header)
    assert re.search(r"\bsize_t\s+ns_stop_token_work_floats\s*\(\s*int\s+N\s*,\s*int\s+S\s*,\s*int\s+D\s*\)", header)
    for name in ("ns_stop_token", "ns_stop_token_work_floats"):
        assert name in _lib.FUNCS
        assert hasattr(_lib.lib(), name)
    names = [f[0] for f in _lib.struct("ns_stop_token_params")._fields_]
    assert names == ["N", "S", "D", "h", "h_dtype", "h_sn", "h_ss", "w", "b", "logits", "out_steps", "pos_weight",
                     "grad_scale", "dh", "dh_sn", "dh_ss", "dw", "db", "acc", "threshold_logit", "stop_steps", "work"]
    assert os.path.exists(os.path.join(os.path.dirname(_lib.LIB_PATH), "stop_token.hip"))


def test_work_size_is_a_function_of_the_shape_only():
    fn = _lib.lib().ns_stop_token_work_floats
    fn.restype = ctypes.c_size_t
    # 32 rows per workgroup: G = ceil(N S / 32) partials of [D] + 2, the logits [N S], one word per utterance
    assert fn(3, 4, 64) == 1 * 64 + 2 + 12 + 3
    assert fn(32, 200, 1024) == 200 * 1024 + 400 + 6400 + 32
    assert fn(0, 4, 64) == 0


@pytest.mark.parametrize("over, word", [
    (dict(h=None), b"h is null"),
    (dict(w=None), b"w is null"),
    (dict(b=None), b"b is null"),
    (dict(D=96), b"D must"),
    (dict(D=0), b"D must"),
    (dict(D=4096), b"D must"),
    (dict(N=0), b"N must"),
    (dict(S=0), b"S must"),
    (dict(h_dtype=2), b"h_dtype"),
    (dict(h_ss=32), b"rows of h"),
    (dict(dh=FAKE), b"dh needs dw"),
    (dict(dh=FAKE, dw=FAKE), b"dh needs dw"),
    (dict(dw=FAKE, db=FAKE), b"need dh"),
    (dict(dh=FAKE, dw=FAKE, db=FAKE, dh_ss=8), b"rows of dh"),
    (dict(acc=FAKE, pos_weight=0.0), b"pos_weight"),
    (dict(out_steps=FAKE, grad_scale=-1.0), b"grad_scale"),
    (dict(stop_steps=FAKE, threshold_logit=float("nan")), b"threshold_logit"),
    (dict(stop_steps=FAKE), b"work is null"),
])
def test_bad_arguments_return_minus_one_with_a_message(over, word):
    lib = _lib.lib()
    rc = lib.ns_stop_token(ctypes.byref(_params(**over)), None)
    assert rc == -1
    msg = lib.ns_last_error()
    assert msg.startswith(b"ns_stop_token:") and word in msg, msg


def test_null_parameter_block():
    lib = _lib.lib()
    assert lib.ns_stop_token(None, None) == -1
    assert b"ns_stop_token" in lib.ns_last_error()
