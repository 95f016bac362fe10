"""The C ABI of Tacotron-1's batched free-running synthesis loop: ns_taco1_decode_max_rows (the rows one launch of
ns_taco1_decode takes) is declared and exported and answers without a device, and the argument checks of
ns_taco1_decode_supported / ns_taco1_decode still reject null or zero-width parameters before any launch."""
import ctypes
import re

from nspeech_amd import _lib


def test_max_rows_is_declared_and_exported():
    src = open(_lib.HEADER_PATH).read()
    assert re.search(r"\bint\s+ns_taco1_decode_max_rows\s*\(\s*void\s*\)\s*;", src)
    assert "ns_taco1_decode_max_rows" in _lib.FUNCS
    assert hasattr(_lib.lib(), "ns_taco1_decode_max_rows")


def test_max_rows_is_a_positive_even_integer():
    fn = _lib.lib().ns_taco1_decode_max_rows
    fn.restype = ctypes.c_int
    fn.argtypes = []
    cap = fn()
    assert cap > 0 and cap % 2 == 0, cap
    assert fn() == cap


def test_bad_arguments_are_still_rejected():
    lib = _lib.lib()
    assert lib.ns_taco1_decode_supported(None) == 0
    assert lib.ns_taco1_decode(None, None, None) == -1
    assert b"ns_taco1_decode" in lib.ns_last_error()
    q = _lib.struct("ns_taco1_decode_params")          # all widths zero, null operands
    assert lib.ns_taco1_decode_supported(ctypes.byref(q)) == 0
    work = ctypes.create_string_buffer(4096)
    assert lib.ns_taco1_decode(ctypes.byref(q), None, None) == -1
    assert b"ns_taco1_decode" in lib.ns_last_error()
    assert lib.ns_taco1_decode(ctypes.byref(q), work, None) == -1
    assert b"ns_taco1_decode" in lib.ns_last_error()
    # the right widths and more than two rows, but null operands: N no longer decides, the operands still do
    q.att.N, q.att.S, q.att.Ti, q.att.Pi, q.att.Tia = 5, 4, 16, 16, 16
    q.att.A, q.att.E, q.att.D1, q.att.D2, q.D = 256, 256, 256, 128, 256
    assert lib.ns_taco1_decode_supported(ctypes.byref(q)) == 0
    assert lib.ns_taco1_decode(ctypes.byref(q), work, None) == -1
    assert b"ns_taco1_decode" in lib.ns_last_error()
