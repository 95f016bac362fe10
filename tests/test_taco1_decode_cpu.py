"""The C ABI of Tacotron-1's free-running synthesis loop (ns_taco1_decode): declared, exported, and argument checks that
return errors on the host - no GPU needed."""
import ctypes
import re

from nspeech_amd import _lib

FUNCS = ("ns_taco1_decode_supported", "ns_taco1_decode_work_bytes", "ns_taco1_decode")


def test_header_declares_the_decode_entry_points():
    src = open(_lib.HEADER_PATH).read()
    assert re.search(r"\}\s*ns_taco1_decode_params\s*;", src)
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(const ns_taco1_decode_params\s*\*" % f, src), f


def test_library_exports_the_decode_entry_points():
    lib = _lib.lib()
    for f in FUNCS:
        assert f in _lib.FUNCS and hasattr(lib, f), f
    st = _lib.STRUCTS["ns_taco1_decode_params"]
    names = [n for n, _ in st._fields_]
    assert names[0] == "att" and "y2" in names and "wpf" in names and "bpf" in names


def test_bad_arguments_return_errors_not_crashes():
    lib = _lib.lib()
    assert lib.ns_taco1_decode_supported(None) == 0
    fn = lib.ns_taco1_decode_work_bytes
    fn.restype = ctypes.c_size_t
    assert fn(None) == 0
    assert lib.ns_taco1_decode(None, None, None) == -1
    q = _lib.struct("ns_taco1_decode_params")          # all widths zero, null operands
    assert lib.ns_taco1_decode_supported(ctypes.byref(q)) == 0
    assert lib.ns_taco1_decode(ctypes.byref(q), None, None) == -1
    work = ctypes.create_string_buffer(64)
    assert lib.ns_taco1_decode(ctypes.byref(q), work, None) == -1
    assert b"ns_taco1_decode" in lib.ns_last_error()
