"""ns_guided_attention is exported, its parameter block follows the header, and its host-side argument checks return -1
with a message before anything is launched (so they run without a GPU, as tests/test_abi_cpu.py does for ns_gemm)."""
import ctypes

import pytest

from nspeech_amd import _lib

FAKE = 0x1000       # a non-null address that is never dereferenced: every case below fails its check on the host


def _params(**over):
    p = _lib.struct("ns_guided_attention_params")
    base = dict(N=2, S=3, Tia=8, in_lengths=FAKE, out_steps=None, sigma=0.4, align=FAKE, da0=None, grad_scale=1.0,
                row_out=FAKE, acc=None)
    base.update(over)
    for k, v in base.items():
        setattr(p, k, v)
    return p


def test_entry_point_is_exported_and_declared():
    assert "ns_guided_attention" in _lib.FUNCS
    assert hasattr(_lib.lib(), "ns_guided_attention")
    names = [f[0] for f in _lib.struct("ns_guided_attention_params")._fields_]
    assert names == ["N", "S", "Tia", "in_lengths", "out_steps", "sigma", "align", "da0", "grad_scale", "row_out", "acc"]


@pytest.mark.parametrize("over, word", [
    (dict(align=None), b"align"),
    (dict(in_lengths=None), b"in_lengths"),
    (dict(row_out=None), b"row_out"),
    (dict(sigma=0.0), b"sigma"),
    (dict(sigma=-0.4), b"sigma"),
    (dict(N=0), b"N must"),
    (dict(S=0), b"S must"),
    (dict(Tia=0), b"Tia must"),
])
def test_bad_arguments_return_minus_one_with_a_message(over, word):
    lib = _lib.lib()
    rc = lib.ns_guided_attention(ctypes.byref(_params(**over)), None)
    assert rc == -1
    msg = lib.ns_last_error()
    assert msg.startswith(b"ns_guided_attention:") and word in msg, msg


def test_null_parameter_block():
    lib = _lib.lib()
    assert lib.ns_guided_attention(None, None) == -1
    assert b"ns_guided_attention" in lib.ns_last_error()
