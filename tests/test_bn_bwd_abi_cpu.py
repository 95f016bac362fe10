"""The argument checks of ns_bn_bwd that need no device: dpre_dtype is 0, or NS_BF16 with dtype NS_F32 - every other
combination is NS_ERR_BAD_ARG before anything is launched (a non-zero dpre_dtype beside bf16 z used to be ignored)."""
import ctypes

import pytest

from nspeech_amd import _lib as L

NS_F32, NS_BF16, NS_F64 = 0, 1, 2


def _block():
    p = L.struct("ns_bn_bwd_params")
    host = ctypes.create_string_buffer(256)            # addresses only: a refused call reads none of them
    at = ctypes.addressof(host)
    for k in ("dy", "z", "dpre", "mean", "istd", "gamma", "work"):
        setattr(p, k, at)
    p.rows, p.C, p.count = 4, 8, 4.0
    return p, host


@pytest.mark.parametrize("dtype,dpre_dtype", [(NS_BF16, NS_BF16), (NS_BF16, NS_F64), (NS_F32, NS_F64), (NS_F32, -1), (NS_F32, 7)])
def test_a_dpre_dtype_outside_the_documented_pair_is_refused(dtype, dpre_dtype):
    lib = L.lib()
    p, host = _block()
    p.dtype, p.dpre_dtype = dtype, dpre_dtype
    assert lib.ns_bn_bwd(ctypes.byref(p), None) == -1                  # NS_ERR_BAD_ARG
    msg = lib.ns_last_error()
    assert b"ns_bn_bwd" in msg and b"dpre_dtype" in msg, msg
    assert host.raw == bytes(256)
