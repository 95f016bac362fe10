"""ns_lstm_seq_params.h_lo_bf16 (include/nspeech_hip.h): the lo plane of the wide forward kernel's pre-split h.  The
member is appended, and the host refuses a lo plane without its hi plane before any launch - so this runs without a GPU
(the pointers below are never followed)."""
import ctypes

from nspeech_amd import _lib

ERR_ARG = -1


def test_struct_ends_with_the_lo_plane():
    p = _lib.struct("ns_lstm_seq_params")
    fields = dict((f[0], f[1]) for f in p._fields_)
    assert "h_lo_bf16" in fields and fields["h_lo_bf16"] is ctypes.c_void_p
    names = [f[0] for f in p._fields_]       # appended: every earlier member keeps its offset
    assert names[-1] == "h_lo_bf16" and names[-2] == "cell_clip"
    assert type(p).h_lo_bf16.offset > type(p).cell_clip.offset > type(p).h_bf16.offset


def test_lo_plane_without_hi_plane_is_refused():
    lib = _lib.lib()
    p = _lib.struct("ns_lstm_seq_params")
    fake = 0x1000                            # non-null; the call is refused before anything could read it
    p.dtype, p.f32_passes = _lib.NS_F32, 3
    p.N, p.T, p.H, p.P, p.padl = 4, 3, 256, 4, 1
    for f in ("xg", "whT_hi", "whT_lo", "h", "c", "gates", "h_lo_bf16"):
        setattr(p, f, fake)
    p.ld_xg, p.ld_h, p.ld_h_bf16 = 1024, 256, 256
    rc = lib.ns_lstm_wide_fwd(ctypes.byref(p), ctypes.c_void_p(fake), None)
    msg = lib.ns_last_error().decode()
    assert rc == ERR_ARG and "h_lo_bf16 without h_bf16" in msg, (rc, msg)
