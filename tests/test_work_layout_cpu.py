"""The sizes of the caller-owned work areas are ABI: callers allocate ns_*_work_bytes() once and tools find the trace
areas from the end.  These functions are pure host arithmetic (no GPU, no pointer is followed), so the values are pinned
exactly.  The numbers were read from a build of commit c99c68c (the last one with hand-written sums beside the pointer
chains; the layouts now come from one struct per kernel and launcher, csrc/carve.h) - per export the smallest supported
shape, the benchmark's, and one with a ragged batch."""
import ctypes as C

import pytest

from nspeech_amd import _lib

FAKE = 0x1000          # non-null, never followed


def _lstm(N, H, P=1, split=False):
    p = _lib.struct("ns_lstm_seq_params")
    p.N, p.H, p.P, p.T = N, H, P, P
    if split:
        p.h_bf16 = p.h_lo_bf16 = FAKE
    return p


def _gru(N, H):
    p = _lib.struct("ns_gru_seq_params")
    p.N, p.H, p.P, p.T = N, H, 1, 1
    return p


def _taco2(N, D1=256):
    p = _lib.struct("ns_taco2_attn_params")
    p.N, p.D1 = N, D1
    return p


def _taco1(N):
    p = _lib.struct("ns_taco1_attn_params")
    p.N = N
    return p


def _taco1_decode(N):
    q = _lib.struct("ns_taco1_decode_params")
    q.att.N = N
    return q


def _taco2_decode(N, D):
    q = _lib.struct("ns_taco2_decode_params")
    q.att.N, q.att.D1, q.D = N, 256, D
    return q


MAKERS = {
    "ns_lstm_cluster_work_bytes": _lstm, "ns_lstm_wide_work_bytes": _lstm, "ns_gru_seq_work_bytes": _gru,
    "ns_taco2_attn_cluster_work_bytes": _taco2, "ns_taco1_attn_cluster_work_bytes": _taco1,
    "ns_taco1_decode_work_bytes": _taco1_decode, "ns_taco2_decode_work_bytes": _taco2_decode,
}

# export -> [(arguments of its maker, bytes at commit c99c68c)]
CASES = {
    "ns_lstm_cluster_work_bytes": [(dict(N=1, H=64), 168192), (dict(N=32, H=256), 823552), (dict(N=17, H=128), 430336)],
    "ns_lstm_wide_work_bytes": [(dict(N=1, H=256, P=2), 147776), (dict(N=32, H=1024, P=200), 8405312), (dict(N=17, H=512, P=9), 1589568),
                                (dict(N=32, H=1024, P=200, split=True), 34619968), (dict(N=33, H=256, P=7, split=True), 908864)],
    "ns_gru_seq_work_bytes": [(dict(N=1, H=128), 1280), (dict(N=32, H=256), 394496), (dict(N=17, H=256), 394496)],
    "ns_taco2_attn_cluster_work_bytes": [(dict(N=1), 139776), (dict(N=32), 3449088), (dict(N=33), 3555840)],
    "ns_taco1_attn_cluster_work_bytes": [(dict(N=1), 65856), (dict(N=32), 2099456), (dict(N=17), 1115456)],
    "ns_taco1_decode_work_bytes": [(dict(N=1), 86400), (dict(N=32), 2756864), (dict(N=17), 1464704)],
    "ns_taco2_decode_work_bytes": [(dict(N=1, D=64), 146176), (dict(N=1, D=1024), 176896), (dict(N=2, D=1024), 320512), (dict(N=33, D=1024), 4772608)],
    "ns_wavenet_post_bytes": [(dict(B=1), 12544), (dict(B=32), 393472), (dict(B=17), 209152)],
}


def value(lib, name, kw):
    fn = getattr(lib, name)
    fn.restype = C.c_size_t
    if name == "ns_wavenet_post_bytes":
        return fn(C.c_int(kw["B"]))
    p = MAKERS[name](**kw)
    return fn(C.byref(p))


@pytest.mark.parametrize("name", sorted(CASES))
def test_work_bytes_are_the_abi_values(name):
    lib = _lib.lib()
    got = [(kw, value(lib, name, kw)) for kw, _ in CASES[name]]
    assert got == CASES[name]


def test_null_params_need_no_bytes():
    lib = _lib.lib()
    for name in MAKERS:
        fn = getattr(lib, name)
        fn.restype = C.c_size_t
        assert fn(None) == 0, name


CHAIN_L0 = 294


def test_chain_fits_turns_at_the_same_layer_counts():
    lib = _lib.lib()
    # shipped widths (R 32, S 512, Q 256), 60 KB of LDS: with the condition table the state of 73 layers fits and that of
    # 74 does not (as test_wavenet_cond_abi_cpu.py has it); without it the turn is between CHAIN_L0 and CHAIN_L0 + 1
    assert lib.ns_wavenet_chain_fits(73, 32, 512, 256, 1) == 1 and lib.ns_wavenet_chain_fits(74, 32, 512, 256, 1) == 0
    assert lib.ns_wavenet_chain_fits(CHAIN_L0, 32, 512, 256, 0) == 1 and lib.ns_wavenet_chain_fits(CHAIN_L0 + 1, 32, 512, 256, 0) == 0
    # narrower layers (R 16: the layout counts L * R floats) move it; nothing fits without layers
    assert lib.ns_wavenet_chain_fits(2 * CHAIN_L0, 16, 512, 256, 0) == 1 and lib.ns_wavenet_chain_fits(2 * CHAIN_L0 + 2, 16, 512, 256, 0) == 0
    assert lib.ns_wavenet_chain_fits(0, 32, 512, 256, 0) == 0
