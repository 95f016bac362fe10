"""The C ABI and host side of prenet dropout, without a device: the four drop_* fields at the end of both attention
parameter blocks as nspeech_amd.ops parses them from include/nspeech_hip.h, ns_dropout_rows declared and exported with
its argument checks, the shipped hparams (the option is there and off), and mask streams that collide neither with the
zoneout streams nor between two data-parallel ranks."""
import ctypes

import pytest

from nspeech_amd import _lib as L
from nspeech_amd import hparams as hparams_mod
from nspeech_amd import ops

FIELDS = [("drop_thr", ctypes.c_uint32), ("drop_seed1", ctypes.c_uint32), ("drop_seed2", ctypes.c_uint32), ("drop_scale", ctypes.c_float)]


@pytest.mark.parametrize("name", ["ns_taco2_attn_params", "ns_taco1_attn_params"])
def test_the_four_fields_end_both_attention_blocks(name):
    p = L.struct(name)
    assert list(p._fields_[-4:]) == FIELDS, p._fields_[-4:]
    for f, _ in FIELDS:
        assert getattr(p, f) == 0                    # a zero-initialised block: off
    q = (ops._attn_params if name == "ns_taco2_attn_params" else ops._taco1_attn_params)(
        dict(drop_thr=1 << 23, drop_seed1=0xFFFFFFFF, drop_seed2=7, drop_scale=2.0))
    assert (q.drop_thr, q.drop_seed1, q.drop_seed2, q.drop_scale) == (1 << 23, 0xFFFFFFFF, 7, 2.0)
    # the decode blocks embed them
    d = L.struct("ns_taco2_decode_params" if name == "ns_taco2_attn_params" else "ns_taco1_decode_params")
    assert d.att.drop_thr == 0


def test_dropout_rows_is_declared_exported_and_checks_its_arguments():
    assert "ns_dropout_rows" in L.FUNCS
    lib = L.lib()
    assert hasattr(lib, "ns_dropout_rows")
    p = L.struct("ns_dropout_rows_params")
    assert [f for f, _ in p._fields_] == ["dtype", "N", "T", "U", "sn", "st", "x", "y", "thr", "seed", "scale", "t0", "n0"]
    assert lib.ns_dropout_rows(None, None) == -1                       # NS_ERR_BAD_ARG
    assert lib.ns_dropout_rows(ctypes.byref(p), None) == -1            # null rows
    assert b"ns_dropout_rows" in lib.ns_last_error()


@pytest.mark.parametrize("model", ["taco2", "taco1"])
def test_the_option_ships_off(model):
    hp = hparams_mod.load(model)
    assert hp.prenet_dropout is False
    assert hp.drop_rate == 0.5
    hp.parse("prenet_dropout=true,drop_rate=0.3")
    assert hp.prenet_dropout is True and hp.drop_rate == 0.3


def test_mask_streams_are_their_own():
    ids = sorted(ops.DROPOUT_STREAMS.values())
    assert len(set(ids)) == 4 and not set(ids) & {2, 3, 4, 5}
    base = (5 * 2654435761 + 97) & 0xFFFFFFFF
    rank1 = base ^ ((1 * 0x9E3779B9) & 0xFFFFFFFF)
    for step in (0, 1, 1000):
        zone = {ops.zoneout_seed(base, step, i) for i in (2, 3, 4, 5)}
        mine = [ops.zoneout_seed(base, step, i) for i in ids]
        other = [ops.zoneout_seed(rank1, step, i) for i in ids]
        assert len(set(mine)) == 4 and not set(mine) & zone
        assert not set(mine) & set(other) and not set(other) & zone
    assert ops.zoneout_seed(base, 0, ids[0]) != ops.zoneout_seed(base, 1, ids[0])        # and every step its own
