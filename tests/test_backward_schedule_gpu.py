"""Where the backward pass runs its optimiser-only work must not change a bit of the result: the weight gradients, the
BatchNorm-backward finalisers and the bf16 operand copies that ride the second stream (Tacotron2._defer) against the
same calls in line, and the overlapped pass against itself - an operand overwritten under a deferred call shows as a
difference between two passes."""
import pytest
import torch

from util import make_batch, small_hparams

pytestmark = pytest.mark.gpu

N, TI, TO = 4, 24, 40
ACT_RELU = 1


def _model(mode):
    from nspeech_amd.models import create_model
    hp = small_hparams()
    m = create_model("taco2", hp, device="cuda:0", dtype=mode, seed=5)
    m.deterministic = True
    return hp, m


def _pass(m, stats0, batch, overlap):
    m.overlap_wgrads = overlap
    m.flat_stats.copy_(stats0)               # the forward pass moves the BatchNorm moving statistics: same start every time
    m.initialize(batch[0], batch[1], None, batch[2], batch[3])
    m.backward()
    torch.cuda.synchronize()
    return m.flat_g.clone(), m.flat_stats.clone()


@pytest.mark.parametrize("mode", ["mixed", "bf16"])
def test_deferred_work_changes_no_bit(dev, mode):
    hp, m = _model(mode)
    stats0 = m.flat_stats.clone()
    batch = make_batch(hp, N, TI, TO, seed=2)
    g_off, s_off = _pass(m, stats0, batch, False)
    assert float(g_off.abs().max()) > 0
    first = None
    for rep in range(3):
        g_on, s_on = _pass(m, stats0, batch, True)
        assert m._side is not None and not m._deferred           # the second stream was used and is drained
        if first is None:
            first = (g_on, s_on)
            diff = (g_on != g_off).nonzero().flatten()
            assert diff.numel() == 0, "%d gradient words differ from the in-line pass, first at %d" % (
                diff.numel(), int(diff[0]))
            assert torch.equal(s_on, s_off), "BatchNorm moving statistics"
        else:
            assert torch.equal(g_on, first[0]), "overlapped pass %d differs from the first" % rep
            assert torch.equal(s_on, first[1])
    assert not torch.equal(s_off, stats0)


def test_bf16_input_cache_survives_a_b_a(dev):
    """_conv_bwd's cache of bf16 layer-input copies: with the weight gradients in line every layer of one `cin` shares
    one buffer, so input A, then B, then A again must not read B's copy through A's stale entry."""
    from nspeech_amd import ops
    hp, m = _model("mixed")
    batch = make_batch(hp, N, TI, TO, seed=3)
    m.overlap_wgrads = False
    m.initialize(batch[0], batch[1], None, batch[2], batch[3])
    m.backward()
    assert m._bf16_w(torch.float32) is not None                 # the mode that makes the copies
    d = m.dims
    Ce, k, Pi = hp.encoder_conv_channels, hp.encoder_conv_width, d["Pi"]
    rows = N * Pi
    gen = torch.Generator().manual_seed(9)
    dy = (torch.randn(rows, Ce, generator=gen) * 0.1).to(dev)
    dx = torch.zeros(rows, Ce, device=dev)
    assert m._enc_in[1].data_ptr() != m._enc_in[2].data_ptr()
    keep = (ops.F32_PASSES, ops.DETERMINISTIC_SPLITK)
    ops.F32_PASSES, ops.DETERMINISTIC_SPLITK = m.passes_bwd, True

    def run(i):
        m.flat_g.zero_()
        m._bwd_sums, m._deferred = {}, []
        m._conv_bwd("encoder/conv_%d" % i, m._enc_in[i], dy, Ce, Ce, k, ACT_RELU, N, TI, Pi, "enc%d" % i, dx)
        torch.cuda.synchronize()
        o = m._o("encoder/conv_%d/conv1d/kernel" % i)
        return m.flat_g[o:o + k * Ce * Ce].clone()

    try:
        m._x16_cache = None
        want = run(2)
        assert float(want.abs().max()) > 0
        m._x16_cache = {}
        assert torch.equal(run(2), want)        # A
        run(1)                                  # B: same cin, same buffer
        assert torch.equal(run(2), want)        # A again
    finally:
        ops.F32_PASSES, ops.DETERMINISTIC_SPLITK = keep
        m._x16_cache = None
