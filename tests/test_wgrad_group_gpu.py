"""The queued weight gradients of the Tacotron-2 backward pass as grouped launches (NS_WGRAD_GROUP, ops.gemm_group)
against the same pass with one launch per product and column sum: in deterministic mode the gradient must not change a
bit, and the grouped pass must repeat itself.  The model is the small one of tests/test_backward_schedule_gpu.py; the
BatchNorm moving statistics are put back before every pass, as there."""
import os

import pytest
import torch

from util import make_batch, small_hparams

pytestmark = pytest.mark.gpu

N, TI, TO = 4, 24, 40
ALL_QUEUES = "decoder,postnet,head"


def _pass(m, stats0, batch, group):
    keep = os.environ.get("NS_WGRAD_GROUP")
    if group is None:
        os.environ.pop("NS_WGRAD_GROUP", None)
    else:
        os.environ["NS_WGRAD_GROUP"] = group
    try:
        m.overlap_wgrads = True
        m.flat_stats.copy_(stats0)
        m.initialize(batch[0], batch[1], None, batch[2], batch[3])
        m.backward()
        torch.cuda.synchronize()
    finally:
        if keep is None:
            os.environ.pop("NS_WGRAD_GROUP", None)
        else:
            os.environ["NS_WGRAD_GROUP"] = keep
    return m.flat_g.clone(), list(m.wgrad_group)


@pytest.mark.parametrize("mode", ["mixed", "bf16"])
def test_grouped_queues_change_no_bit(dev, mode):
    from nspeech_amd.models import create_model
    hp = small_hparams()
    m = create_model("taco2", hp, device="cuda:0", dtype=mode, seed=5)
    m.deterministic = True
    stats0 = m.flat_stats.clone()
    batch = make_batch(hp, N, TI, TO, seed=2)
    g_single, rec = _pass(m, stats0, batch, "")
    assert rec == [], rec                                    # the empty list: today's launches, nothing grouped
    assert float(g_single.abs().max()) > 0
    first = None
    for rep in range(3):
        g, rec = _pass(m, stats0, batch, ALL_QUEUES)          # every queue grouped (the default groups the decoder queue)
        assert m._side is not None and not m._deferred
        assert rec, "no grouped launch was recorded"
        if first is None:
            first = g
            diff = (g != g_single).nonzero().flatten()
            assert diff.numel() == 0, "%d gradient words differ from the single launches, first at %d" % (
                diff.numel(), int(diff[0]))
        else:
            assert torch.equal(g, first), "grouped pass %d differs from the first" % rep
    # the decoder queue: the output projection's pair rides the flush in front of the decoder LSTMs' recurrences, the two
    # LSTMs' and the attention RNN's products and column sums the one in front of the encoder - at most two launches
    dec = [launches for queues, launches in rec if "decoder" in queues.split("+")]
    assert dec and sum(len(l) for l in dec) <= 2 and sum(sum(l) for l in dec) > 2, rec


def test_one_queue_at_a_time(dev):
    from nspeech_amd.models import create_model
    hp = small_hparams()
    m = create_model("taco2", hp, device="cuda:0", dtype="mixed", seed=5)
    m.deterministic = True
    stats0 = m.flat_stats.clone()
    batch = make_batch(hp, N, TI, TO, seed=2)
    g_single, _ = _pass(m, stats0, batch, "")
    for queues in (None, "decoder", "postnet,head"):         # None: the default
        g, rec = _pass(m, stats0, batch, queues)
        assert rec and all(set(q.split("+")) <= set((queues or "decoder").split(",")) for q, _ in rec), rec
        assert torch.equal(g, g_single), queues
