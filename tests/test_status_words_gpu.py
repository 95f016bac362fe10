"""The status words of a training step: every consulted persistent launch has a work area of its own
(Tacotron2._persistent), so a word raised in the forward pass is still raised when check_status() and ns_adam read it.

Every launcher clears its work area, status word included.  Up to version 107 Tacotron-1's GRUs shared work areas - a
BiGRU group's forward and backward launch, all four windows of both passes of a decoder GRU - so the next launch erased
a raised word and Adam applied an update computed from invalid activations.

No kernel is made to time out here: a word is "raised" by writing an int into it from the host between two passes.

Shapes: Tacotron-1 at the shipped widths at (4, 24, 40) in `mixed` mode, the smallest shape of
test_taco1_fullwidth_gpu.py - 8 decoder steps, so _gru_pair runs four windows of two steps, and N = 4 pads a 16-row
group; Tacotron-2 at (2, 24, 40) in `mixed` mode, the smallest shape of test_taco2_fullwidth_gpu.py, where the decoder
LSTMs take the wide kernels and the expand BiLSTM and the attention RNN the cluster kernels.

read_losses() asks check_status() before it looks at the skip flag, so with the word still raised it reports the
time-out itself.  The tests therefore lower the word again (from the host, after the optimiser has run) in front of
read_losses(): what then raises is the flag that ns_adam left, the skipped-step error."""
import numpy as np
import pytest
import torch

from util import make_batch

pytestmark = pytest.mark.gpu

PERSISTENT = ("seq", "cluster", "wide", "persistent")
SHAPES = {"taco1": (4, 24, 40), "taco2": (2, 24, 40)}


@pytest.fixture(scope="module")
def models(dev):
    """name -> (model, batch), built once: a skipped step changes no parameter, and every pass relaunches (and so
    clears) every work area."""
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.models import create_model
    cache = {}

    def get(name):
        if name not in cache:
            hp = hparams_mod.load(name)
            N, Ti, To = SHAPES[name]
            m = create_model(name, hp, device="cuda:0", dtype="mixed", seed=5)
            m.add_optimizer(global_step=0)
            cache[name] = (m, make_batch(hp, N, Ti, To, seed=N + 40))
        return cache[name]
    return get


def _set_word(w, value):
    torch.cuda.synchronize()
    w[:1].view(torch.int32).copy_(torch.tensor([value], dtype=torch.int32))
    torch.cuda.synchronize()


@pytest.mark.parametrize("name, count", [("taco1", 22), ("taco2", None)])
def test_every_consulted_launch_has_its_own_work_area(models, name, count):
    m, (inputs, lengths, mel, lin) = models(name)
    m.initialize(inputs, lengths, None, mel, lin)
    m.backward()
    m.check_status()
    words = m._status_words
    ptrs = [w.data_ptr() for w in words.values()]
    assert len(set(ptrs)) == len(ptrs), sorted(words)
    forms = {k: v for k, v in m.last_paths.items() if v in PERSISTENT}
    for k in forms:
        key = tuple(k.split(":"))
        assert key in words or any(w[:len(key)] == key for w in words), (k, sorted(words))
    if name == "taco1":
        # two BiGRU groups and the attention RNN, forward and backward; 2 GRUs x 4 windows x 2 passes
        assert m.last_paths["gru_pair"] == "pipelined x4", m.last_paths
        assert len(words) == count, sorted(words)
        assert forms == {k: "seq" for k in ("enc_gru:fwd", "enc_gru:bwd", "post_gru:fwd", "post_gru:bwd", "gru_1:fwd",
                                            "gru_1:bwd", "gru_2:fwd", "gru_2:bwd")} | {"attn:fwd": "cluster", "attn:bwd": "cluster"}
    else:
        assert "wide" in forms.values() and "cluster" in forms.values(), m.last_paths
        assert len(words) == len(forms), (sorted(words), forms)


def _forward_word_survives(m, batch, key):
    inputs, lengths, mel, lin = batch
    before = m.numpy_params()
    step = m.global_step
    m.initialize(inputs, lengths, None, mel, lin)
    w = m._status_words[key]
    _set_word(w, 7)
    m.backward()
    with pytest.raises(RuntimeError) as e:
        m.check_status()
    assert repr(key) in str(e.value) and "status 7" in str(e.value), str(e.value)
    m.apply_gradients()
    _set_word(w, 0)               # (see the module's docstring: read_losses() would report the time-out itself)
    with pytest.raises(RuntimeError, match="the optimiser step was skipped"):
        m.read_losses()
    assert m.global_step == step
    after = m.numpy_params()
    assert all(np.array_equal(before[k], after[k]) for k in before), [k for k in before if not np.array_equal(before[k], after[k])]


@pytest.mark.parametrize("key", [("enc_gru", "fwd"), ("gru_1", "fwd", 0), ("gru_2", "fwd", 3), ("attn", "fwd")],
                         ids=lambda k: "-".join(str(x) for x in k))
def test_taco1_forward_word_survives_the_backward_pass(models, key):
    """(On version 107, with the shared areas - keys without the window - the three GRU cases fail at check_status():
    the backward launch has cleared the word.  profiles/persistent_launch.txt.)"""
    m, batch = models("taco1")
    _forward_word_survives(m, batch, key)


def test_taco2_forward_word_survives_the_backward_pass(models):
    m, batch = models("taco2")
    _forward_word_survives(m, batch, ("dec1", "fwd"))
