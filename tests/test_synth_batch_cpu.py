"""The host side of Synthesizer.synthesize_batch that needs no GPU: the padded text batch, the chunks of at most 32, and
the refusals and the empty call, which come before the model is touched."""
import numpy as np
import pytest

from nspeech_amd import hparams as hparams_mod
from nspeech_amd.synthesizer import MAX_BATCH, Synthesizer, batch_chunks, pad_text_batch


def test_pad_text_batch():
    seqs = [[5, 6, 7], [9], [1, 2, 3, 4, 8], [3, 3]]
    inputs, lengths = pad_text_batch(seqs)
    assert inputs.dtype == np.int32 and lengths.dtype == np.int32
    assert inputs.shape == (4, 5) and lengths.tolist() == [3, 1, 5, 2]
    for row, s in zip(inputs, seqs):
        assert row[:len(s)].tolist() == s and not row[len(s):].any()         # pad id 0, as the feeder's _pad
    one, n = pad_text_batch([[4, 2]])
    assert one.tolist() == [[4, 2]] and n.tolist() == [2]


def test_chunks_of_at_most_32_in_order():
    assert MAX_BATCH == 32
    chunks = batch_chunks(70)
    assert chunks == [(0, 32), (32, 64), (64, 70)]
    items = list(range(70))
    parts = [items[a:b] for a, b in chunks]
    assert [len(p) for p in parts] == [32, 32, 6] and sum(parts, []) == items
    assert batch_chunks(0) == [] and batch_chunks(32) == [(0, 32)] and batch_chunks(33) == [(0, 32), (32, 33)]


def test_empty_call_and_refusals_need_no_model():
    synth = Synthesizer(hparams_mod.load("taco2"))
    assert synth.model is None
    assert synth.synthesize_batch([]) == []
    assert synth.synthesize_batch([], speaker_ids=[]) == []
    with pytest.raises(ValueError, match="speaker_ids"):
        synth.synthesize_batch(["a", "b", "c"], speaker_ids=[0, 1])
    with pytest.raises(ValueError, match="speaker_ids"):
        synth.synthesize_batch([], speaker_ids=[0])
    with pytest.raises(ValueError, match="vocoder"):
        synth.synthesize_batch(["a"], vocoder="melgan")
    with pytest.raises(ValueError, match="load_vocoder"):
        synth.synthesize_batch(["a"], vocoder="wavenet")
