"""DataFeeder.target_lengths: the frame count of every row of the batch that next_batch() just returned, in the batch's
row order (after the in-batch shuffle), with and without the prefetch thread.  The reference never masks the padding, so
its batches carry no such thing; the guided attention loss needs it.  Feature extraction is stubbed (it needs the GPU)."""
import os
import random

import numpy as np

from nspeech_amd import hparams as hparams_mod
from nspeech_amd.datasets.datafeeder import DataFeeder, prepare_batch


def _corpus(tmp_path, n):
    os.makedirs(tmp_path / "wavs", exist_ok=True)
    with open(tmp_path / "metadata.csv", "w") as f:
        for i in range(n):
            f.write("utt%03d|raw|%s\n" % (i, " ".join(["word"] * (1 + i % 4))))
    return str(tmp_path)


def _feeder(tmp_path, prefetch, n=30):
    hp = hparams_mod.load("taco2")
    hp.batch_size, hp.batch_group_size, hp.outputs_per_step = 4, 3, 5

    def loader(path):
        return int(os.path.basename(path)[3:6])

    def features(i):           # utterance i: 11 .. 47 frames, every frame of it holds the value i + 1
        T = 11 + (i * 7) % 37
        return (np.full((hp.num_freq, T), float(i + 1), np.float32), np.full((hp.num_mels, T), float(i + 1), np.float32))
    return DataFeeder(hp, ljspeech=_corpus(tmp_path, n), seed=4, prefetch=prefetch, features=features, loader=loader,
                      trim=False)


def _check(f, batch):
    inputs, lengths, mel, lin = batch
    tl = f.target_lengths
    assert isinstance(tl, np.ndarray) and tl.dtype == np.int32 and tl.shape == (mel.shape[0],)
    for i in range(mel.shape[0]):
        utt = int(mel[i, 0, 0]) - 1                           # which utterance sits in row i
        assert tl[i] == 11 + (utt * 7) % 37
        assert (mel[i, :tl[i]] == utt + 1).all() and (lin[i, :tl[i]] == utt + 1).all()
        assert not mel[i, tl[i]:].any() and not lin[i, tl[i]:].any()       # rows past it are padding
    assert mel.shape[1] > tl.max() and mel.shape[1] % 5 == 0               # + 1 frame, rounded up to r
    return tl


def test_target_lengths_follow_their_rows(tmp_path):
    f = _feeder(tmp_path, prefetch=False)
    assert f.target_lengths is None
    seen = [_check(f, f.next_batch()).tolist() for _ in range(9)]
    assert any(row != sorted(row) for row in seen)        # the in-batch shuffle happened: the lengths moved with it
    assert len({tuple(r) for r in seen}) > 1


def test_prefetch_thread_carries_the_same_lengths(tmp_path):
    a, b = _feeder(tmp_path / "a", prefetch=False), _feeder(tmp_path / "b", prefetch=True)
    try:
        for _ in range(8):
            # the thread has queued batches ahead of this one: the attribute must belong to the batch just returned
            ta, tb = _check(a, a.next_batch()), _check(b, b.next_batch())
            assert np.array_equal(ta, tb)
    finally:
        b.stop()


def test_prepare_batch_reports_lengths_without_changing_what_it_returns():
    mk = lambda: [(np.arange(2, 2 + L, dtype=np.int32), 0, np.ones((T, 8), np.float32), np.ones((T, 9), np.float32))
                  for L, T in ((5, 17), (9, 24), (3, 20), (4, 7))]
    plain = prepare_batch(mk(), 5, random.Random(3))
    frames = []
    out = prepare_batch(mk(), 5, random.Random(3), target_lengths=frames)
    assert len(plain) == len(out) == 5 and all(np.array_equal(x, y) for x, y in zip(plain, out))
    assert frames == [int(out[3][i, :, 0].sum()) for i in range(4)] and sorted(frames) == [7, 17, 20, 24]
