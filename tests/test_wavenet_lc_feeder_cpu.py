"""WavenetFeeder(local_condition="mel") on the host: every piece carries the frame-rate rows of its own waveform's mel in the
alignment of WaveNetModel.initialize(hold=, t0=) - position m of a piece reads row max(0, m + t0) // hop of what the piece
carries, which must be row max(0, a0 + m) // hop of the mel for the piece's absolute start a0.  Stub loader, stub mel_fn
(mel_fn(wav)[f] = f plus a tag of the waveform, so a row says where it came from): no GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RF, SS, HOP = 50, 100, 16
WAVES = {"A.wav": (0.5 * np.sin(np.arange(1, 1001) * 0.37)).astype(np.float32),
         "B.wav": (0.5 * np.cos(np.arange(1, 701) * 0.21)).astype(np.float32)}
TAG = {1000: 1000.0, 700: 2000.0}                 # by waveform length


def _feeder(tmp_path, **kw):
    from nspeech_amd import hparams as H
    from nspeech_amd.datasets.wavenet_feeder import WavenetFeeder
    hp = H.load("wavenet")
    hp.sample_size, hp.batch_size, hp.queue_size = SS, 4, 16
    hp.sample_rate, hp.frame_shift_ms = 16000, 1.0             # hop = 16 samples
    if not os.path.exists(tmp_path / "wavs"):
        os.makedirs(tmp_path / "wavs")
        with open(tmp_path / "metadata.csv", "w") as f:
            f.write("A|x|x\nB|y|y\n")
    return WavenetFeeder(hp, RF, ljspeech=str(tmp_path), loader=lambda p: WAVES[os.path.basename(p)], silence_threshold=None,
                         seed=3, **kw)


def _mel(wav):
    """[frames, 2]: column 0 = the row's index + the waveform's tag, column 1 = the index alone; 1 + len // hop rows"""
    f = np.arange(1 + len(wav) // HOP, dtype=np.float32)
    return np.stack([f + TAG[len(wav)], f], axis=1)


def test_every_position_reads_its_own_mel_row(tmp_path):
    fd = _feeder(tmp_path, local_condition="mel", mel_fn=_mel)
    T0 = RF + SS - 1
    F = (T0 + HOP - 2) // HOP + 1
    assert fd.lc_hold == HOP and fd.lc_frames == F
    seen = set()
    for _ in range(4):
        batch = fd.next_batch()
        lc, t0 = fd.local_conditions, fd.lc_t0
        assert lc.shape == (4, F, 2) and lc.dtype == np.float32 and t0.shape == (4,) and t0.dtype == np.int32
        for n in range(4):
            # which waveform and which piece: the piece's samples say (pieces of the padded waveform every SS samples)
            found = None
            for name, w in WAVES.items():
                padded = np.concatenate([np.zeros(RF, np.float32), w])
                for k in range((len(padded) - RF - 1) // SS + 1):
                    if len(padded) - k * SS > RF + SS and np.array_equal(batch[n], padded[k * SS:k * SS + RF + SS]):
                        found = (name, k)
            assert found is not None
            seen.add(found)
            w = WAVES[found[0]]
            mel = _mel(w)
            a0 = found[1] * SS - RF
            m = np.arange(T0)
            got = lc[n, np.maximum(0, m + int(t0[n])) // fd.lc_hold]
            rows = np.maximum(0, a0 + m) // HOP
            assert rows.max() < len(mel)                       # (these waveforms never run out of real rows inside a piece)
            assert np.array_equal(got, mel[rows]), (found, int(t0[n]))
            assert (0 <= t0[n] < HOP) if a0 >= 0 else t0[n] == a0
    assert len(seen) > 4 and {s[0] for s in seen} == set(WAVES)


def test_rows_past_the_mel_repeat_the_last_real_row(tmp_path):
    # waveform A: 9 pieces, the last from a0 = 750 = row 46 on; a mel of 47 rows ends inside every later piece
    short = lambda wav: _mel(wav)[:47]             # noqa: E731
    fd = _feeder(tmp_path, local_condition="mel", mel_fn=short)
    pieces = fd._next_pieces()
    assert len(pieces) == 9 and len(pieces[0]) == 4
    for k, (_p, _sid, rows, t0) in enumerate(pieces):
        assert rows.shape == (fd.lc_frames, 2)
        a0 = k * SS - RF
        r0 = max(0, a0) // HOP
        assert t0 == a0 - r0 * HOP and t0 < HOP                   # so the fixed count always reaches the last position
        assert np.array_equal(rows[:, 1], np.minimum(np.arange(r0, r0 + fd.lc_frames), 46))
    # a mel without the first row of some piece is refused, not stretched
    fd = _feeder(tmp_path, local_condition="mel", mel_fn=lambda wav: _mel(wav)[:46])
    try:
        fd._next_pieces()
    except ValueError as e:
        assert "46 rows" in str(e)
    else:
        raise AssertionError("a mel that ends before a piece starts must be refused")


def test_default_feeder_never_heard_of_the_option(tmp_path):
    a = _feeder(tmp_path)
    b = _feeder(tmp_path, local_condition=None, mel_fn=_mel)
    c = _feeder(tmp_path, local_condition="mel", mel_fn=_mel)
    for _ in range(5):
        x, y, z = a.next_batch(), b.next_batch(), c.next_batch()
        assert np.array_equal(x, y) and np.array_equal(a.speaker_ids, b.speaker_ids)
        assert np.array_equal(x, z) and np.array_equal(a.speaker_ids, c.speaker_ids)      # the option draws no random number
        assert getattr(a, "local_conditions", None) is None and getattr(b, "local_conditions", None) is None
    assert all(len(p) == 2 for p in a._next_pieces())
    try:
        _feeder(tmp_path, local_condition="linear")
    except ValueError:
        pass
    else:
        raise AssertionError("an unknown local_condition must be refused")
