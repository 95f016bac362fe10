"""Training pieces for simple_wavenet (datasets/WavenetDataFeeder.py:19-167 of the reference).

Same walk as the reference: the item list is read in order and reshuffled at every wrap-around (:148-167); a waveform
is trimmed of leading / trailing silence (`trim_silence`, process.py:45-54, threshold 0.1), padded with
receptive_field zeros in front and cut into pieces of receptive_field + sample_size samples that overlap by the
receptive field (:104-125); pieces go through a shuffling buffer of `queue_size` entries that hands out random
elements once it holds more than min_dequeue_ratio * queue_size (tf.RandomShuffleQueue, :71-83), `batch_size` at a
time.

Local conditions (local_condition="mel"; default None: nothing below is computed and the walk, the pieces and the random
stream are what they were).  The reference attaches a mel image of receptive_field rows to every piece (:127-135), which
no layer's output length equals; here a piece carries the frame-rate rows of its own waveform's mel instead, in the
alignment WaveNetModel.initialize(hold=, t0=) and generate() share.  The mel of a trimmed waveform is taken once, before
the receptive_field zeros go in front, so row r covers the waveform's samples r * hop .. r * hop + hop - 1 (hop from the
audio hparams, utils/audio.py:_stft_parameters).  Piece k starts at absolute position a0 = k * sample_size - rf (negative:
inside the zeros) and gets the rows from r0 = max(0, a0) // hop on (mel_fn must return that row for every piece: at
least one row per started hop of the waveform, else ValueError), padded with its last real row to the fixed count
F = (T0 + hop - 2) // hop + 1 for T0 = rf + sample_size - 1 network-input positions, and t0 = a0 - r0 * hop: its position
m reads row max(0, m + t0) // hop of what it carries = row max(0, a0 + m) // hop of the mel."""
import random

import numpy as np

from ..utils import audio
from .datafeeder import load_librispeech_corpus, load_ljspeech_metadata, load_vctk_file_names
from .process import trim_silence  # noqa: F401  (process.py:45-54)


class WavenetFeeder(object):
    def __init__(self, hparams, receptive_field, ljspeech=None, vctk=None, librispeech=None, seed=0, loader=None,
                 silence_threshold=0.1, local_condition=None, mel_fn=None):
        self.hp = hparams
        self.rf = int(receptive_field)
        self.sample_size = int(hparams.sample_size)
        self.silence_threshold = silence_threshold
        self.items = load_ljspeech_metadata(ljspeech) if ljspeech else []
        self.items += load_vctk_file_names(vctk) if vctk else []
        self.items += load_librispeech_corpus(librispeech) if librispeech else []
        assert self.items, "No data found"
        pairs = sorted({(dataset, str(spk)) for _, _, spk, dataset in self.items})
        self.speaker2id = {v: k for k, v in enumerate(pairs)}
        self._rng = random.Random(seed)
        self._offset = 0
        self._loader = loader or audio.load_wav
        self._pool = []           # the shuffling buffer: (piece, speaker id)
        self.capacity = int(hparams.queue_size)
        self.min_after = int(hparams.min_dequeue_ratio * hparams.queue_size)
        self.speaker_ids = None
        if local_condition not in (None, "mel"):
            raise ValueError("local_condition %r: None or 'mel'" % (local_condition,))
        self.local_condition = local_condition
        self.local_conditions = self.lc_t0 = self.lc_hold = None
        if local_condition:
            self._mel_fn = mel_fn or (lambda wav: audio.melspectrogram(wav).T)      # [frames, num_mels]
            self.lc_hold = int(hparams.frame_shift_ms / 1000 * hparams.sample_rate)
            self.lc_frames = (self.rf + self.sample_size - 1 + self.lc_hold - 2) // self.lc_hold + 1

    def _next_pieces(self):
        if self._offset >= len(self.items):
            self._offset = 0
            self._rng.shuffle(self.items)
        path, _text, spk, dataset = self.items[self._offset]
        self._offset += 1
        wav = np.asarray(self._loader(path), np.float32)
        if self.silence_threshold is not None:
            wav = trim_silence(wav, self.silence_threshold)
        mel = None
        if self.local_condition and len(wav) > self.sample_size:        # (a shorter waveform gives no piece)
            mel = np.asarray(self._mel_fn(wav), np.float32)
            mel = mel.reshape(len(mel), -1)
        wav = np.pad(wav, [self.rf, 0], "constant")
        sid = self.speaker2id[dataset, str(spk)]
        out = []
        while len(wav) > self.rf + self.sample_size:
            piece = wav[:self.rf + self.sample_size].copy()
            if mel is None:
                out.append((piece, sid))
            else:
                a0 = len(out) * self.sample_size - self.rf
                r0 = max(0, a0) // self.lc_hold
                if r0 >= len(mel):      # (audio.melspectrogram has 1 + len // hop rows: every sample has its row)
                    raise ValueError("mel_fn gave %d rows of %d samples: the piece that starts at sample %d has none"
                                     % (len(mel), self.lc_hold, a0))
                rows = mel[r0:r0 + self.lc_frames]
                if len(rows) < self.lc_frames:
                    rows = np.concatenate([rows, np.repeat(rows[-1:], self.lc_frames - len(rows), axis=0)])
                out.append((piece, sid, rows.copy(), a0 - r0 * self.lc_hold))
            wav = wav[self.sample_size:]
        return out

    @property
    def size(self):
        return len(self._pool)

    def next_batch(self):
        """float32 [batch_size, receptive_field + sample_size]; .speaker_ids [batch_size]; with local_condition="mel" also
        .local_conditions float32 [batch_size, F, num_mels], .lc_t0 int32 [batch_size] (and .lc_hold = hop)."""
        n = int(self.hp.batch_size)
        idle = 0
        while len(self._pool) < max(n + self.min_after, 1):
            got = self._next_pieces()
            room = max(self.capacity, n + self.min_after) - len(self._pool)
            self._pool.extend(got[:max(room, 0)] if room < len(got) else got)
            idle = idle + 1 if not got else 0
            if idle > 2 * len(self.items):
                raise RuntimeError("no waveform is longer than sample_size after trimming silence")
        picks = sorted(self._rng.sample(range(len(self._pool)), n), reverse=True)
        batch = [self._pool.pop(i) for i in picks]
        self.speaker_ids = np.asarray([b[1] for b in batch], np.int32)
        if self.local_condition:
            self.local_conditions = np.stack([b[2] for b in batch])
            self.lc_t0 = np.asarray([b[3] for b in batch], np.int32)
        return np.stack([b[0] for b in batch])
