"""Utterance processing in front of the feeder (datasets/process.py:23-68 of the reference): load -> trim the silent ends
-> both spectrograms.  `trim_wav` is what the training path uses (process.py:27); `trim_silence` (process.py:45-54) is the
WaveNet feeder's.

Frame energies come from one running sum of squares (float64) instead of a frame matrix: a 10 s utterance is 391 frames of
1024 samples, and the decision per frame is a comparison of two sums, so the intervals are integers that either agree with
the oracle's per-frame loops or do not (`tests/test_feeder_cpu.py`)."""
import os

import numpy as np

from ..utils import audio


def _loud_frames(wav, top_db, frame_length, hop_length):
    """[3P] librosa 0.6.0 effects._signal_to_frame_nonsilent with ref = np.max: frames (centred, reflect padded) whose mean
    square is within top_db of the loudest frame's; both sides of the ratio are floored at 1e-10 (power_to_db's amin)."""
    y = np.pad(np.asarray(wav, np.float64), frame_length // 2, mode="reflect")
    n_frames = 1 + (len(y) - frame_length) // hop_length
    sq = np.concatenate([[0.0], np.cumsum(y * y)])
    starts = np.arange(n_frames) * hop_length
    mse = np.maximum((sq[starts + frame_length] - sq[starts]) / frame_length, 0.0)
    return _loud_from_power(mse, top_db)


def _loud_from_power(mse, top_db):
    """The decision of _loud_frames on the frames' mean squares (host sums or ns_frame_power's)."""
    amin = 1e-10
    return 10.0 * np.log10(np.maximum(amin, mse)) - 10.0 * np.log10(max(amin, float(mse.max()))) > -top_db


def _intervals(loud, hop_length, num_samples):
    """Runs of loud frames -> [start, end) sample intervals, clipped to the signal."""
    edges = np.flatnonzero(np.diff(loud.astype(np.int64))) + 1
    edges = np.concatenate([[0] if loud[0] else [], edges, [len(loud)] if loud[-1] else []]).astype(np.int64)
    return np.minimum(edges * hop_length, num_samples).reshape(-1, 2)


def split(wav, top_db=60, frame_length=2048, hop_length=512):
    """[3P] librosa 0.6.0 effects.split: [start, end) sample intervals of the runs of loud frames, clipped to the signal."""
    return _intervals(_loud_frames(wav, top_db, frame_length, hop_length), hop_length, len(wav))


def trim_silence(wav, threshold, frame_length=2048, hop_length=512):
    """process.py:45-54 over librosa.feature.rmse [3P, librosa 0.6: centred frames of 2048 every 512 samples, reflect
    padded] -> wav[first loud frame * 512 : last loud frame * 512]; all silence -> empty."""
    if wav.size < frame_length:
        frame_length = wav.size
    if wav.size == 0:
        return wav
    y = np.pad(wav.astype(np.float64), frame_length // 2, mode="reflect")
    n_frames = 1 + (len(y) - frame_length) // hop_length
    sq = np.concatenate([[0.0], np.cumsum(y * y)])
    starts = np.arange(n_frames) * hop_length
    energy = np.sqrt((sq[starts + frame_length] - sq[starts]) / frame_length)
    loud = np.nonzero(energy > threshold)[0] * hop_length
    return wav[loud[0]:loud[-1]] if loud.size else wav[:0]


def _find_start(splits, min_samples=2000):
    """process.py:56-60."""
    for split_start, split_end in splits:
        if split_end - split_start > min_samples:
            return max(0, int(split_start) - min_samples)
    return 0


def _find_end(splits, num_samples, min_samples=2000):
    """process.py:63-67."""
    for split_start, split_end in reversed(list(splits)):
        if split_end - split_start > min_samples:
            return min(num_samples, int(split_end) + min_samples)
    return num_samples


def trim_wav(wav, threshold_db=25):
    """process.py:39-42: trims silence from the ends of the wav (the second positional argument of librosa's split is
    top_db; frames of 1024 every 512 samples)."""
    splits = split(wav, threshold_db, frame_length=1024, hop_length=512)
    return wav[_find_start(splits):_find_end(splits, len(wav))]


# ---------------------------------------------------------------- the same decisions for a waveform on the device
# Only the frames' energies are per-sample work; ns_frame_power (csrc/frontend.hip) forms them where the waveform is and
# a few hundred float64 values come back.  The thresholds, the run detection and _find_start / _find_end are the host
# functions above.  The kernel adds each frame directly, the host forms differences of one running sum: a frame within
# rounding (about 1e-4 dB on a 10 s clip) of the threshold may fall on the other side.
def frame_power_device(wav, frame_length, hop_length):
    """wav: float32 CUDA tensor [n] -> float64 NumPy [1 + n // hop_length], the mean square of every centred,
    reflect-padded frame.  The read-back waits for an event on the current stream and for nothing else: no device-wide
    synchronise, so a feeder thread that calls this never stalls the training stream."""
    import torch
    from .. import _lib as L, ops
    assert torch.is_tensor(wav) and wav.is_cuda and wav.dtype == torch.float32 and wav.dim() == 1
    wav = wav.contiguous()
    n = wav.numel()
    with torch.cuda.device(wav.device):
        out = torch.empty(1 + n // hop_length, dtype=torch.float64, device=wav.device)
        p = L.struct("ns_frame_power_params")
        p.x, p.n, p.frame_length, p.hop = ops.ptr(wav), n, int(frame_length), int(hop_length)
        p.out, p.n_frames = ops.ptr(out), out.numel()
        L.call("ns_frame_power", p, ops.stream())
        host = torch.empty(out.shape, dtype=torch.float64, pin_memory=True)
        host.copy_(out, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        ev.synchronize()
    return host.numpy().copy()


def trim_bounds_device(wav, threshold_db=25):
    """(start, end) with trim_wav(w) == w[start:end], for a float32 CUDA tensor."""
    n = wav.numel()
    if n <= 512:        # shorter than the reflection of one frame (25 ms at 20 kHz): nothing worth a launch
        host = wav.cpu().numpy()
        splits = split(host, threshold_db, frame_length=1024, hop_length=512)
    else:
        loud = _loud_from_power(frame_power_device(wav, 1024, 512), threshold_db)
        splits = _intervals(loud, 512, n)
    return _find_start(splits), _find_end(splits, n)


def trim_silence_bounds_device(wav, threshold, frame_length=2048, hop_length=512):
    """(start, end) with trim_silence(w, threshold) == w[start:end] for a float32 CUDA tensor of at least frame_length
    samples; all silence -> (0, 0)."""
    if wav.numel() < frame_length:
        raise ValueError("trim_silence_bounds_device: %d samples, fewer than one frame of %d" % (wav.numel(), frame_length))
    energy = np.sqrt(frame_power_device(wav, frame_length, hop_length))
    loud = np.nonzero(energy > threshold)[0] * hop_length
    return (int(loud[0]), int(loud[-1])) if loud.size else (0, 0)


def process_utterance_device(wav_path, dataset_id=None):
    """process_utterance with everything behind the file decode on the device: one upload of the native-rate samples,
    ns_resample, ns_frame_power (+ one small read-back for the trim bounds), ns_spectrogram.  Returns (id, trimmed wav,
    linear [T, F], mel [T, M], n_frames) with the three arrays as float32 CUDA tensors holding process_utterance's
    values."""
    idx = os.path.basename(wav_path)[:-4]
    wav = audio.load_wav_device(wav_path)
    start, end = trim_bounds_device(wav)
    wav = wav[start:end]
    lin, mel = audio.spectrogram_and_mel_device(wav)
    return idx, wav, lin, mel, lin.shape[0]


def process_utterance(wav_path, dataset_id=None, loader=None):
    """process.py:23-36: (id, trimmed wav, linear [T, F], mel [T, M], n_frames); both spectrograms from ONE pass of the
    fused GPU feature kernel."""
    idx = os.path.basename(wav_path)[:-4]
    wav = trim_wav((loader or audio.load_wav)(wav_path))
    lin, mel = audio.spectrogram_and_mel(wav)
    return idx, wav, lin.T, mel.T, lin.shape[1]


def build_from_path(filenames, num_workers=1, tqdm=lambda x: x, limit=0):
    """process.py:10-18.  The reference farms utterances out to worker processes because its two librosa STFTs are host
    work; here the features are one GPU launch per utterance, so the walk is sequential (num_workers is accepted and
    ignored).  Keeps the reference's `len(futures) > limit` cut, i.e. limit + 1 items."""
    out = []
    for wav_path, _text, _speaker, dataset_id in filenames:
        if limit and len(out) > limit:
            break
        out.append(process_utterance(wav_path, dataset_id))
    return list(tqdm(out))
