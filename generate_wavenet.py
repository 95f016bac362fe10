#!/usr/bin/env python3
"""Waveform generation from a simple_wavenet checkpoint, the reference's generate_wavenet.py surface (:48-224): positional
checkpoint, --samples --temperature --wav_out_path --save_every --fast_generation --wav_seed.

The reference script builds WaveNetModel and needs a wavenet_params.json that the repository does not ship
(generate_wavenet.py:21,51); here the network is wavenet.yaml's (+ --hparams; --gc_channels / --gc_cardinality / --gc_id
for a speaker-conditioned checkpoint of train_wavenet.py --model wavenet, :214-231), restored from
train_wavenet.py's model.ckpt-<step>.  --fast_generation true (default) at temperature 1.0 = the persistent incremental
generator on the GPU (one workgroup per waveform; float64 softmax and inverse-CDF draw in the kernel).
--incremental_temperature true keeps that generator at ANY --temperature - the kernel draws from softmax(logits /
temperature), scale_prediction below in float64; --temperature 0 is argmax - and then a local condition is accepted at any
temperature too; it needs --fast_generation true.
--stop_at_endpoint true (default false: the output is what it was) arms the incremental generator with
audio.endpoint_rule() - it stops drawing behind the first 0.8 s that stay under -40 dB, where audio.find_endpoint would
cut the finished waveform - and writes the waveform cut at that end; it needs the incremental generator as well, in one
call (no --save_every).
--stream_chunk N (the incremental generator again, not with --save_every) draws the same --samples with the same
random numbers as the run without it, as ONE generation resumed every N samples (generate_stream: no re-seeding, unlike
--save_every), and rewrites --wav_out_path after every chunk while the next one is being drawn; the finished file is the
file of the run without the flag.  With --stop_at_endpoint true the partial files hold what has been drawn and the
finished one is cut at the end point.
--lc_channels N --local_condition FILE.npy --lc_hold H draw from a locally conditioned checkpoint: the file is float
[rows, N], row r conditions generated samples r * H .. r * H + H - 1 (a mel spectrogram: H = the hop), the seed in
front takes row 0; this path is the incremental generator's alone.  Any other
temperature, or --fast_generation false, takes the full-window path of generate_wavenet.py:104-142: predict_proba over the
last receptive_field samples, temperature scaling and the draw on the host, including the reference's own consistency
check at temperature 1.0 (:133-138, scaled == unscaled); without --incremental_temperature that routing is unchanged."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from nspeech_amd import hparams as hparams_mod  # noqa: E402
from nspeech_amd.models import create_model  # noqa: E402
from nspeech_amd.models.wavenet import mu_law_decode, mu_law_encode  # noqa: E402
from nspeech_amd.utils import audio  # noqa: E402

SAMPLES = 16000
TEMPERATURE = 1.0
SILENCE_THRESHOLD = 0.1
SAMPLE_RATE = 16000          # the reference reads it from wavenet_params.json; WaveNet runs on 16 kHz mu-law audio


def write_wav(waveform, sample_rate, filename):
    import wave
    y = np.clip(np.asarray(waveform, np.float64), -1.0, 1.0)
    with wave.open(filename, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sample_rate)
        f.writeframes((y * 32767.0).astype("<i2").tobytes())
    print("Updated wav file at {}".format(filename))


def create_seed(filename, quantization_channels, window_size, silence_threshold=SILENCE_THRESHOLD):
    """generate_wavenet.py:32-45: load, trim silence, mu-law encode, keep at most window_size samples."""
    from nspeech_amd.datasets.wavenet_feeder import trim_silence
    wav = trim_silence(np.asarray(audio.load_wav(filename), np.float32), silence_threshold)
    return mu_law_encode(wav[None], quantization_channels)[0][:window_size]


def scale_prediction(prediction, temperature):
    """generate_wavenet.py:124-130."""
    with np.errstate(divide="ignore"):
        scaled = np.log(prediction) / temperature
        scaled = scaled - np.logaddexp.reduce(scaled)
        return np.exp(scaled)


def main(args):
    inc_t = bool(getattr(args, "incremental_temperature", False))
    if inc_t and not args.fast_generation:
        raise ValueError("--incremental_temperature true tempers the incremental generator's draws: it needs "
                         "--fast_generation true (the full-window path scales on the host at any --temperature already)")
    stop = bool(getattr(args, "stop_at_endpoint", False))
    if stop and not (args.fast_generation and (inc_t or args.temperature == 1.0)):
        raise ValueError("--stop_at_endpoint true is the incremental generator's own stop: it needs --fast_generation true and "
                         "--temperature 1.0, or any --temperature with --incremental_temperature true")
    if stop and getattr(args, "save_every", None):
        raise ValueError("--stop_at_endpoint true draws in one call (the rule counts silence across the whole waveform): "
                         "no --save_every")
    chunk = getattr(args, "stream_chunk", None)
    if chunk and not (args.fast_generation and (inc_t or args.temperature == 1.0)):
        raise ValueError("--stream_chunk N hands out the incremental generator's samples while it draws: it needs "
                         "--fast_generation true and --temperature 1.0, or any --temperature with --incremental_temperature true")
    if chunk and getattr(args, "save_every", None):
        raise ValueError("--stream_chunk N and --save_every N are two ways to write partial results (one generator resumed "
                         "chunk by chunk, or one restarted per chunk): one of them")
    hp = hparams_mod.load("wavenet")
    hp.parse(args.hparams)
    gc = None
    if args.gc_channels is not None:                # generate_wavenet.py:221-231: the speaker whose voice is drawn
        hp.gc_channels, hp.gc_category_cardinality = args.gc_channels, args.gc_cardinality
        gc = np.asarray([args.gc_id])
    lc = None
    if args.lc_channels:
        hp.lc_channels = args.lc_channels
        if not args.local_condition:
            raise ValueError("--lc_channels needs --local_condition FILE.npy")
        if not (args.fast_generation and (inc_t or args.temperature == 1.0)):
            raise ValueError("A local condition is drawn from by the incremental generator only: --fast_generation true and "
                             "--temperature 1.0, or any --temperature with --incremental_temperature true (predict_proba "
                             "takes no local condition).")
        lc = np.asarray(np.load(args.local_condition), np.float32)
        if lc.ndim != 2 or lc.shape[1] != args.lc_channels:
            raise ValueError("--local_condition holds %s, expected [rows, %d]" % (lc.shape, args.lc_channels))
        if args.lc_hold < 1:
            raise ValueError("--lc_hold must be at least 1 (generated samples per row of --local_condition), got %d" % args.lc_hold)
        if lc.shape[0] * args.lc_hold < args.samples:
            raise ValueError("--local_condition has %d rows of --lc_hold %d samples: fewer than --samples %d"
                             % (lc.shape[0], args.lc_hold, args.samples))
    elif args.local_condition:
        raise ValueError("--local_condition needs --lc_channels N with N > 0: the checkpoint's local condition channels")
    full = bool(hp.use_biases or hp.scalar_input or hp.gc_channels or hp.lc_channels)
    net = create_model("wavenet" if full else "simple_wavenet", hp, device="cuda:0", dtype=args.precision)
    cond = dict(global_conditions=gc) if full else {}
    cond1 = dict(global_condition=None if gc is None else gc[0]) if full else {}
    print("Restoring model from {}".format(args.checkpoint))
    net.load_state_dict(torch.load(args.checkpoint, map_location="cpu", weights_only=True))
    q, rf = hp.quantization_channels, net.rf
    rng = np.random.default_rng(args.seed)
    if args.wav_seed:
        waveform = create_seed(args.wav_seed, q, rf).tolist()
        if len(waveform) < rf:                      # the generator wants a full window: silence in front
            waveform = [q // 2] * (rf - len(waveform)) + waveform
    else:                                           # silence with a single random sample at the end (:84-86)
        waveform = [q // 2] * (rf - 1) + [int(rng.integers(q))]
    fast = args.fast_generation and (inc_t or args.temperature == 1.0)
    if fast:
        if inc_t:
            cond.update(temperature=args.temperature)
        if stop:
            cond.update(endpoint=audio.endpoint_rule())
        done = 0
        if chunk:                                   # ONE generator, resumed chunk by chunk: the run without chunking, heard earlier
            if lc is not None:                      # (as below at done = 0, n = samples: every row is on the device from the start)
                cond.update(local_conditions=lc[None, :(args.samples - 1) // args.lc_hold + 1], hold=args.lc_hold, t0=-rf)
            first = len(waveform)
            stream = net.generate_stream(np.asarray(waveform[-rf:], np.int32), args.samples, chunk,
                                         uniforms=rng.random((1, args.samples)), **cond)
            for piece in stream:
                waveform.extend(int(x) for x in piece[0])
                done = stream.drawn
                print("Sample {:3<d}/{:3<d}".format(done, args.samples), end="\r")
                last = done >= args.samples or (stop and bool(stream.fired[0]))
                if args.wav_out_path and not last:
                    write_wav(mu_law_decode(np.asarray(waveform), q), SAMPLE_RATE, args.wav_out_path)
            if stop:                                # the generated samples in front of their end point
                n_kept = int(net.last_ends[0].item())
                print("End point at sample {} of {}".format(n_kept, args.samples))
                del waveform[first + n_kept:]
            done = args.samples
        while done < args.samples:                  # in chunks, so that --save_every can write partial results
            n = min(args.samples - done, args.save_every or args.samples)
            if lc is not None:
                # row 0 belongs to the first generated sample, so this chunk's rf seed samples stand at done - rf .. done - 1
                # of the condition's time axis (in front of it they take row 0); only the chunk's own rows go to the device
                t0, H = done - rf, args.lc_hold
                r0, r1 = max(0, t0) // H, (done + n - 1) // H
                cond.update(local_conditions=lc[None, r0:r1 + 1], hold=H, t0=t0 - r0 * H)
            ids = net.generate(np.asarray(waveform[-rf:], np.int32), n, uniforms=rng.random((1, n)), **cond)
            if stop:                                # (one chunk) the generated samples in front of their end point
                n_kept = int(net.last_ends[0].item())
                print("End point at sample {} of {}".format(n_kept, n))
                ids = ids[:, :rf + n_kept]
            waveform.extend(int(x) for x in ids[0, rf:].cpu().numpy())
            done += n
            print("Sample {:3<d}/{:3<d}".format(done, args.samples), end="\r")
            if args.wav_out_path and args.save_every and done < args.samples:
                write_wav(mu_law_decode(np.asarray(waveform), q), SAMPLE_RATE, args.wav_out_path)
    else:
        for step in range(args.samples):
            window = waveform[-rf:] if len(waveform) > rf else waveform
            prediction = net.predict_proba(window, **cond1).double().cpu().numpy()
            scaled = scale_prediction(prediction, args.temperature)
            if args.temperature == 1.0:             # the reference's own check (:133-138)
                np.testing.assert_allclose(prediction, scaled, atol=1e-5,
                                           err_msg="Prediction scaling at temperature=1.0 is not working as intended.")
            waveform.append(int(rng.choice(np.arange(q), p=scaled / scaled.sum())))
            if (step + 1) % 100 == 0:
                print("Sample {:3<d}/{:3<d}".format(step + 1, args.samples), end="\r")
            if args.wav_out_path and args.save_every and (step + 1) % args.save_every == 0:
                write_wav(mu_law_decode(np.asarray(waveform), q), SAMPLE_RATE, args.wav_out_path)
    print()
    if args.wav_out_path:
        write_wav(mu_law_decode(np.asarray(waveform), q), SAMPLE_RATE, args.wav_out_path)
    print("Finished generating.")
    return waveform


if __name__ == "__main__":
    def _str_to_bool(s):
        if s.lower() not in ["true", "false"]:
            raise ValueError("Argument needs to be a boolean, got {}".format(s))
        return {"true": True, "false": False}[s.lower()]

    def _ensure_positive_float(f):
        if float(f) < 0:
            raise argparse.ArgumentTypeError("Argument must be greater than zero")
        return float(f)

    parser = argparse.ArgumentParser(description="WaveNet generation script")
    parser.add_argument("checkpoint", type=str, help="Which model checkpoint to generate from")
    parser.add_argument("--samples", type=int, default=SAMPLES)
    parser.add_argument("--temperature", type=_ensure_positive_float, default=TEMPERATURE)
    parser.add_argument("--logdir", type=str, default="./logdir")
    parser.add_argument("--wavenet_params", type=str, default=None, help="ignored: the network is wavenet.yaml's")
    parser.add_argument("--wav_out_path", type=str, default=None)
    parser.add_argument("--save_every", type=int, default=None)
    parser.add_argument("--fast_generation", type=_str_to_bool, default=True)
    parser.add_argument("--incremental_temperature", type=_str_to_bool, default=False,
                        help="keep the incremental generator at any --temperature (0 = argmax); needs --fast_generation true")
    parser.add_argument("--stop_at_endpoint", type=_str_to_bool, default=False,
                        help="stop drawing at the end point audio.find_endpoint would cut at; needs the incremental generator")
    parser.add_argument("--stream_chunk", type=int, default=None,
                        help="write --wav_out_path after every N samples of ONE resumed generation; needs the incremental generator")
    parser.add_argument("--wav_seed", type=str, default=None)
    parser.add_argument("--gc_channels", type=int, default=None)
    parser.add_argument("--gc_cardinality", type=int, default=None)
    parser.add_argument("--gc_id", type=int, default=None)
    parser.add_argument("--lc_channels", type=int, default=None)
    parser.add_argument("--local_condition", type=str, default=None, help="float [rows, lc_channels] .npy, row 0 at the first generated sample")
    parser.add_argument("--lc_hold", type=int, default=1, help="generated samples per row of --local_condition")
    parser.add_argument("--hparams", default="")
    parser.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    parser.add_argument("--seed", type=int, default=0)
    a = parser.parse_args()
    if a.gc_channels is not None:                   # generate_wavenet.py:221-231
        if a.gc_cardinality is None:
            raise ValueError("Globally conditioning but gc_cardinality not specified. Use --gc_cardinality=377 for full "
                             "VCTK corpus.")
        if a.gc_id is None:
            raise ValueError("Globally conditioning, but global condition was not specified. Use --gc_id to specify global "
                             "condition.")
    main(a)
