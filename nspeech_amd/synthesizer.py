"""Inference wrapper with the reference's surface (neural_speech/synthesizer.py:9-54):
Synthesizer(hparams).load(checkpoint_path, model_name); .synthesize(text, speaker_id) ->
(wav, mel[T,80], lin[T,1025]).  The waveform is Griffin-Lim of the linear output, then
inv_preemphasis and find_endpoint, exactly the reference's order (synthesizer.py:30,52-53).

load_vocoder(checkpoint_path, wavenet_hparams) + synthesize(text, vocoder="wavenet") vocode the mel output through a
WaveNet trained on mel local conditions (train_wavenet.py --hparams lc_channels=<num_mels>) instead: one mel row per hop
samples, a seed of receptive-field silence in front of row 0, T * hop samples drawn by the incremental generator.

synthesize_batch(texts, speaker_ids) is the same for many texts: one model pass per 32 of them, one Griffin-Lim call
(or one WaveNet generate) per pass and one audio.finish_waves for the inv_preemphasis / find_endpoint tail.

With hparam stop_token (Tacotron-2) the model also says at which decoder step each utterance stops
(model.output_lengths()); synthesize / synthesize_stream / synthesize_batch then cut mel and lin there and hand the
vocoder the cut arrays (use_stop_token=True, the default; False or a model without a stop token: the path as it was)."""
import numpy as np
import torch

from . import hparams as hparams_mod
from .models import create_model
from .utils import audio
from .utils.text import text_to_sequence


MAX_BATCH = 32      # texts per model pass: the rows one packed decode step takes (ns_rows32)


def pad_text_batch(seqs):
    """Symbol-id sequences of different lengths -> (inputs int32 [N, T_max] padded with id 0 as the feeder's _pad does,
    lengths int32 [N])."""
    lengths = np.asarray([len(s) for s in seqs], dtype=np.int32)
    inputs = np.zeros((len(seqs), int(lengths.max()) if len(seqs) else 0), dtype=np.int32)
    for i, s in enumerate(seqs):
        inputs[i, :len(s)] = np.asarray(s, dtype=np.int32)
    return inputs, lengths


def batch_chunks(n, size=MAX_BATCH):
    """[(start, stop)] of the consecutive chunks of at most `size` that cover range(n), in order."""
    return [(s, min(n, s + size)) for s in range(0, n, size)]


class SynthesisStream(object):
    """What Synthesizer.synthesize_stream returns: .mel [T, num_mels] and .lin [T, num_freq] of the text, and an iteration
    over float32 pieces of its waveform: mu_law_decode of the vocoder's generate_stream `codes` at B = 1.  rule:
    generate's endpoint triple - then a piece ends at safe_prefix of the samples drawn so far, the last one at the end
    point - or None for the uncut waveform."""

    def __init__(self, vocoder, codes, mel, lin, rule):
        from .models.wavenet import endpoint_code
        self.vocoder, self.codes, self.mel, self.lin, self.rule = vocoder, codes, mel, lin, rule
        self.below = endpoint_code(vocoder.Q, rule[2]) if rule is not None else None
        self._drawn = np.zeros(codes.total - codes.n_seed, np.int32)      # every code drawn so far
        self._out, self._done = 0, False                                  # samples handed out; the last piece is out

    def __iter__(self):
        return self

    def __next__(self):
        from .models.wavenet import mu_law_decode, safe_prefix
        while not self._done:
            piece = next(self.codes, None)
            if self.rule is None:
                if piece is None:
                    break
                return mu_law_decode(piece[0], self.vocoder.Q)
            drawn = self.codes.drawn
            if piece is not None:
                self._drawn[drawn - piece.shape[1]:drawn] = piece[0]
            if piece is None or self.codes.fired[0]:       # all drawn, or the rule fired in this chunk: up to the end point
                self._done = True
                upto = int(self.codes.ends[0])
            else:
                window, hop = int(self.rule[0]), int(self.rule[1])
                upto = safe_prefix(self._drawn[max(0, drawn - (window - hop)):drawn], drawn, self.below, window, hop)
            if upto > self._out:
                out = mu_law_decode(self._drawn[self._out:upto], self.vocoder.Q)
                self._out = upto
                return out
        raise StopIteration


class Synthesizer(object):
    def __init__(self, hparams, dtype="mixed", device="cuda:0"):
        self.hparams = hparams
        self.dtype = dtype
        self.device = device
        self.model = None
        self.vocoder = None

    def load(self, checkpoint_path, model_name="taco2"):
        print("Constructing model: %s" % model_name)
        hparams_mod.set_hparams(self.hparams)
        self.model = create_model(model_name, self.hparams, device=self.device, dtype=self.dtype)
        if checkpoint_path is not None:
            print("Loading checkpoint: %s" % checkpoint_path)
            from .utils import tf_bundle
            if tf_bundle.is_bundle(checkpoint_path):       # a TensorFlow checkpoint prefix (model.ckpt-N.index + data)
                tf_bundle.load_into_model(self.model, checkpoint_path)
            else:
                self.model.load_state_dict(torch.load(checkpoint_path, map_location="cpu", weights_only=True))
        return self

    def load_vocoder(self, checkpoint_path, hparams, dtype="bf16"):
        """A WaveNetModel with lc_channels = num_mels as the vocoder of synthesize(vocoder="wavenet"): `hparams` is the
        WaveNet's set (hparams.load("wavenet") + what it was trained with), checkpoint_path a model.ckpt-<step> of
        train_wavenet.py (None: the initial weights), dtype the WaveNet's compute mode.  Its local condition must be this
        synthesizer's mel: the same channel count, sample rate and hop, else ValueError.
        Leaves the synthesizer's own hparams as the current set (hparams.set_hparams): loading the WaveNet's set with
        hparams.load("wavenet") made THAT the current one, and the audio code reads the current set."""
        hp, mine = hparams, self.hparams
        hop = lambda h: int(h.frame_shift_ms / 1000 * h.sample_rate)      # utils/audio.py:_stft_parameters
        if int(hp.lc_channels or 0) != int(mine.num_mels):
            raise ValueError("vocoder lc_channels = %s, the synthesizer's mel has num_mels = %d channels"
                             % (hp.lc_channels, mine.num_mels))
        if int(hp.sample_rate) != int(mine.sample_rate):
            raise ValueError("vocoder sample_rate %s != %s" % (hp.sample_rate, mine.sample_rate))
        if hop(hp) != hop(mine):
            raise ValueError("vocoder hop %d samples != %d" % (hop(hp), hop(mine)))
        if hp.scalar_input:
            raise ValueError("a scalar_input WaveNet has no incremental generator")
        v = create_model("wavenet", hp, device=self.device, dtype=dtype)
        if checkpoint_path is not None:
            print("Loading vocoder checkpoint: %s" % checkpoint_path)
            v.load_state_dict(torch.load(checkpoint_path, map_location="cpu", weights_only=True))
        self.vocoder, self._vocoder_hop = v, hop(mine)
        hparams_mod.set_hparams(mine)
        return self

    def _wavenet_vocode_batch(self, mels, seed=0, global_conditions=None, temperature=1.0, endpoint=False):
        """mels float [B, T, num_mels] -> float32 [B, T * hop] in [-1, 1], ONE generate call: row r of a mel conditions
        samples r * hop .. r * hop + hop - 1; the seed - receptive-field copies of mu_law_encode(0) - stands at t0 = -rf
        and takes row 0.  Waveform i draws from np.random.default_rng(seed + i).random(T * hop), so B = 1 is the stream
        generate(seed=seed) draws itself.  temperature: generate's - softmax(logits / temperature) draws, 0 = argmax (then
        the uniforms have no effect).  No inv_preemphasis: the WaveNet feeder's waveforms are not pre-emphasised.
        endpoint=True: the generator stops every waveform at its end point (generate(endpoint=audio.endpoint_rule())) and
        the call returns (waves, ends) - waves a list of B float32 arrays, waves[i] the ends[i] samples in front of
        waveform i's end point, equal to full[i, :audio.find_endpoint(full[i])] of the call without it; only what was
        drawn is copied to the host and decoded."""
        from .models.wavenet import mu_law_decode
        v = self.vocoder
        seed_ids, n, kw = self._wavenet_vocode_args(mels, seed, global_conditions, temperature, endpoint)
        B = len(seed_ids)
        ids = v.generate(seed_ids, n, **kw)
        if not endpoint:
            return mu_law_decode(ids[:, v.rf:].cpu().numpy(), v.Q)
        ends = [int(e) for e in v.last_ends.cpu().numpy()]
        return [mu_law_decode(ids[i, v.rf:v.rf + ends[i]].cpu().numpy(), v.Q) for i in range(B)], ends

    def _wavenet_vocode_args(self, mels, seed, global_conditions, temperature, endpoint):
        """(seed_ids, n_samples, keywords) of the vocoder's generate / generate_stream for mels float [B, T, num_mels]:
        _wavenet_vocode_batch's seed silence, uniforms and conditions."""
        from .models.wavenet import mu_law_encode
        v, hop = self.vocoder, self._vocoder_hop
        mels = np.asarray(mels, np.float32)
        B, n = mels.shape[0], mels.shape[1] * hop
        silence = int(mu_law_encode(np.zeros(1, np.float32), v.Q)[0])
        uniforms = np.stack([np.random.default_rng(seed + i).random(n) for i in range(B)])
        return np.full((B, v.rf), silence, np.int32), n, dict(
            uniforms=uniforms, global_conditions=global_conditions, local_conditions=mels, hold=hop, t0=-v.rf,
            temperature=temperature, endpoint=audio.endpoint_rule() if endpoint else None)

    def _wavenet_vocode(self, mel, seed=0, global_conditions=None, temperature=1.0):
        """mel float [T, num_mels] -> float32 [T * hop]: _wavenet_vocode_batch of the one mel."""
        return self._wavenet_vocode_batch(np.asarray(mel, np.float32)[None], seed=seed, global_conditions=global_conditions,
                                          temperature=temperature)[0]

    def _stop_frames(self, use_stop_token):
        """Frames per row up to and including its stop step (model.output_lengths(), one host read), or None: the model
        has no stop token, or the caller does not want it used - then nothing is cut."""
        m = self.model
        if not (use_stop_token and getattr(m, "stop_token", False)):
            return None
        return m.output_lengths()

    def synthesize(self, text, speaker_id=0, vocoder="griffin_lim", seed=0, temperature=1.0, stop_at_endpoint=True,
                   use_stop_token=True):
        """use_stop_token (models with hparam stop_token only): mel and lin are cut to model.output_lengths()[0] frames
        and the vocoder receives the cut arrays; inv_preemphasis and find_endpoint still run behind it and can only cut
        further.  False, or a model without a stop token: all max_iters * outputs_per_step frames, as ever.
        vocoder="wavenet" (after load_vocoder): the mel output through the WaveNet; seed: of the draws' random stream
        (generate(seed=)); temperature: of the draws (generate(temperature=): below 1 trades hiss for muffling, 0 is the
        deterministic argmax vocode); stop_at_endpoint: the generator applies find_endpoint's rule to its own output and
        stops drawing at the end of the first silent window, instead of drawing all T * hop samples and cutting on the
        host (False) - the same array, bit for bit.  All three unused by Griffin-Lim."""
        if vocoder not in ("griffin_lim", "wavenet"):
            raise ValueError("vocoder %r: 'griffin_lim' or 'wavenet'" % (vocoder,))
        if vocoder == "wavenet" and self.vocoder is None:
            raise ValueError("vocoder='wavenet' needs load_vocoder(checkpoint_path, hparams) first")
        cleaner_names = [x.strip() for x in self.hparams.cleaners.split(",")]
        seq = text_to_sequence(text, cleaner_names)
        inputs = np.asarray([seq], dtype=np.int32)
        lengths = np.asarray([len(seq)], dtype=np.int32)
        m = self.model
        m.initialize(inputs, lengths, np.asarray([speaker_id], dtype=np.int32))
        frames = self._stop_frames(use_stop_token)
        keep = slice(None) if frames is None else slice(0, int(frames[0]))
        if vocoder == "wavenet":
            mel = m.mel_outputs[0].float().cpu().numpy()[keep]
            lin = m.linear_outputs[0].float().cpu().numpy()[keep]
            m.check_status()    # (as below: invalid outputs are never vocoded)
            gc = np.asarray([speaker_id]) if self.vocoder.gc else None
            if stop_at_endpoint:
                wavs, _ = self._wavenet_vocode_batch(mel[None], seed=seed, global_conditions=gc, temperature=temperature,
                                                     endpoint=True)
                return wavs[0], mel, lin
            wav = self._wavenet_vocode(mel, seed=seed, global_conditions=gc, temperature=temperature)
            return wav[:audio.find_endpoint(wav)], mel, lin
        wav = audio.inv_spectrogram_tensorflow(m.linear_outputs[0][keep].contiguous())
        mel = m.mel_outputs[0].float().cpu().numpy()[keep]
        lin = m.linear_outputs[0].float().cpu().numpy()[keep]
        m.check_status()        # after the host copies (stream synchronised): a persistent BiLSTM kernel that gave up
                                # on an exchange leaves invalid outputs behind - never vocode those silently
        wav = audio.inv_preemphasis(wav.cpu().numpy())
        wav = wav[:audio.find_endpoint(wav)]
        return wav, mel, lin

    def synthesize_stream(self, text, speaker_id=0, chunk_samples=None, seed=0, temperature=1.0, stop_at_endpoint=True,
                          use_stop_token=True):
        """synthesize(text, vocoder="wavenet") heard while it is drawn (after load_vocoder; the same refusals;
        use_stop_token: synthesize's - the vocoder draws only the frames up to the stop step).  The
        Tacotron pass and check_status() run before this returns; the result is an iterable (SynthesisStream) with .mel
        and .lin set, whose iteration yields float32 pieces of the waveform, one per chunk_samples drawn samples (None:
        20 hops) - the vocoder's generate_stream, so the generator is never restarted and keeps drawing while a piece
        is consumed.  seed, temperature: synthesize's.
        stop_at_endpoint=True: a step hands out only what audio.find_endpoint can no longer cut (safe_prefix of the
        samples drawn so far - up to window - hop trailing silent samples are held back, and a step with nothing safe
        yields nothing), the last step hands out the rest up to the end point, and the generator stops drawing there:
        np.concatenate(list(stream)) is synthesize(text, vocoder="wavenet", same arguments)[0] bit for bit.
        False: all T * hop samples are yielded as they are drawn, UNCUT - find_endpoint is not applied at all, since
        what it would cut has been handed out by then."""
        if self.vocoder is None:
            raise ValueError("vocoder='wavenet' needs load_vocoder(checkpoint_path, hparams) first")
        cleaner_names = [x.strip() for x in self.hparams.cleaners.split(",")]
        seq = text_to_sequence(text, cleaner_names)
        m = self.model
        m.initialize(np.asarray([seq], dtype=np.int32), np.asarray([len(seq)], dtype=np.int32),
                     np.asarray([speaker_id], dtype=np.int32))
        frames = self._stop_frames(use_stop_token)
        keep = slice(None) if frames is None else slice(0, int(frames[0]))
        mel = m.mel_outputs[0].float().cpu().numpy()[keep]
        lin = m.linear_outputs[0].float().cpu().numpy()[keep]
        m.check_status()        # (as in synthesize: invalid outputs are never vocoded)
        gc = np.asarray([speaker_id]) if self.vocoder.gc else None
        seed_ids, n, kw = self._wavenet_vocode_args(mel[None], seed, gc, temperature, bool(stop_at_endpoint))
        chunk = 20 * self._vocoder_hop if chunk_samples is None else int(chunk_samples)
        return SynthesisStream(self.vocoder, self.vocoder.generate_stream(seed_ids, n, chunk, **kw), mel, lin, kw["endpoint"])

    def synthesize_batch(self, texts, speaker_ids=0, vocoder="griffin_lim", seed=0, temperature=1.0, stop_at_endpoint=True,
                         use_stop_token=True):
        """synthesize for a list of texts: [(wav, mel, lin)] in the order of `texts`, every entry with the shapes and
        dtypes synthesize returns.  speaker_ids: one int for all, or one id per text.  More than MAX_BATCH texts run as
        consecutive chunks of at most MAX_BATCH in the given order (never sorted: see below); [] returns [].
        Per chunk: ONE model pass on the padded texts, then
          griffin_lim: one griffin_lim_gpu on linear_outputs [N, T, F], one audio.finish_waves (inv_preemphasis and
            find_endpoint of all N on the device), one copy to the host each of the waves, the ends, the mels and the
            linears, check_status() behind them as in synthesize, wav[i] = y[i, :ends[i]];
          wavenet: one generate for the chunk, text i of the LIST drawing from np.random.default_rng(seed + i) at
            `temperature` (generate(temperature=), 0 = argmax; unused by Griffin-Lim), every waveform stopped at its
            end point by the generator itself (stop_at_endpoint, as in synthesize; False: all T * hop samples drawn
            and find_endpoint per row on the host - the same arrays); mu-law decoding on the host, no pre-emphasis.
        Row i is the row of a PADDED batch: the encoder's convolutions read the padding behind a shorter text, as the
        reference's graph would, and other kernels run at N > 2 than at N = 1 (model.last_paths["decode"]).  So entry i
        is close to synthesize(texts[i]), not bit-equal to it - and depends on which texts share its chunk.  The WaveNet
        rows of different batch sizes are not promised bit-equal either: the condition products are dispatched by
        shape.
        use_stop_token (models with hparam stop_token only; False: the path above, bit for bit): still one model pass per
        chunk; entry i's mel / lin are cut to its own length model.output_lengths()[i]; the vocoder runs once on the
        chunk cut to its longest row, and wave i is cut to min(ends[i], the vocoder's length for row i's frame count):
        audio.griffin_lim_length(frames) for Griffin-Lim, frames * hop for the WaveNet.  The WaveNet's generate offers
        nothing for rows of unequal length (its local conditions are one [B, T, C] array), so it draws every row to the
        longest row's length - or to its end point - and the cut happens here."""
        if vocoder not in ("griffin_lim", "wavenet"):
            raise ValueError("vocoder %r: 'griffin_lim' or 'wavenet'" % (vocoder,))
        texts = list(texts)
        if np.ndim(speaker_ids) == 0:
            speakers = np.full(len(texts), int(speaker_ids), dtype=np.int32)
        else:
            speakers = np.asarray(speaker_ids, dtype=np.int32).reshape(-1)
            if len(speakers) != len(texts):
                raise ValueError("%d speaker_ids for %d texts" % (len(speakers), len(texts)))
        if not texts:
            return []
        if vocoder == "wavenet" and self.vocoder is None:
            raise ValueError("vocoder='wavenet' needs load_vocoder(checkpoint_path, hparams) first")
        cleaner_names = [x.strip() for x in self.hparams.cleaners.split(",")]
        seqs = [text_to_sequence(t, cleaner_names) for t in texts]
        m = self.model
        out = []
        for start, stop in batch_chunks(len(seqs)):
            inputs, lengths = pad_text_batch(seqs[start:stop])
            spk = speakers[start:stop]
            m.initialize(inputs, lengths, spk)
            frames = self._stop_frames(use_stop_token)
            keep = slice(None) if frames is None else slice(0, int(frames.max()))
            if vocoder == "wavenet":
                mels = m.mel_outputs.float().cpu().numpy()[:, keep]
                lins = m.linear_outputs.float().cpu().numpy()[:, keep]
                m.check_status()            # (as in synthesize: invalid outputs are never vocoded)
                full = self._wavenet_vocode_batch(mels, seed=seed + start, global_conditions=spk if self.vocoder.gc else None,
                                                  temperature=temperature, endpoint=bool(stop_at_endpoint))
                wavs = full[0] if stop_at_endpoint else [w[:audio.find_endpoint(w)] for w in full]
                limit = None if frames is None else frames * self._vocoder_hop
            else:
                y, ends = audio.finish_waves(audio.griffin_lim_gpu(m.linear_outputs[:, keep]))
                y, ends = y.cpu().numpy(), ends.cpu().numpy()
                mels = m.mel_outputs.float().cpu().numpy()[:, keep]
                lins = m.linear_outputs.float().cpu().numpy()[:, keep]
                m.check_status()            # after the host copies, before anything is handed out
                wavs = [y[i, :int(ends[i])] for i in range(stop - start)]
                limit = None if frames is None else [audio.griffin_lim_length(int(f)) for f in frames]
            if frames is None:
                out.extend((wavs[i], mels[i], lins[i]) for i in range(stop - start))
            else:
                out.extend((wavs[i][:int(limit[i])], mels[i, :int(frames[i])], lins[i, :int(frames[i])])
                           for i in range(stop - start))
        return out
