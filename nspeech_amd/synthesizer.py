"""Inference wrapper with the reference's surface (neural_speech/synthesizer.py:9-54):
Synthesizer(hparams).load(checkpoint_path, model_name); .synthesize(text, speaker_id) ->
(wav, mel[T,80], lin[T,1025]).  The waveform is Griffin-Lim of the linear output, then
inv_preemphasis and find_endpoint, exactly the reference's order (synthesizer.py:30,52-53).

load_vocoder(checkpoint_path, wavenet_hparams) + synthesize(text, vocoder="wavenet") vocode the mel output through a
WaveNet trained on mel local conditions (train_wavenet.py --hparams lc_channels=<num_mels>) instead: one mel row per hop
samples, a seed of receptive-field silence in front of row 0, T * hop samples drawn by the incremental generator."""
import numpy as np
import torch

from . import hparams as hparams_mod
from .models import create_model
from .utils import audio
from .utils.text import text_to_sequence


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

    def _wavenet_vocode(self, mel, seed=0, global_conditions=None):
        """mel float [T, num_mels] -> float32 [T * hop] in [-1, 1]: row r conditions samples r * hop .. r * hop + hop - 1;
        the seed - receptive-field copies of mu_law_encode(0) - stands at t0 = -rf and takes row 0.  No inv_preemphasis:
        the WaveNet feeder's waveforms are not pre-emphasised."""
        from .models.wavenet import mu_law_decode, mu_law_encode
        v, hop = self.vocoder, self._vocoder_hop
        silence = int(mu_law_encode(np.zeros(1, np.float32), v.Q)[0])
        ids = v.generate(np.full((1, v.rf), silence, np.int32), len(mel) * hop, seed=seed, global_conditions=global_conditions,
                         local_conditions=np.asarray(mel, np.float32)[None], hold=hop, t0=-v.rf)
        return mu_law_decode(ids[0, v.rf:].cpu().numpy(), v.Q)

    def synthesize(self, text, speaker_id=0, vocoder="griffin_lim", seed=0):
        """vocoder="wavenet" (after load_vocoder): the mel output through the WaveNet; seed: of the draws' random stream
        (generate(seed=)), unused by Griffin-Lim."""
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
        if vocoder == "wavenet":
            mel = m.mel_outputs[0].float().cpu().numpy()
            lin = m.linear_outputs[0].float().cpu().numpy()
            m.check_status()    # (as below: invalid outputs are never vocoded)
            gc = np.asarray([speaker_id]) if self.vocoder.gc else None
            wav = self._wavenet_vocode(mel, seed=seed, global_conditions=gc)
            return wav[:audio.find_endpoint(wav)], mel, lin
        wav = audio.inv_spectrogram_tensorflow(m.linear_outputs[0].contiguous())
        mel = m.mel_outputs[0].float().cpu().numpy()
        lin = m.linear_outputs[0].float().cpu().numpy()
        m.check_status()        # after the host copies (stream synchronised): a persistent BiLSTM kernel that gave up
                                # on an exchange leaves invalid outputs behind - never vocode those silently
        wav = audio.inv_preemphasis(wav.cpu().numpy())
        wav = wav[:audio.find_endpoint(wav)]
        return wav, mel, lin
