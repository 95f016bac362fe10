"""Synthesizer.synthesize_batch: every entry against the calls it is made of - one model pass on the padded texts, then
per row the single-clip functions (Griffin-Lim, inv_preemphasis, find_endpoint) or one batched WaveNet generate - bit
for bit, with synthesize itself left as it was.  Small Tacotron-2 widths, three decoder steps, no checkpoint."""
import numpy as np
import pytest

from test_wavenet_hold_gpu import TACO_SMALL, _hp

pytestmark = pytest.mark.gpu

TEXTS = ["Hello, World.", "Dr. Jones arrived at 9 o'clock.", "Yes."]


@pytest.fixture(scope="module")
def synth(dev):
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.synthesizer import Synthesizer
    hp = hparams_mod.load("taco2")
    for k, v in TACO_SMALL.items():
        setattr(hp, k, v)
    hparams_mod.set_hparams(hp)
    return Synthesizer(hp, dtype="bf16").load(None, "taco2")


def _current(synth):
    from nspeech_amd import hparams as hparams_mod
    hparams_mod.set_hparams(synth.hparams)


def _seqs(synth, texts):
    from nspeech_amd.utils.text import text_to_sequence
    names = [x.strip() for x in synth.hparams.cleaners.split(",")]
    return [text_to_sequence(t, names) for t in texts]


def test_griffin_lim_rows_are_the_single_clip_functions_on_the_padded_batch(synth):
    from nspeech_amd.synthesizer import pad_text_batch
    from nspeech_amd.utils import audio as A
    _current(synth)
    seqs = _seqs(synth, TEXTS)
    assert len(set(len(s) for s in seqs)) == 3
    before = synth.synthesize(TEXTS[0])
    got = synth.synthesize_batch(TEXTS)
    after = synth.synthesize(TEXTS[0])
    assert all(np.array_equal(a, b) for a, b in zip(before, after))          # the old path is untouched
    assert len(got) == 3 and all(len(g) == 3 for g in got)
    m = synth.model
    inputs, lengths = pad_text_batch(seqs)
    m.initialize(inputs, lengths, np.zeros(3, np.int32))
    mels, lins = m.mel_outputs.float().cpu().numpy(), m.linear_outputs.float().cpu().numpy()
    m.check_status()
    for i, (wav, mel, lin) in enumerate(got):
        assert mel.shape == before[1].shape and lin.shape == before[2].shape
        assert wav.dtype == before[0].dtype and mel.dtype == before[1].dtype and lin.dtype == before[2].dtype and wav.ndim == 1
        assert np.array_equal(mel, mels[i]) and np.array_equal(lin, lins[i]), i
        want = A.inv_preemphasis(A.inv_spectrogram_tensorflow(m.linear_outputs[i].contiguous()).cpu().numpy())
        want = want[:A.find_endpoint(want)]
        assert len(want) > 0 and np.isfinite(want).all()
        assert np.array_equal(wav, want), (i, len(wav), len(want))
    # a padded row is close to the text on its own, and not it: the entries differ between the rows at least
    assert not np.array_equal(got[0][1], got[1][1])
    # one speaker id per text is the same call
    again = synth.synthesize_batch(TEXTS, speaker_ids=[0, 0, 0])
    assert all(np.array_equal(a, b) for g, h in zip(got, again) for a, b in zip(g, h))


def test_wavenet_rows_are_one_batched_generate(synth):
    from nspeech_amd.models.wavenet import mu_law_decode, mu_law_encode
    from nspeech_amd.utils import audio as A
    small = dict(dilations_depth=1, dilations_length=4, residual_channels=32, dilation_channels=32, skip_channels=64,
                 quantization_channels=64)
    synth.load_vocoder(None, _hp(lc_channels=80, use_biases=True, **small))      # (leaves the synthesizer's hparams current)
    try:
        hp, v = synth.hparams, synth.vocoder
        T, hop = hp.max_iters * hp.outputs_per_step, 250
        assert T * hop < 5000
        got = synth.synthesize_batch(TEXTS, vocoder="wavenet", seed=5)
        mels = np.stack([g[1] for g in got])
        assert mels.shape == (3, T, 80)
        silence = int(mu_law_encode(np.zeros(1, np.float32), v.Q)[0])
        uniforms = np.stack([np.random.default_rng(5 + i).random(T * hop) for i in range(3)])
        ids = v.generate(np.full((3, v.rf), silence, np.int32), T * hop, uniforms=uniforms, local_conditions=mels, hold=hop,
                         t0=-v.rf)
        for i in range(3):
            want = mu_law_decode(ids[i, v.rf:].cpu().numpy(), v.Q)
            assert len(set(ids[i, v.rf:].cpu().numpy().tolist())) > 1
            want = want[:A.find_endpoint(want)]
            assert got[i][0].dtype == np.float32 and np.array_equal(got[i][0], want), i
        one = synth._wavenet_vocode(mels[0], seed=5)
        assert one.shape == (T * hop,) and np.array_equal(one, synth._wavenet_vocode_batch(mels[0][None], seed=5)[0])
    finally:
        synth.vocoder = None


def test_more_than_32_texts_run_as_chunks_in_order(synth):
    _current(synth)
    text = "Yes."
    got = synth.synthesize_batch([text] * 33)
    assert len(got) == 33
    alone = synth.synthesize_batch([text])[0]
    assert all(np.array_equal(a, b) for a, b in zip(got[32], alone))         # the 33rd is a chunk of one
