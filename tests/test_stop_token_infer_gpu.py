"""The stop token at synthesis (hparams stop_token, stop_threshold): one ns_stop_token launch on the h2 history of whichever
decode path ran, inside the captured graph; model.stop_logits / stop_steps / decoder_h2 / output_lengths(); the
Synthesizer cutting mel, lin and the vocoder's input there; checkpoints with and without the stop variables."""
import numpy as np
import pytest
import torch

import stop_token_ref as R
from util import make_batch, small_hparams

pytestmark = pytest.mark.gpu

STOP = ("decoder/stop_projection/kernel", "decoder/stop_projection/bias")
U = 2.0 ** -24


def _model(hp, dtype="fp32", seed=3):
    from nspeech_amd.models import create_model
    return create_model("taco2", hp, device="cuda:0", dtype=dtype, seed=seed)


def _set_stop(m, kernel, bias):
    pv = m.numpy_params()
    pv[STOP[0]] = np.asarray(kernel, np.float32).reshape(-1, 1)
    pv[STOP[1]] = np.asarray([bias], np.float32)
    m.load_numpy(pv, m.numpy_stats())


def _z_bound(h, w, b):
    D = h.shape[-1]
    g = (D + 2) * U / (1.0 - (D + 2) * U)
    return g * (np.abs(h * w).sum(axis=-1) + abs(b))


def _expected(m, thr):
    """Float64 stop steps from the history the kernel read (m.decoder_h2) and the model's stop variables - after the
    margin rule of tests/test_stop_token_contract_gpu.py: no logit up to and including a row's first crossing lies within
    100 rounding bounds of the threshold."""
    h = m.decoder_h2.float().cpu().numpy().astype(np.float64)
    pv = m.numpy_params()
    w, b = pv[STOP[0]].astype(np.float64).reshape(-1), float(pv[STOP[1]][0])
    z = h @ w + b
    want = R.stop_steps(z, thr)
    ez = _z_bound(h, w, b)
    for n in range(z.shape[0]):
        upto = int(want[n])
        gap = np.abs(z[n, :upto] - thr) / ez[n, :upto]
        assert gap.min() > 100.0, "row %d: a deciding logit lies within %.1f bounds of the threshold" % (n, gap.min())
    return z, want


def _pick_stop_variables(h, thr=0.0, tries=50):
    """A random kernel, scaled, and a bias such that the rows of h [N, S, D] stop at different steps (one row: somewhere
    inside (1, S)), with the margin rule kept a thousandfold.  Only the history decides - it does not depend on the stop
    variables - so a test may run one pass, choose, load and run again."""
    h = np.asarray(h, np.float64)
    N, S, D = h.shape
    for seed in range(tries):
        rng = np.random.RandomState(1000 + seed)
        w = rng.standard_normal(D)
        z0 = h @ w
        w *= 4.0 / max(z0.std(), 1e-30)                 # logits of a few units
        z0 = h @ w
        b = thr - float(np.quantile(z0, 0.75))          # a quarter of the steps over the threshold
        w32, b32 = w.astype(np.float32), float(np.float32(b))
        z = h @ w32.astype(np.float64) + b32
        want = R.stop_steps(z, thr)
        ok = len(set(want.tolist())) >= min(N, 2) and (N > 1 or 1 < want[0] < S)
        ok = ok and all((np.abs(z[n, :want[n]] - thr) / _z_bound(h[n, :want[n]], w32.astype(np.float64), b32)).min() > 1000.0
                        for n in range(N))
        if ok:
            return w32, b32, want
    raise AssertionError("no stop kernel within %d seeds" % tries)


def test_bias_decides_when_the_kernel_is_zero(dev):
    hp_on, hp_off = small_hparams(max_iters=8, stop_token=True), small_hparams(max_iters=8)
    on, off = _model(hp_on), _model(hp_off)
    p_on, p_off = on.numpy_params(), off.numpy_params()
    assert all(np.array_equal(p_on[k], p_off[k]) for k in p_off)
    inputs, lengths, _, _ = make_batch(hp_on, 2, 12, 10, seed=4)
    D = hp_on.decoder_lstm_units
    _set_stop(on, np.zeros(D), -10.0)
    on.initialize(inputs, lengths)
    off.initialize(inputs, lengths)
    on.check_status()
    assert on.last_paths["decode"] == off.last_paths["decode"] == "persistent"
    assert on.stop_steps.dtype == torch.int32 and on.stop_steps.cpu().tolist() == [8, 8]
    assert tuple(on.stop_logits.shape) == (2, 8) and tuple(on.decoder_h2.shape) == (2, 8, D)
    assert torch.equal(on.stop_logits.cpu(), torch.full((2, 8), -10.0))
    assert on.output_lengths().tolist() == [8 * hp_on.outputs_per_step] * 2
    for name in ("mel_outputs", "linear_outputs", "alignments"):
        assert torch.equal(getattr(on, name), getattr(off, name)), name
    assert off.stop_steps is None and off.stop_logits is None and off.decoder_h2 is None
    with pytest.raises(ValueError, match="stop_token"):
        off.output_lengths()
    _set_stop(on, np.zeros(D), 10.0)
    on.use_graph = False
    on.initialize(inputs, lengths)
    assert on.stop_steps.cpu().tolist() == [1, 1]
    assert on.output_lengths().tolist() == [hp_on.outputs_per_step] * 2


@pytest.mark.parametrize("N, path, dtype", [(2, "persistent", "mixed"), (3, "rows32", "mixed"), (2, "step", "mixed"),
                                            (3, "step", "fp32"), (3, "step", "bf16")])
def test_random_kernel_on_every_decode_path(dev, N, path, dtype):
    """Eager, capture + replay, replay, replay with new inputs (the loop of test_inference_graph_replay_matches_eager):
    the stop steps are the float64 ones of the history each path kept, and the graph's are the eager model's."""
    thr_p = 0.4
    thr = R.threshold_logit(thr_p)
    hp = small_hparams(max_iters=8, stop_token=True, stop_threshold=thr_p)
    m, e = _model(hp, dtype), _model(hp, dtype)
    e.use_graph = False
    for x in (m, e):
        if path == "step":
            x.use_decode_kernel = False
            x.use_rows32 = False
    inputs, lengths, _, _ = make_batch(hp, N, 11, 10, seed=1)
    e.initialize(inputs, lengths)               # the history does not depend on the stop variables: choose them from it
    w, b, _ = _pick_stop_variables(e.decoder_h2.float().cpu().numpy(), thr)
    _set_stop(m, w, b)
    _set_stop(e, w, b)
    e._infer_graph = None
    seen = set()
    for seed in (1, 2, 3, 4):
        inputs, lengths, _, _ = make_batch(hp, N, 11, 10, seed=seed)
        m.initialize(inputs, lengths)
        e.initialize(inputs, lengths)
        assert (m._infer_graph["graph"] is not None) == (seed > 1)
        assert m.last_paths["decode"] == path
        z, want = _expected(m, float(np.float32(thr)))
        got = m.stop_steps.cpu().numpy()
        print("%s N=%d seed %d: stop steps %s" % (path, N, seed, got.tolist()))
        assert got.tolist() == want.tolist()
        assert m.decoder_h2.dtype == (torch.bfloat16 if (dtype == "bf16" and path == "step") else torch.float32)
        assert np.abs(m.stop_logits.cpu().numpy() - z).max() <= 1e-4 * max(1.0, np.abs(z).max())
        assert m.output_lengths().tolist() == (want * hp.outputs_per_step).tolist()
        assert torch.equal(m.stop_steps, e.stop_steps) and torch.equal(m.stop_logits, e.stop_logits)
        seen.update(got.tolist())
    assert len(seen) >= 2


@pytest.fixture(scope="module")
def synth(dev):
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.synthesizer import Synthesizer
    hp = small_hparams(max_iters=8, num_freq=1025, num_mels=80, stop_token=True)
    hparams_mod.set_hparams(hp)
    return Synthesizer(hp, dtype="bf16").load(None, "taco2")


def _current(synth):
    from nspeech_amd import hparams as hparams_mod
    hparams_mod.set_hparams(synth.hparams)


def test_synthesize_cuts_at_the_stop_step(dev, synth):
    from nspeech_amd.utils import audio
    _current(synth)
    hp, m = synth.hparams, synth.model
    T = 8 * hp.outputs_per_step
    text = "Hello, World."
    wav0, mel0, lin0 = synth.synthesize(text, use_stop_token=False)
    assert mel0.shape == (T, 80) and lin0.shape == (T, 1025)
    w, b, want = _pick_stop_variables(m.decoder_h2.float().cpu().numpy())
    _set_stop(m, w, b)
    wav, mel, lin = synth.synthesize(text)
    frames = int(m.output_lengths()[0])
    assert frames == int(want[0]) * hp.outputs_per_step and hp.outputs_per_step < frames < T
    assert mel.shape == (frames, 80) and lin.shape == (frames, 1025)
    assert np.array_equal(mel, mel0[:frames]) and np.array_equal(lin, lin0[:frames])
    assert wav.ndim == 1 and 0 < len(wav) <= audio.griffin_lim_length(frames) and np.isfinite(wav).all()
    assert audio.griffin_lim_length(frames) == (frames - 1) * 250 + 1000
    # the switch of the call: today's shapes, and today's arrays
    wav1, mel1, lin1 = synth.synthesize(text, use_stop_token=False)
    assert mel1.shape == (T, 80) and lin1.shape == (T, 1025)
    assert np.array_equal(mel1, mel0) and np.array_equal(lin1, lin0) and np.array_equal(wav1, wav0)


def test_synthesize_batch_cuts_every_row_at_its_own_step(dev, synth):
    from nspeech_amd.utils import audio
    _current(synth)
    hp, m = synth.hparams, synth.model
    r, T = hp.outputs_per_step, 8 * hp.outputs_per_step
    texts = ["Hello, World.", "A much longer sentence than the first one.", "Short."]
    full = synth.synthesize_batch(texts, use_stop_token=False)
    assert [x[1].shape for x in full] == [(T, 80)] * 3
    w, b, want = _pick_stop_variables(m.decoder_h2.float().cpu().numpy())
    assert len(set(want.tolist())) >= 2
    _set_stop(m, w, b)
    out = synth.synthesize_batch(texts)
    lens = m.output_lengths()
    assert lens.tolist() == (want * r).tolist()
    for i, (wav, mel, lin) in enumerate(out):
        assert mel.shape == (lens[i], 80) and lin.shape == (lens[i], 1025)
        assert np.array_equal(mel, full[i][1][:lens[i]]) and np.array_equal(lin, full[i][2][:lens[i]])
        assert wav.ndim == 1 and 0 < len(wav) <= audio.griffin_lim_length(int(lens[i])) and np.isfinite(wav).all()
    again = synth.synthesize_batch(texts, use_stop_token=False)
    for a, f in zip(again, full):
        assert all(np.array_equal(x, y) for x, y in zip(a, f))


def _train_two_steps(m, hp):
    batch = make_batch(hp, 3, 11, 20, seed=5)
    m.add_optimizer(global_step=0)
    for _ in range(2):
        m.step(*batch, target_lengths=np.asarray([20, 12, 3]))


def test_state_dict_round_trip_keeps_the_stop_variables(dev, capsys):
    hp = small_hparams(stop_token=True)
    a, b = _model(hp, seed=3), _model(hp, seed=8)
    _train_two_steps(a, hp)
    sd = a.state_dict()
    assert all("model/inference/" + k in sd for k in STOP)
    capsys.readouterr()
    b.load_state_dict(sd)
    assert "stop" not in capsys.readouterr().out
    pa, pb = a.numpy_params(), b.numpy_params()
    assert all(np.array_equal(pa[k], pb[k]) for k in pa)
    (ma, va), (mb, vb) = a.numpy_adam_slots(), b.numpy_adam_slots()
    assert all(np.array_equal(ma[k], mb[k]) and np.array_equal(va[k], vb[k]) for k in ma)
    assert np.abs(ma[STOP[0]]).max() > 0.0 and np.abs(va[STOP[1]]).max() > 0.0 and b.global_step == 2


def test_checkpoints_across_the_switch(dev, capsys):
    hp_on, hp_off = small_hparams(stop_token=True), small_hparams()
    off = _model(hp_off, seed=3)
    _train_two_steps(off, hp_off)
    old = off.state_dict()              # what a checkpoint from before the switch holds
    assert not [k for k in old if "stop_projection" in k]
    on = _model(hp_on, seed=8)
    init = on.numpy_params()
    capsys.readouterr()
    on.load_state_dict(old)
    said = capsys.readouterr().out
    assert said.count("\n") == 1 and "no stop-token variables" in said
    p_on, p_off = on.numpy_params(), off.numpy_params()
    assert all(np.array_equal(p_on[k], p_off[k]) for k in p_off)
    assert all(np.array_equal(p_on[k], init[k]) for k in STOP)
    (m_on, v_on), (m_off, v_off) = on.numpy_adam_slots(), off.numpy_adam_slots()
    assert all(np.array_equal(m_on[k], m_off[k]) and np.array_equal(v_on[k], v_off[k]) for k in m_off)
    assert np.abs(m_off["dense/kernel"]).max() > 0.0            # a variable behind the new ones: its moments moved along
    assert all(not m_on[k].any() and not v_on[k].any() for k in STOP)
    assert on.global_step == 2 and np.array_equal(on.numpy_stats()["encoder/conv_0/batch_normalization/moving_mean"],
                                                   off.numpy_stats()["encoder/conv_0/batch_normalization/moving_mean"])
    # it trains on from there
    _train_two_steps(on, hp_on)
    assert np.isfinite(on.loss) and on.stop_loss > 0.0
    # the opposite direction: the stop variables are ignored, one line says so
    new = on.state_dict()
    back = _model(hp_off, seed=9)
    capsys.readouterr()
    back.load_state_dict(new)
    said = capsys.readouterr().out
    assert said.count("\n") == 1 and "ignored" in said
    p_back, p_new = back.numpy_params(), on.numpy_params()
    assert all(np.array_equal(p_back[k], p_new[k]) for k in p_back)
    (m_b, v_b), (m_n, v_n) = back.numpy_adam_slots(), on.numpy_adam_slots()
    assert all(np.array_equal(m_b[k], m_n[k]) and np.array_equal(v_b[k], v_n[k]) for k in m_b)


def test_tacotron1_refuses_the_switch(dev):
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.models import create_model
    hp = hparams_mod.load("taco1")
    hp.stop_token = True
    with pytest.raises(ValueError, match="only the Tacotron-2 model"):
        create_model("taco1", hp, device="cuda:0", dtype="fp32")
