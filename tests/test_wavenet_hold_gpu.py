"""Frame-rate ("held") local conditions in WaveNet training: ns_wavenet_hold_sum against a float64 sum, the model with
initialize(hold=, t0=) against oracle/wavenet_oracle.py: loss_full on the condition expanded per sample, training and
generation reading the same row for the same (hold, t0), the bf16 mode beside the per-sample form, the refusals, and
Synthesizer.synthesize(vocoder="wavenet").

Position m of item n reads condition row max(0, m + t0[n]) // hold (include/nspeech_hip.h, ns_wavenet_gate_params)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _hp(**over):
    from nspeech_amd import hparams as hparams_mod
    hp = hparams_mod.load("wavenet")
    small = dict(dilations_depth=2, dilations_length=3, residual_channels=16, dilation_channels=16, skip_channels=32,
                 quantization_channels=64)
    small.update(over)
    for k, v in small.items():
        setattr(hp, k, v)
    return hp


def _audio(N, T, seed):
    rng = np.random.RandomState(seed)
    t = np.arange(T) / 16000.0
    return np.stack([0.6 * np.sin(2 * np.pi * rng.uniform(100, 900) * t + rng.uniform(0, 6)) + 0.05 * rng.randn(T)
                     for _ in range(N)]).astype(np.float32)


def _randomise(m, seed):
    """Biases start at zero and a square embedding as the identity (wavenet.py:20-33): give them values, so that a bias
    added to the wrong tensor or a swapped filter / gate half shows."""
    rng = np.random.RandomState(seed)
    p = m.numpy_params()
    for k in p:
        if k.endswith("_bias") or k.endswith("gc_embedding"):
            p[k] = (rng.randn(*p[k].shape) * 0.3).astype(np.float32)
    m.load_numpy_params(p)
    return p


def _t0s(t0, N):
    return np.repeat(np.asarray(t0, np.int64).reshape(-1), N)[:N] if np.ndim(t0) == 0 else np.asarray(t0, np.int64)


def _rows(T, hold, t0, N):
    """row index per (item, position), and the number of rows that needs"""
    idx = np.stack([np.maximum(0, np.arange(T) + t) // hold for t in _t0s(t0, N)])
    return idx, int(idx.max()) + 1


# ------------------------------------------------------------------ 1. ns_wavenet_hold_sum
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [4, 32])
@pytest.mark.parametrize("T,hold,t0", [(37, 5, [-9, 0, 3]),       # N * T = 111: no frame boundary on an item boundary
                                       (37, 1, [-9, 0, 3]), (37, 50, [-9, 0, 3]), (37, 5, None)])
def test_hold_sum_against_float64(dev, T, hold, t0, C, dtype):
    from nspeech_amd import ops
    N, W = 3, 2 * C
    idx, need = _rows(T, hold, t0 if t0 is not None else 0, N)
    rows = need + 1                              # the extra row has no position: zeros
    rng = np.random.RandomState(C + hold)
    x = rng.randn(N, T, W).astype(np.float32)
    dz = torch.from_numpy(x).to(dev)
    if dtype == "bf16":
        dz = dz.to(torch.bfloat16)
        x = dz.float().cpu().numpy()             # the sum runs over the values as rounded to bf16
    t0d = None if t0 is None else torch.tensor(t0, dtype=torch.int32, device=dev)
    ld, off = W + 3, 2                           # a column offset inside a wider output
    outs = []
    for _ in range(2):
        out = torch.full((N * rows * ld,), float("nan"), dtype=torch.float32, device=dev)
        ops.wavenet_hold_sum(dz.view(-1), N, T, C, out, ld, rows, hold, t0d, out_off=off)
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0], outs[1], equal_nan=True)                  # bit-identical from run to run
    flat = outs[0]
    got = np.stack([flat[off + i * ld: off + i * ld + W] for i in range(N * rows)]).reshape(N, rows, W)
    mask = np.ones(flat.shape, bool)
    for i in range(N * rows):
        mask[off + i * ld: off + i * ld + W] = False
    assert np.isnan(flat[mask]).all()            # nothing written outside the rows' own columns
    x64 = x.astype(np.float64)
    worst = 0.0
    for n in range(N):
        for r in range(rows):
            sel = idx[n] == r
            want = x64[n, sel].sum(axis=0)
            bound = sel.sum() * 2.0 ** -23 * np.abs(x64[n, sel]).sum(axis=0)      # fp32 summation of n_r terms
            err = np.abs(got[n, r] - want)
            assert (err <= bound).all(), (n, r, err.max(), bound.min())
            if not sel.any():
                assert not got[n, r].any()
            worst = max(worst, err.max())
    assert not got[:, rows - 1].any()
    print("hold_sum %s C=%d hold=%d: max error %.3e" % (dtype, C, hold, worst))


def test_hold_sum_and_gate_check_their_arguments(dev):
    from nspeech_amd import ops
    from nspeech_amd._lib import NSError
    dz = torch.zeros(2 * 8 * 8, device=dev)
    out = torch.zeros(64, device=dev)
    for kw, text in ((dict(cond_rows=2, cond_hold=0), "cond_hold"), (dict(cond_rows=0, cond_hold=2), "cond_rows")):
        with pytest.raises(NSError, match=text):
            ops.wavenet_hold_sum(dz, 2, 8, 4, out, 8, kw["cond_rows"], kw["cond_hold"])
        with pytest.raises(NSError, match=text):
            ops.wavenet_gate(dz, 16, 4, 8, 0, out=torch.zeros(64, device=dev), ld_out=4, cond=out, ld_cond=8, **kw)
    with pytest.raises(NSError, match="ld_out"):
        ops.wavenet_hold_sum(dz, 2, 8, 4, out, 7, 2, 2)
    with pytest.raises(NSError, match="ld_cond"):
        ops.wavenet_gate(dz, 16, 4, 8, 0, out=torch.zeros(64, device=dev), ld_out=4, cond=out, ld_cond=7, cond_rows=2, cond_hold=2)
    with pytest.raises(TypeError):               # dz is fp32 or bf16
        ops.wavenet_hold_sum(dz.double(), 2, 8, 4, out, 8, 2, 2)


def test_gate_clamps_the_row_at_both_ends(dev):
    """Two rows for positions that would ask for rows -2 .. 3: the kernel reads rows 0 and 1 only (the Python layer refuses
    such a call; the kernel must still stay inside cond)."""
    from nspeech_amd import ops
    N, T, C, hold = 2, 8, 4, 2
    rng = np.random.RandomState(0)
    z = rng.randn(N * T, 2 * C).astype(np.float32)
    cond = rng.randn(N, 2, 2 * C).astype(np.float32)
    t0 = np.array([-3, 1])
    out = torch.full((N * T * C,), float("nan"), device=dev)
    ops.wavenet_gate(torch.from_numpy(z).to(dev).view(-1), N * T, C, T, 0, out=out, ld_out=C,
                     cond=torch.from_numpy(cond).to(dev).view(-1), ld_cond=2 * C, cond_rows=2, cond_hold=hold,
                     cond_t0=torch.tensor(t0, dtype=torch.int32, device=dev))
    r = np.minimum(1, np.maximum(0, np.arange(T)[None] + t0[:, None]) // hold)
    zz = z.reshape(N, T, 2 * C).astype(np.float64) + cond[np.arange(N)[:, None], r].astype(np.float64)
    want = np.tanh(zz[..., :C]) / (1 + np.exp(-zz[..., C:]))
    assert np.abs(out.cpu().numpy().reshape(N, T, C) - want).max() < 1e-6


# ------------------------------------------------------------------ 2. the model in fp32 against the oracle
FP32_CASES = {
    "hold 5": (dict(lc_channels=3, use_biases=True), 5, [-9, 0, 7]),
    "hold 1": (dict(lc_channels=3, use_biases=True), 1, 0),
    "hold 100": (dict(lc_channels=3, use_biases=True), 100, 0),
    "hold 5, gc category": (dict(lc_channels=3, use_biases=True, gc_channels=4, gc_category_cardinality=3), 5, [-9, 0, 7]),
}
_SHARED = {}


def _case_data(name, N=3, T=64):
    """Inputs of a case and the oracle's float64 loss, logits and gradients on the condition expanded per sample -
    computed once, shared by the fp32 and the bf16 test."""
    if name in _SHARED:
        return _SHARED[name]
    from oracle import wavenet_oracle as O
    from nspeech_amd.models import create_model
    over, hold, t0 = FP32_CASES[name]
    hp = _hp(**over)
    m = create_model("wavenet", hp, device="cuda:0", dtype="fp32", seed=4)
    params = _randomise(m, 7)
    audio = _audio(N, T, seed=2)
    rng = np.random.RandomState(3)
    idx, F = _rows(T - 1, hold, t0, N)
    frames = rng.randn(N, F, hp.lc_channels).astype(np.float32)
    gc = None
    if hp.gc_channels:
        gc = rng.randint(0, hp.gc_category_cardinality, size=N)
        gc[0] = gc[-1]
    expanded = np.stack([frames[n, idx[n]] for n in range(N)])               # [N, T - 1, lc]: the per-sample form
    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    loss, logits = O.loss_full(p, hp.values(), audio, gc, expanded)
    loss.backward()
    grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in p.items()}
    _SHARED[name] = dict(over=over, hold=hold, t0=t0, params=params, audio=audio, frames=frames, gc=gc, expanded=expanded,
                         loss=loss.item(), logits=logits.detach().numpy(), grads=grads)
    return _SHARED[name]


@pytest.mark.parametrize("case", sorted(FP32_CASES))
def test_held_condition_fp32_matches_oracle(dev, case):
    from nspeech_amd.models import create_model
    d = _case_data(case)
    m = create_model("wavenet", _hp(**d["over"]), device="cuda:0", dtype="fp32", seed=4)
    m.load_numpy_params(d["params"])
    m.initialize(d["audio"], d["gc"], d["frames"], hold=d["hold"], t0=d["t0"])
    m.backward()
    got_loss = m.read_losses()
    logits = d["logits"]
    assert np.abs(m.raw_output.cpu().numpy() - logits).max() < 2e-5 * max(1.0, np.abs(logits).max())
    assert abs(got_loss - d["loss"]) < 1e-5 * max(1.0, abs(d["loss"]))
    got = m.numpy_grads()
    assert set(got) == set(d["grads"])
    for k, want in d["grads"].items():
        scale = np.abs(want).max()
        assert np.abs(got[k] - want).max() < 1e-4 * scale + 1e-8, (k, np.abs(got[k] - want).max(), scale)
        if k.endswith("lc_filter") or k.endswith("lc_gate"):
            assert scale > 0, k
    # step() without arguments replays the batch with its hold and t0
    m.add_optimizer(0)
    m.step()
    assert abs(m.loss - d["loss"]) < 1e-5 * max(1.0, abs(d["loss"]))          # (the loss of the parameters before the step)


# ------------------------------------------------------------------ 3. training and generation read the same rows
def test_training_and_generation_agree_on_hold_and_t0(dev):
    from nspeech_amd.models import create_model
    hp = _hp(lc_channels=3, use_biases=True)
    m = create_model("wavenet", hp, device="cuda:0", dtype="fp32", seed=9)
    _randomise(m, 11)
    rng = np.random.RandomState(1)
    n_seed, n_new, hold = m.rf + 3, 8, 3
    t0 = -(m.rf + 1)
    seed = rng.randint(0, hp.quantization_channels, size=(1, n_seed))
    frames = rng.randn(1, max(0, n_seed + n_new - 1 + t0) // hold + 1, 3).astype(np.float32)
    assert frames.shape[1] >= 4                  # the drawn samples span several rows
    ids = m.generate(seed, n_new, uniforms=rng.rand(1, n_new), local_conditions=frames, hold=hold, t0=t0)
    want = m.last_probs.cpu().numpy().astype(np.float64)
    m.initialize_ids(ids, local_conditions=frames, hold=hold, t0=t0)
    lg = m.raw_output[0, -1].double().cpu().numpy()          # the row that predicts the last drawn sample
    pr = np.exp(lg - lg.max())
    pr /= pr.sum()
    err = np.abs(pr - want).max()
    print("training's softmax against the generator's last_probs: %.3e" % err)
    assert err < 1e-5
    # and the check can see a row off by one: frames moved by one row change the distribution by far more
    m.initialize_ids(ids, local_conditions=np.roll(frames, 1, axis=1), hold=hold, t0=t0)
    lg = m.raw_output[0, -1].double().cpu().numpy()
    p2 = np.exp(lg - lg.max())
    assert np.abs(p2 / p2.sum() - want).max() > 1e-3


# ------------------------------------------------------------------ 4. bf16: the held form beside the per-sample form
def test_held_condition_bf16_no_worse_than_per_sample(dev):
    """Both forms add the condition term in fp32 to the same pre-activations; only the order of summation differs.  Per
    tensor the held form's error against the float64 oracle is at most 2 x the per-sample form's."""
    from nspeech_amd.models import create_model
    d = _case_data("hold 5")
    errs = {}
    for form in ("per sample", "held"):
        m = create_model("wavenet", _hp(**d["over"]), device="cuda:0", dtype="bf16", seed=4)
        m.load_numpy_params(d["params"])
        if form == "held":
            m.initialize(d["audio"], d["gc"], d["frames"], hold=d["hold"], t0=d["t0"])
        else:
            m.initialize(d["audio"], d["gc"], d["expanded"])
        m.backward()
        e = {"logits": np.abs(m.raw_output.cpu().numpy() - d["logits"]).max(), "loss": abs(m.read_losses() - d["loss"])}
        got = m.numpy_grads()
        for k, want in d["grads"].items():
            e[k] = np.abs(got[k] - want).max()
        errs[form] = e
    for k in errs["held"]:
        print("bf16 error vs float64  %-52s per sample %.3e  held %.3e" % (k, errs["per sample"][k], errs["held"][k]))
    bad = {k: (errs["held"][k], errs["per sample"][k]) for k in errs["held"] if errs["held"][k] > 2 * errs["per sample"][k]}
    assert not bad, bad


# ------------------------------------------------------------------ 5. refusals
def test_refusals_come_before_any_launch(dev):
    from nspeech_amd.models import create_model
    N, T = 3, 64
    audio = _audio(N, T, seed=2)
    m = create_model("wavenet", _hp(lc_channels=3), device="cuda:0", dtype="fp32", seed=4)
    frames = np.zeros((N, 13, 3), np.float32)                # positions 0 .. 62 at hold 5 from t0 = 0: rows 0 .. 12
    m.initialize(audio, None, frames, hold=5, t0=0)
    m.backward()
    state = (m.ids, m._last, m._held, m._net_in)
    logits, grads = m.raw_output.clone(), m.flat_g.clone()
    for kw in (dict(hold=0), dict(hold=5, t0=[0, 0]),
               dict(hold=5, t0=[0, 0, 3])):                  # item 2 reaches row 13
        with pytest.raises(ValueError):
            m.initialize(audio + 0.1, None, frames, **kw)
    with pytest.raises(ValueError):
        m.initialize(audio + 0.1, None, frames[:, :12], hold=5)
    # a refused call launched nothing and replaced nothing: the model still holds the last good batch
    assert all(a is b for a, b in zip(state, (m.ids, m._last, m._held, m._net_in)))
    assert torch.equal(m.raw_output, logits) and torch.equal(m.flat_g, grads)
    m.initialize(audio, None, frames, hold=5, t0=[-9, 0, 2])
    plain = create_model("wavenet", _hp(use_biases=True), device="cuda:0", dtype="fp32", seed=4)
    with pytest.raises(ValueError):
        plain.initialize(audio, None, frames, hold=5)
    # hold=None: the per-sample form as before
    m.initialize(audio, None, np.zeros((N, T - 1, 3), np.float32))
    m.backward()
    assert np.isfinite(m.read_losses())


# ------------------------------------------------------------------ 6. Synthesizer
TACO_SMALL = dict(embedding_dim=32, encoder_conv_channels=64, encoder_lstm_units=32, attention_dim=64, decoder_lstm_units=64,
                  postnet_conv_channels=64, expand_conv_channels=64, expand_lstm_units=32, batch_size=2, batch_group_size=2,
                  max_iters=3)


def test_synthesizer_vocodes_through_the_wavenet(dev):
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.models.wavenet import mu_law_decode, mu_law_encode
    from nspeech_amd.synthesizer import Synthesizer
    small = dict(dilations_depth=1, dilations_length=4, residual_channels=32, dilation_channels=32, skip_channels=64,
                 quantization_channels=64)
    whp = _hp(lc_channels=80, use_biases=True, **small)
    bad = _hp(lc_channels=40, **small)
    hp = hparams_mod.load("taco2")
    for k, v in TACO_SMALL.items():
        setattr(hp, k, v)
    hparams_mod.set_hparams(hp)
    synth = Synthesizer(hp, dtype="bf16").load(None, "taco2")
    text = "Hello, World."
    before = synth.synthesize(text)
    with pytest.raises(ValueError):
        synth.synthesize(text, vocoder="wavenet")            # no vocoder yet
    with pytest.raises(ValueError, match="lc_channels"):
        synth.load_vocoder(None, bad)
    for name, value in (("sample_rate", 16000), ("frame_shift_ms", 10.0)):
        other = _hp(lc_channels=80, **small)
        setattr(other, name, value)
        with pytest.raises(ValueError, match="sample_rate" if name == "sample_rate" else "hop"):
            synth.load_vocoder(None, other)
    assert synth.vocoder is None
    synth.load_vocoder(None, whp)
    after = synth.synthesize(text)                           # the default call is what it was
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    T, hop = hp.max_iters * hp.outputs_per_step, 250
    assert T * hop < 5000
    wav, mel, lin = synth.synthesize(text, vocoder="wavenet", seed=5)
    assert mel.shape == (T, 80) and np.array_equal(mel, before[1]) and np.array_equal(lin, before[2])
    assert wav.ndim == 1 and len(wav) <= T * hop and np.isfinite(wav).all() and np.abs(wav).max() <= 1.0
    v = synth.vocoder
    Q = v.Q
    silence = int(mu_law_encode(np.zeros(1, np.float32), Q)[0])
    ids = v.generate(np.full((1, v.rf), silence, np.int32), T * hop, seed=5, local_conditions=mel[None], hold=hop, t0=-v.rf)
    want = mu_law_decode(ids[0, v.rf:].cpu().numpy(), Q)
    full = synth._wavenet_vocode(mel, seed=5)                # what synthesize cuts at find_endpoint
    assert full.shape == (T * hop,) and np.array_equal(full, want)
    assert np.array_equal(wav, want[:len(wav)])
    assert len(set(ids[0, v.rf:].cpu().numpy().tolist())) > 1
