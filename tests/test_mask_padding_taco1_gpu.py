"""L1 losses over each utterance's real frames in the Tacotron-1 training step (hparam mask_padding): the small
configuration and driver of tests/test_taco1_gpu.py against the float64 oracle with masked_loss_ref.masked_taco_loss in
place of taco1_loss (the mel term lands in the decoder-output gradient: P = (S + 1) r, padl = r), a padded frame's linear
target that no longer matters, full lengths = the switch off, the switch off = the step as it was, bit-equal scalars from
step to step, and one `mixed` step."""
import numpy as np
import pytest
import torch

import masked_loss_ref as R
from test_taco1_gpu import _hp, _stabilise
from util import make_batch

pytestmark = pytest.mark.gpu

SHAPE = (3, 11, 20)             # N, T_in, T_out; outputs_per_step 5 -> S = 4
FRAMES = (20, 12, 3)


def _hps(**over):
    hp = _hp()
    for k, v in over.items():
        setattr(hp, k, v)
    return hp


def _model(hp, dtype="fp32", seed=4):
    from nspeech_amd.models import create_model
    return create_model("taco1", hp, device="cuda:0", dtype=dtype, seed=seed)


def _oracle(hp, params, stats, inputs, lengths, mel, lin, frames, need_grad=True):
    from oracle import taco1_oracle as O
    f64 = torch.float64
    p = {k: torch.tensor(v, dtype=f64, requires_grad=need_grad) for k, v in params.items()}
    p.update({k: torch.tensor(v, dtype=f64) for k, v in stats.items()})
    hpd = hp.values()
    tm, tl = torch.tensor(mel, dtype=f64), torch.tensor(lin, dtype=f64)
    with torch.set_grad_enabled(need_grad):
        out = O.taco1_forward(p, hpd, torch.tensor(inputs), torch.tensor(lengths), tm, tl)
        if frames is None:
            loss, mel_loss, lin_loss = O.taco1_loss(hpd, out, tm, tl)
        else:
            loss, mel_loss, lin_loss = R.masked_taco_loss(out, tm, tl, frames, int(3000 / (hp.sample_rate * 0.5) * hp.num_freq))
    grads = None
    if need_grad:
        loss.backward()
        grads = {k: (p[k].grad.numpy() if p[k].grad is not None else np.zeros_like(params[k])) for k in params}
    return dict(loss=float(loss.detach()), mel=float(mel_loss.detach()), lin=float(lin_loss.detach()), grads=grads)


def test_step_matches_the_oracle_with_the_masked_loss(dev):
    N, Ti, To = SHAPE
    hp = _hps(mask_padding=True)
    assert hp.outputs_per_step == 5
    m = _model(hp)
    assert m.mask_padding is True
    params, stats = m.numpy_params(), m.numpy_stats()
    inputs, lengths, mel, lin = make_batch(hp, N, Ti, To, seed=N)
    mel, lin = _stabilise(hp, params, stats, inputs, lengths, mel, lin)
    want = _oracle(hp, params, stats, inputs, lengths, mel, lin, FRAMES)
    plain = _oracle(hp, params, stats, inputs, lengths, mel, lin, None)
    m.initialize(inputs, lengths, None, mel, lin, target_lengths=np.asarray(FRAMES))
    m.backward()
    m.read_losses()
    torch.cuda.synchronize()
    print("loss %.7f (oracle %.7f masked, %.7f over the padded batch)  mel %.7f (%.7f)  linear %.7f (%.7f)"
          % (m.loss, want["loss"], plain["loss"], m.mel_loss, want["mel"], m.linear_loss, want["lin"]))
    assert abs(m.loss - want["loss"]) < 1e-5 * max(1.0, abs(want["loss"]))
    assert abs(m.mel_loss - want["mel"]) < 1e-5 and abs(m.linear_loss - want["lin"]) < 1e-5
    assert m.loss == m.mel_loss + m.linear_loss
    got = m.numpy_grads()
    bad = []
    for k, gk in want["grads"].items():
        scale = np.abs(gk).max()
        err = np.abs(got[k] - gk).max()
        if err > 2e-3 * scale + 5e-6:
            bad.append((k, float(err), float(scale)))
    print("gradient tensors over the bound:", bad)
    assert not bad, bad
    # power: on the CPU, with the seed-4 parameters and this batch, the oracle's gradient of the loss over the padded
    # batch misses that bound by more than 10x on 121 of the 124 tensors (prenet/dense_1/bias by 430x, the embedding by
    # 270x, the linear head dense/kernel by 110x; the three that do not are two biases in front of a BatchNorm and the
    # attention query layer), and the loss is 1.020222 masked against 1.046101
    miss = {k: np.abs(plain["grads"][k] - gk).max() / (2e-3 * np.abs(gk).max() + 5e-6) for k, gk in want["grads"].items()}
    far = [k for k, v in miss.items() if v > 10]
    print("%d of %d tensors of the unmasked gradient miss the bound by more than 10x" % (len(far), len(miss)))
    assert len(far) > len(miss) // 2
    for k in ("prenet/dense_1/bias", "prenet/dense_1/kernel", "embedding/embedding", "post_cbhg/dense/kernel", "dense/kernel"):
        assert miss[k] > 10, (k, miss[k])
    assert abs(plain["loss"] - want["loss"]) > 100 * 1e-5


def _one_step(m, batch, frames=None):
    inputs, lengths, mel, lin = batch
    m.deterministic = True
    m.add_optimizer(global_step=0)
    m.step(inputs, lengths, mel, lin, target_lengths=frames)
    torch.cuda.synchronize()
    return m.flat_g.clone(), m.scal.clone(), (m.loss, m.mel_loss, m.linear_loss), m.flat_stats.clone()


def _bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_linear_targets_of_padded_frames_do_not_matter(dev):
    """Not the mel targets: they also feed the teacher-forced decoder, so a change to them does move the result."""
    N, Ti, To = SHAPE
    hp = _hps(mask_padding=True, deterministic_gradients=True)
    inputs, lengths, mel, lin = make_batch(hp, N, Ti, To, seed=5)
    other = lin.copy()
    for n, tn in enumerate(FRAMES):
        other[n, tn:] = 5.0 - other[n, tn:]
    a = _one_step(_model(hp), (inputs, lengths, mel, lin), np.asarray(FRAMES))
    b = _one_step(_model(hp), (inputs, lengths, mel, other), np.asarray(FRAMES))
    assert _bits(a[0], b[0]) and _bits(a[1], b[1]) and a[2] == b[2]
    c = _one_step(_model(_hps(deterministic_gradients=True)), (inputs, lengths, mel, other), np.asarray(FRAMES))
    assert abs(c[2][0] - a[2][0]) > 1e-2


def test_full_lengths_give_the_gradients_of_the_switch_off(dev):
    N, Ti, To = SHAPE
    batch = make_batch(_hp(), N, Ti, To, seed=5)
    on = _one_step(_model(_hps(mask_padding=True, deterministic_gradients=True)), batch, np.full(N, To))
    none = _one_step(_model(_hps(mask_padding=True, deterministic_gradients=True)), batch, None)
    off = _one_step(_model(_hps(deterministic_gradients=True)), batch, np.full(N, To))
    assert _bits(on[0], off[0]) and _bits(on[3], off[3])
    assert _bits(on[0], none[0]) and _bits(on[1], none[1])
    for x, y in zip(on[2], off[2]):                                # the sums are added in another order
        assert abs(x - y) <= 1e-5 * max(1.0, abs(y)), (on[2], off[2])


def test_switch_off_is_the_step_as_it_was(dev):
    """scal[0:4], ns_l1_loss' float-atomic sums, to 1e-6 relative (tests/test_guided_attn_taco2_gpu.py: _same_scalars);
    everything else bit for bit."""
    N, Ti, To = SHAPE
    hp0 = _hp()
    assert hp0.mask_padding is False
    batch = make_batch(hp0, N, Ti, To, seed=5)
    m1 = _model(_hp())
    g0, s0, l0, st0 = _one_step(_model(hp0), batch)
    g1, s1, l1, st1 = _one_step(m1, batch, np.asarray(FRAMES))
    assert _bits(g0, g1) and _bits(st0, st1)
    assert _bits(s0[4:], s1[4:])
    assert ((s0[:4] - s1[:4]).abs() <= 1e-6 * s1[:4].abs()).all(), (s0, s1)
    assert all(abs(x - y) <= 1e-6 * abs(y) for x, y in zip(l0, l1)), (l0, l1)
    assert "l1m_work" not in m1._bufs


def test_masked_steps_repeat_bit_for_bit_scalars_included(dev):
    N, Ti, To = SHAPE
    hp = _hps(mask_padding=True, deterministic_gradients=True)
    batch = make_batch(hp, N, Ti, To, seed=5)
    m = _model(hp)
    runs = []
    for _ in range(2):
        m.initialize(*batch[:2], None, *batch[2:], target_lengths=np.asarray(FRAMES))
        m.backward()
        torch.cuda.synchronize()
        runs.append((m.flat_g.clone(), m.scal.clone()))
    assert float(runs[0][1][0]) > 0.0 and float(runs[0][1][3]) > 0.0
    assert _bits(runs[0][0], runs[1][0])
    assert _bits(runs[0][1], runs[1][1]), (runs[0][1], runs[1][1])


def test_mixed_step(dev):
    N, Ti, To = SHAPE
    hp = _hps(mask_padding=True)
    batch = make_batch(hp, N, Ti, To, seed=5)
    m = _model(hp, "mixed")
    want = _oracle(hp, m.numpy_params(), m.numpy_stats(), *batch, FRAMES, need_grad=False)
    m.add_loss().add_optimizer(global_step=0)
    loss = m.step(*batch, target_lengths=np.asarray(FRAMES))
    m.check_status()
    print("mixed loss %.6f, oracle %.6f" % (loss, want["loss"]))
    assert abs(loss - want["loss"]) < 3e-2 * abs(want["loss"])     # test_taco2_gpu's bound for the mixed loss
    assert loss == m.mel_loss + m.linear_loss
    assert np.isfinite(m.flat_g.cpu().numpy()).all()
