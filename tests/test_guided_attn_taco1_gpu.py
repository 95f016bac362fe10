"""Guided attention loss in the Tacotron-1 training step: the shipped widths (persistent attention backward, the path with
a da0 term) against the float64 oracle with the term added to its loss, and the refusal of the launch-per-step path.

The driver is the one of tests/test_taco1_fullwidth_gpu.py restated with the term: targets moved off the oracle's free
predictions (L1 sign() gradients), the model's forward pass, then the oracle on the model's own ReLU branches
(taco2_oracle.MASK_FORCE) with weight * L_att(out["alignments"]) added to taco1_loss before backward().  The bounds are
that file's BOUNDS["fp32"]."""
import numpy as np
import pytest
import torch

import guided_attn_ref as R
from test_taco1_fullwidth_gpu import BOUNDS, _model_masks
from util import make_batch, rel_l2, rel_max

pytestmark = pytest.mark.gpu

SHAPE = (4, 24, 40)                 # outputs_per_step 5 -> S = 8
FRAMES = (40, 33, 17, 4)            # -> S_n = (8, 7, 4, 1)


def _oracle(hp, params, stats, inputs, lengths, mel, lin, steps=None, weight=0.0, sigma=0.4, need_grad=True, force=None):
    from oracle import taco1_oracle as O1, taco2_oracle as O2
    f64 = torch.float64
    p = {k: torch.tensor(v, dtype=f64, requires_grad=need_grad) for k, v in params.items()}
    p.update({k: torch.tensor(v, dtype=f64) for k, v in stats.items()})
    O2.MASK_FORCE = None if force is None else [np.asarray(x) for x in force]
    try:
        with torch.set_grad_enabled(need_grad):
            out = O1.taco1_forward(p, hp.values(), torch.tensor(inputs), torch.tensor(lengths), torch.tensor(mel, dtype=f64),
                                   torch.tensor(lin, dtype=f64))
            loss, _, _ = O1.taco1_loss(hp.values(), out, torch.tensor(mel, dtype=f64), torch.tensor(lin, dtype=f64))
            att = R.torch_loss(out["alignments"], lengths, steps, sigma)
            focus = R.torch_focus(out["alignments"], lengths, steps)
            total = loss + weight * att if weight else loss
    finally:
        O2.MASK_FORCE = None
    grads = None
    if need_grad:
        total.backward()
        grads = {k: (p[k].grad.numpy() if p[k].grad is not None else np.zeros_like(params[k])) for k in params}
    return out, dict(loss=float(total.detach()), att=float(att.detach()), focus=float(focus.detach())), grads


def test_shipped_widths_match_the_oracle_with_the_term(dev):
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.models import create_model
    N, Ti, To = SHAPE
    weight, sigma, margin = 1.0, 0.4, 2e-3
    hp = hparams_mod.load("taco1")
    hp.guided_attention_weight, hp.guided_attention_sigma = weight, sigma
    m = create_model("taco1", hp, device="cuda:0", dtype="fp32", seed=5)
    inputs, lengths, mel, lin = make_batch(hp, N, Ti, To, seed=N + 40)
    steps = R.out_steps(FRAMES, hp.outputs_per_step, To // hp.outputs_per_step)
    assert steps.tolist() == [8, 7, 4, 1]
    params, stats = m.numpy_params(), m.numpy_stats()
    mel, lin = mel.copy(), lin.copy()
    for _ in range(3):                              # L1 targets off the free pass' predictions (sign() gradients)
        free, _, _ = _oracle(hp, params, stats, inputs, lengths, mel, lin, need_grad=False)
        bm = np.abs(free["mel_outputs"].numpy() - mel) < margin
        bl = np.abs(free["linear_outputs"].numpy() - lin) < margin
        if not bm.any() and not bl.any():
            break
        mel[bm] -= 10 * margin
        lin[bl] -= 10 * margin
    m.initialize(inputs, lengths, None, mel, lin, target_lengths=np.asarray(FRAMES))
    masks = _model_masks(m)
    _, want, grads = _oracle(hp, params, stats, inputs, lengths, mel, lin, steps, weight, sigma, force=masks)
    _, _, plain = _oracle(hp, params, stats, inputs, lengths, mel, lin, steps, 0.0, sigma, force=masks)
    m.backward()
    m.read_losses()
    m.check_status()
    assert m.last_paths["attn:fwd"] == "cluster" and m.last_paths["attn:bwd"] == "cluster"
    b = BOUNDS["fp32"]
    print("loss %.7f (oracle %.7f)  attention_loss %.7f (%.7f)  attention_focus %.7f (%.7f)"
          % (m.loss, want["loss"], m.attention_loss, want["att"], m.attention_focus, want["focus"]))
    assert abs(m.loss - want["loss"]) < b["loss"] * abs(want["loss"])
    assert abs(m.attention_loss - want["att"]) < 1e-5 and abs(m.attention_focus - want["focus"]) < 1e-5
    assert abs(m.loss - (m.mel_loss + m.linear_loss + weight * m.attention_loss)) < 1e-12
    got = m.numpy_grads()
    gn = np.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in grads.values()))
    rep = {}
    for k in grads:
        if k.endswith("conv1d/bias") or np.linalg.norm(grads[k]) < 1e-9 * gn:      # zero true gradient in front of BatchNorm
            rep[k] = (float(np.linalg.norm(got[k] - grads[k]) / gn), float(np.abs(got[k] - grads[k]).max() / gn))
        else:
            rep[k] = (rel_l2(got[k], grads[k]), rel_max(got[k], grads[k]))
    worst = sorted(rep.items(), key=lambda kv: -kv[1][0])[:3]
    med = float(np.median([v[0] for v in rep.values()]))
    print("worst gradients %s; median %.2e" % ([(k, float("%.2e" % v[0])) for k, v in worst], med))
    bad = [(k, v) for k, v in rep.items() if not (v[0] < b["grad_l2"] and v[1] < b["grad_max"])]
    assert not bad, bad
    assert med < b["grad_l2_median"]
    # power: the term moves the attention query layer's gradient by far more than the bound allows
    k = "decoder/attention/query_layer/kernel"
    moved = rel_l2(plain[k], grads[k])
    print("query_layer gradient moves by %.3e (rel L2) with the term; bound %.1e" % (moved, b["grad_l2"]))
    assert moved > 10 * b["grad_l2"]


def test_launch_per_step_attention_refuses_a_positive_weight(dev):
    from test_taco1_gpu import _hp
    from nspeech_amd.models import create_model
    hp = _hp()                      # attention_dim 64: not the width of the persistent attention kernels
    hp.guided_attention_weight = 1.0
    m = create_model("taco1", hp, device="cuda:0", dtype="fp32", seed=4)
    inputs, lengths, mel, lin = make_batch(hp, 2, 9, 15, seed=2)
    m.add_loss().add_optimizer(global_step=0)           # nothing is known about the path before a forward pass
    with pytest.raises(ValueError, match="launch-per-step"):
        m.step(inputs, lengths, mel, lin)
    assert m.last_paths["attn:fwd"] == "step"
    with pytest.raises(ValueError, match="guided_attention_weight"):
        m.add_loss()                                    # known now
    # weight 0 on the same path trains as ever, and its summary still carries the two scores
    hp0 = _hp()
    m0 = create_model("taco1", hp0, device="cuda:0", dtype="fp32", seed=4)
    m0.add_loss().add_optimizer(global_step=0).add_stats()
    assert np.isfinite(m0.step(inputs, lengths, mel, lin))
    s = m0.stats()
    assert 0.0 <= s["loss_attention"] < 1.0 and 0.0 < s["attention_focus"] <= 1.0
