"""hparam prenet_dropout in the two Tacotron models: training passes with live prenet dropout against the float64 oracles
whose `prenet` is replaced by tests/prenet_dropout_ref.py: patched_prenet on the SAME masks (the model's own
prenet_dropout_args(), restated by the NumPy generator of that module), forward and backward, through the persistent
attention clusters (shipped and small widths) and the step-launch forms (small widths with the persistent form switched
off; Tacotron-1's Python loop); and what the
option must leave alone: off is the parent's pass bit for bit, synthesis is the identity, every step draws new masks.

Bounds: tests/test_taco2_fullwidth_gpu.py's BOUNDS at the shipped widths, tests/test_zoneout_gpu.py's small-width bounds,
tests/test_taco1_fullwidth_gpu.py's BOUNDS / FLIPS for Tacotron-1.  MATTER_THRESHOLD is fixed on the CPU by
tests/test_prenet_dropout_ref_cpu.py: ten times the small-width output bound, which the oracle's masked and plain passes
exceed on the inputs below."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import prenet_dropout_ref as PR
from util import check_flips, make_batch, oracle_report, rel_l2, rel_max, small_hparams, stabilise_targets

pytestmark = pytest.mark.gpu

SMALL_OUT_BOUND = 5e-4                      # tests/test_zoneout_gpu.py: outputs of a small-width fp32 pass, max norm
MATTER_THRESHOLD = 10 * SMALL_OUT_BOUND
MATTER = dict(seed=3, rate=0.5, shape=(3, 11, 20), batch_seed=3)
DEC, ENC = "decoder/decoder_prenet", "prenet"


def expected_args(seed, rate, step, prenet="decoder"):
    """prenet_dropout_args() of a single-process model built with `seed` at global step `step`, stated independently:
    the zoneout base seed, mask streams 8 / 9 (decoder prenet) and 10 / 11 (Tacotron-1's encoder prenet)."""
    from nspeech_amd import ops
    base = (int(seed) * 2654435761 + 97) & 0xFFFFFFFF
    a, b = {"decoder": (8, 9), "encoder": (10, 11)}[prenet]
    return (PR.threshold(rate), 1.0 / (1.0 - rate), ops.zoneout_seed(base, step, a), ops.zoneout_seed(base, step, b))


def oracle_masks(seed, rate, step, N, S, Ti=None, widths=(256, 128)):
    """{scope: (keep1, keep2)} for patched_prenet: the decoder prenet's masks [S, N, U], with Ti also the encoder's [Ti, N, U]."""
    thr, _, s1, s2 = expected_args(seed, rate, step)
    out = {DEC: (~PR.dropped(s1, thr, S, N, 256), ~PR.dropped(s2, thr, S, N, 128))}
    if Ti is not None:
        _, _, e1, e2 = expected_args(seed, rate, step, "encoder")
        out[ENC] = (~PR.dropped(e1, thr, Ti, N, widths[0]), ~PR.dropped(e2, thr, Ti, N, widths[1]))
    return out


def mask_sets():
    """(label, dropped, rate) of the masks the tests below draw (tests/test_prenet_dropout_ref_cpu.py checks their shares)."""
    out = []
    for label, seed, rate, N, S, Ti in (("matter", MATTER["seed"], MATTER["rate"], 3, 4, None), ("taco2 shipped", 5, 0.5, 3, 8, None),
                                        ("taco1 shipped", 5, 0.5, 4, 8, 24)):
        for scope, pair in oracle_masks(seed, rate, 0, N, S, Ti).items():
            for i, k in enumerate(pair):
                out.append(("%s %s layer %d" % (label, scope, i + 1), ~k, rate))
    return out


def matter_inputs():
    """The masks-matter case on the CPU: hparams, the model's initial parameters and statistics (the values a model
    built with the same seed loads), and the batch."""
    from nspeech_amd.models import params as P_
    from nspeech_amd.utils.text.symbols import symbols
    hp = small_hparams()
    pv, sv = P_.init_values(*P_.taco2_layout(hp, len(symbols)), MATTER["seed"])
    N, Ti, To = MATTER["shape"]
    inputs, lengths, mel, lin = make_batch(hp, N, Ti, To, seed=MATTER["batch_seed"])
    return hp, pv, sv, inputs, lengths, mel, lin


def _drop_hp(hp, rate=0.5):
    hp.prenet_dropout = True
    hp.drop_rate = rate
    return hp


def _taco2_report(monkeypatch, hp, mode, shape, seed, batch_seed, rate=0.5):
    from oracle import taco2_oracle as O
    from nspeech_amd.models import create_model
    N, Ti, To = shape
    m = create_model("taco2", _drop_hp(hp, rate), device="cuda:0", dtype=mode, seed=seed)
    args = m.prenet_dropout_args()
    assert args == expected_args(seed, rate, 0), (args, expected_args(seed, rate, 0))
    monkeypatch.setattr(O, "prenet", PR.patched_prenet(O, oracle_masks(seed, rate, 0, N, To // hp.outputs_per_step), args[1]))
    inputs, lengths, mel, lin = make_batch(hp, N, Ti, To, seed=batch_seed)
    mel, lin = stabilise_targets(hp, m.numpy_params(), m.numpy_stats(), inputs, lengths, mel, lin)
    rep = oracle_report(m, hp, inputs, lengths, mel, lin)
    m.check_status()
    p1 = m._bufs["dec_p1"][:N * (To // hp.outputs_per_step + 1) * 256].float().view(N, -1, 256)[:, 1:]
    share = float((p1 == 0).float().mean())
    assert share > rate, share                       # the dropped units and the ReLU's own zeros
    return m, rep, (inputs, lengths, mel, lin)


@pytest.mark.parametrize("mode", ["fp32", "mixed"])
def test_taco2_shipped_widths_with_dropout_match_oracle(dev, monkeypatch, mode):
    from nspeech_amd import hparams as hparams_mod
    from test_taco2_fullwidth_gpu import _check
    hp = hparams_mod.load("taco2")
    shape = (3, 24, 40)
    m, rep, _ = _taco2_report(monkeypatch, hp, mode, shape, 5, 23)
    assert rep["paths"]["attn:fwd"] == "cluster" and rep["paths"]["attn:bwd"] == "cluster", rep["paths"]
    _check(rep, mode, shape)


@pytest.mark.parametrize("path", ["step", "cluster"])
def test_taco2_small_widths_with_dropout_match_oracle(dev, monkeypatch, path):
    """Small widths (attention 64: the A = 64 cluster kernels by default; with the persistent form switched off
    ns_taco2_attn_fwd / _bwd with ns_dropout_rows between the step launches); and the masks matter."""
    from nspeech_amd.models import create_model
    from nspeech_amd.models.tacotron2 import Tacotron2
    monkeypatch.setattr(Tacotron2, "use_attn_cluster", path == "cluster")
    hp = small_hparams()
    m, rep, (inputs, lengths, mel, lin) = _taco2_report(monkeypatch, hp, "fp32", MATTER["shape"], MATTER["seed"], MATTER["batch_seed"],
                                                        MATTER["rate"])
    assert rep["paths"]["attn:fwd"] == path and rep["paths"]["attn:bwd"] == path, rep["paths"]
    check_flips(rep, "fp32")
    for k, (l2, mx, l1) in rep["out"].items():
        assert mx < SMALL_OUT_BOUND, (k, mx)
    assert abs(rep["loss"][0] - rep["loss"][1]) < 1e-5 * abs(rep["loss"][1])
    bad = [(k, v) for k, v in rep["grad"].items() if not v[1] < 2e-3]
    assert not bad, bad
    # masks matter: the same-seed plain model on the same batch gives other decoder outputs, by more than the threshold
    plain = create_model("taco2", small_hparams(), device="cuda:0", dtype="fp32", seed=MATTER["seed"])
    plain.initialize(inputs, lengths, None, mel, lin)
    d = rel_max(m.decoder_outputs.float().cpu().numpy(), plain.decoder_outputs.float().cpu().numpy())
    print("dropout vs plain decoder outputs: rel max %.3e (threshold %.1e)" % (d, MATTER_THRESHOLD))
    assert d > MATTER_THRESHOLD, d


@pytest.mark.parametrize("mode", ["fp32", "mixed"])
def test_taco1_shipped_widths_with_dropout_match_oracle(dev, monkeypatch, mode):
    """Decoder prenet inside the attention clusters of csrc/attn_gru.hip and the encoder prenet through ns_dropout_rows."""
    import test_taco1_fullwidth_gpu as T1
    from oracle import taco1_oracle as O1, taco2_oracle as O2
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.models import create_model
    hp = _drop_hp(hparams_mod.load("taco1"))
    N, Ti, To = 4, 24, 40
    m = create_model("taco1", hp, device="cuda:0", dtype=mode, seed=5)
    assert m.prenet_dropout_args() == expected_args(5, 0.5, 0) and m.prenet_dropout_args("encoder") == expected_args(5, 0.5, 0, "encoder")
    masks = oracle_masks(5, 0.5, 0, N, To // hp.outputs_per_step, Ti, tuple(hp.encoder_prenet))
    monkeypatch.setattr(O1, "prenet", PR.patched_prenet(O2, masks, PR.scale_of(0.5)))
    inputs, lengths, mel, lin = make_batch(hp, N, Ti, To, seed=N + 40)
    rep = T1._report(m, hp, inputs, lengths, mel, lin)
    m.check_status()
    for k, v in T1.PATHS[mode].items():
        assert rep["paths"].get(k) == v, (k, rep["paths"])
    pre1 = m._bufs["a:pre1"][:N * m.dims["Pi"] * 256].float().view(N, -1, 256)[:, m.padl:m.padl + Ti]
    assert bool((pre1 == 0).cpu()[torch.from_numpy(~masks[ENC][0]).permute(1, 0, 2)].all()), "a dropped unit of the encoder prenet is not 0"
    b = T1.BOUNDS[mode]
    check_flips(rep, mode, bounds=T1.FLIPS[mode])
    assert rep["out"]["mel_outputs"][2] < b["mel_l1"], rep["out"]["mel_outputs"]
    for k, (l2, mx, l1) in rep["out"].items():
        assert mx < b["out"], (k, l2, mx, l1)
    got, want = rep["loss"]
    assert abs(got - want) < b["loss"] * abs(want), rep["loss"]
    bad = [(k, v) for k, v in rep["grad"].items() if not (v[0] < b["grad_l2"] and v[1] < b["grad_max"])]
    assert not bad, bad
    assert float(np.median([v[0] for v in rep["grad"].values()])) < b["grad_l2_median"]


def test_taco1_step_loop_draws_the_masks_of_the_cluster_kernel(dev, monkeypatch):
    """Tacotron-1's launch-per-step attention loop (ns_dropout_rows behind the p1 / p2 products and on dp2 / df1) against the
    persistent kernel on the same masks: same zero pattern exactly, outputs and gradients to rounding (the bounds of
    tests/test_taco1_fullwidth_gpu.py's comparison of the two forms)."""
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.models import create_model
    from nspeech_amd.models.tacotron import Tacotron
    hp = _drop_hp(hparams_mod.load("taco1"), 0.1)
    N, Ti, To = 4, 17, 30
    inputs, lengths, mel, lin = make_batch(hp, N, Ti, To, seed=9)
    res = {}
    for cluster in (True, False):
        monkeypatch.setattr(Tacotron, "use_attn_cluster", cluster)
        m = create_model("taco1", hp, device="cuda:0", dtype="bf16x3", seed=5)
        m.initialize(inputs, lengths, None, mel, lin)
        m.backward()
        m.read_losses()
        m.check_status()
        assert m.last_paths["attn:fwd"] == m.last_paths["attn:bwd"] == ("cluster" if cluster else "step")
        S1 = To // hp.outputs_per_step + 1
        res[cluster] = (m.mel_outputs.float().cpu().numpy(), m.numpy_grads(), m.loss, (m._bufs["dec_p1"][:N * S1 * 256] == 0).cpu(),
                        (m._bufs["dec_xa"][:N * S1 * 384].view(N, S1, 384)[:, :, :128] == 0).cpu())
    assert torch.equal(res[True][3], res[False][3]) and torch.equal(res[True][4], res[False][4])
    thr, _, s1, _ = expected_args(5, 0.1, 0)
    S = To // hp.outputs_per_step
    dropped = torch.from_numpy(PR.dropped(s1, thr, S, N, 256)).permute(1, 0, 2)
    z = res[False][3].view(N, S + 1, 256)[:, 1:]
    assert bool(z[dropped].all()) and 0.05 < float(dropped.float().mean()) < 0.15
    assert rel_max(res[True][0], res[False][0]) < 2e-5
    assert abs(res[True][2] - res[False][2]) < 1e-6 * abs(res[False][2])
    gn = np.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in res[False][1].values()))
    errs = sorted((rel_l2(res[True][1][k], res[False][1][k]), k) for k in res[True][1]
                  if not k.endswith("conv1d/bias") and np.linalg.norm(res[False][1][k]) > 1e-9 * gn)
    assert errs[len(errs) // 2][0] < 1e-4, errs[len(errs) // 2]
    assert errs[-1][0] < 3e-2, errs[-1]


def _train_pass(hp, batch, kind="taco2"):
    from nspeech_amd.models import create_model
    hp.deterministic_gradients = True
    m = create_model(kind, hp, device="cuda:0", dtype="fp32", seed=3)
    inputs, lengths, mel, lin = batch
    m.initialize(inputs, lengths, None, mel, lin)
    m.backward()
    m.read_losses()
    return m, m.mel_outputs.clone(), m.linear_outputs.clone(), m.flat_g.clone()


def test_off_is_off(dev):
    """prenet_dropout = false, and true at drop_rate 0, hand the kernels no dropout block: outputs and gradients equal,
    bit for bit, those of a model whose hparams do not have the key at all."""
    hp0 = small_hparams()
    batch = make_batch(hp0, 3, 11, 20, seed=3)
    del hp0._d["prenet_dropout"]
    assert "prenet_dropout" not in hp0
    ref = _train_pass(hp0, batch)
    assert ref[0].prenet_dropout_args() is None and ref[0]._dropout_block() == {}
    for over in (dict(prenet_dropout=False), dict(prenet_dropout=True, drop_rate=0.0)):
        got = _train_pass(small_hparams(**over), batch)
        assert got[0].prenet_dropout_args() is None and "drop_thr" not in got[0]._attn_args
        for a, b in zip(ref[1:], got[1:]):
            assert torch.equal(a, b), over
    with pytest.raises(ValueError):
        _train_pass(small_hparams(prenet_dropout=True, drop_rate=1.0), batch)
    with pytest.raises(ValueError):
        _train_pass(small_hparams(prenet_dropout=True, drop_rate=-0.1), batch)


def test_off_is_off_in_tacotron1(dev, monkeypatch):
    """The same for Tacotron-1's own plumbing (encoder prenet, cluster arguments, step loop): with the option off, or on
    at rate 0, no ns_dropout_rows launch is issued, the attention block carries no drop_* field and the outputs equal,
    bit for bit, those of a model whose hparams lack the key; with it on both appear."""
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd import ops
    from nspeech_amd.models import create_model
    calls = []
    orig = ops.dropout_rows
    monkeypatch.setattr(ops, "dropout_rows", lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1])
    hp0 = hparams_mod.load("taco1")
    batch = make_batch(hp0, 3, 11, 20, seed=3)
    del hp0._d["prenet_dropout"]

    def run(hp):
        m = create_model("taco1", hp, device="cuda:0", dtype="fp32", seed=3)
        del calls[:]
        m.initialize(batch[0], batch[1], None, batch[2], batch[3])
        m.backward()
        m.read_losses()
        return m, m.mel_outputs.clone(), m.linear_outputs.clone(), len(calls)
    ref = run(hp0)
    assert ref[3] == 0 and "drop_thr" not in ref[0]._attn_args
    for over in (dict(prenet_dropout=False), dict(prenet_dropout=True, drop_rate=0.0)):
        hp = hparams_mod.load("taco1")
        for k, v in over.items():
            setattr(hp, k, v)
        got = run(hp)
        assert got[3] == 0 and "drop_thr" not in got[0]._attn_args and got[0].prenet_dropout_args("encoder") is None
        assert torch.equal(ref[1], got[1]) and torch.equal(ref[2], got[2]), over
    on = run(_drop_hp(hparams_mod.load("taco1")))
    assert on[3] == 4 and on[0]._attn_args["drop_thr"] == PR.threshold(0.5)      # two encoder layers, forward and backward
    assert not torch.equal(ref[1], on[1])


@pytest.mark.parametrize("kind", ["taco2", "taco1"])
def test_every_training_step_draws_new_masks(dev, kind):
    """Two consecutive optimiser steps: each draws the masks the generator states for ITS global step (the decoder
    prenet's p1 and, for Tacotron-1, the encoder prenet's first layer), and they differ."""
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.models import create_model
    hp = _drop_hp(small_hparams() if kind == "taco2" else hparams_mod.load("taco1"))
    N, Ti, To = 3, 11, 20
    S = To // hp.outputs_per_step
    m = create_model(kind, hp, device="cuda:0", dtype="fp32", seed=3)
    inputs, lengths, mel, lin = make_batch(hp, N, Ti, To, seed=3)
    m.add_optimizer(global_step=0)
    zeros = []
    for step in (0, 1):
        assert m.global_step == step and m.prenet_dropout_args() == expected_args(3, 0.5, step)
        m.step(inputs, lengths, mel, lin)
        z = (m._bufs["dec_p1"][:N * (S + 1) * 256].view(N, S + 1, 256)[:, 1:] == 0).cpu()
        thr, _, s1, _ = expected_args(3, 0.5, step)
        assert bool(z[torch.from_numpy(PR.dropped(s1, thr, S, N, 256)).permute(1, 0, 2)].all())
        if kind == "taco1":
            W = hp.encoder_prenet[0]
            ze = (m._bufs["a:pre1"][:N * m.dims["Pi"] * W].view(N, -1, W)[:, m.padl:m.padl + Ti] == 0).cpu()
            e1 = expected_args(3, 0.5, step, "encoder")[2]
            assert bool(ze[torch.from_numpy(PR.dropped(e1, thr, Ti, N, W)).permute(1, 0, 2)].all())
            z = torch.cat([z.reshape(-1), ze.reshape(-1)])
        zeros.append(z)
    assert not torch.equal(zeros[0], zeros[1])


@pytest.mark.parametrize("kind", ["taco2", "taco1"])
def test_synthesis_is_the_identity(dev, kind):
    """initialize(inputs, lengths) with the option on is the option off, bit for bit, through the same decode path."""
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.models import create_model
    res = []
    for on in (False, True):
        if kind == "taco2":
            hp = small_hparams(max_iters=6)
        else:
            hp = hparams_mod.load("taco1")
            hp.max_iters = 4
        hp.prenet_dropout = on
        m = create_model(kind, hp, device="cuda:0", dtype="fp32", seed=2)
        inputs, lengths, _, _ = make_batch(hp, 2, 12, 10, seed=4)
        m.initialize(inputs, lengths)
        m.check_status()
        res.append((m.last_paths["decode"], m.mel_outputs.clone(), m.linear_outputs.clone(), m.alignments.clone()))
    assert res[0][0] == res[1][0] == "persistent"
    for a, b in zip(res[0][1:], res[1][1:]):
        assert torch.equal(a, b)


def test_train_cli_takes_the_option(tmp_path):
    from test_cli_gpu import ROOT, SMALL, _corpus
    data = str(tmp_path / "lj")
    os.makedirs(data)
    _corpus(data)
    logs = str(tmp_path / "logs")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--ljspeech", data, "--model", "taco2", "--log_dir", logs,
                        "--hparams", SMALL + ",prenet_dropout=true,drop_rate=0.3", "--checkpoint_interval", "2", "--precision", "bf16",
                        "--summary-interval", "1", "--max_steps", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    run = os.path.join(logs, "logs-taco2")
    assert os.path.exists(os.path.join(run, "model.ckpt-2"))
    import json
    ev = [json.loads(l) for l in open(os.path.join(run, "events.jsonl"))]
    assert [e["step"] for e in ev] == [1, 2] and all(np.isfinite(e["loss"]) for e in ev)
    assert "prenet_dropout: True" in r.stdout or "prenet_dropout: True" in open(os.path.join(run, "train.log")).read()
