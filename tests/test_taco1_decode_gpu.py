"""Tacotron-1 free-running synthesis as ONE persistent launch (ns_taco1_decode, csrc/attn_gru.hip "free-running
synthesis") at the shipped widths of hparams/taco1.yaml: against the launch-per-step loop on the same weights, against
the float64 oracle, with speakers, over the full 300 steps, repeated calls, and the fall-back for shapes it does not
cover."""
import numpy as np
import pytest
import torch

from util import make_batch, rel_max

pytestmark = pytest.mark.gpu

# persistent loop against the step loop on the same weights, 40 free-running steps, T_in = 37 (ragged), largest
# |difference| / largest |value|.  Measured on one MI355X (N = 1 / 2):
#   fp32    mel 1.1e-5 / 1.2e-5   align 2.1e-7 / 2.8e-7
#   mixed   mel 1.9e-5 / 1.9e-5   align 2.8e-7 / 2.8e-7
#   bf16x3  mel 1.9e-5 / 1.9e-5   align 2.8e-7 / 2.8e-7
#   bf16    mel 8.8e-3 / 8.7e-3   align 2.8e-7 / 3.7e-7   (the step loop runs the decoder GRUs on bf16 weights, the
#                                                          kernel on the fp32 master weights)
#   300 steps, T_in = 160, N = 2, mixed: mel 3.5e-5, align 3.4e-7;  speakers (fp32): mel 6.7e-7
LOOP_BOUNDS = {"fp32": 1e-4, "mixed": 1e-4, "bf16x3": 1e-4, "bf16": 0.05}
# against the float64 oracle: the "out" bounds of test_taco1_fullwidth_gpu.py.  Measured (N = 1 / 2): fp32 mel 2.1e-5 /
# 2.3e-5, linear 3.2e-5 / 3.9e-5, align 2.4e-7 / 2.5e-7; mixed mel 2.4e-5 / 2.4e-5, linear 3.3e-5 / 3.8e-5
ORACLE_BOUNDS = {"fp32": 3e-4, "bf16x3": 3e-4, "mixed": 3e-4, "bf16": 0.12}


def _hp(steps, speakers=1):
    from nspeech_amd import hparams as hparams_mod
    hp = hparams_mod.load("taco1")
    hp.max_iters = steps
    if speakers > 1:
        hp.num_speakers = speakers
    return hp


def _spread_speaker_path(m):
    """The default initialisation leaves the speaker path almost inert; spread the table and the biases so that a wrong
    row block or a missed speaker term shows (as test_taco1_gpu.py does)."""
    p = m.numpy_params()
    rs = np.random.RandomState(11)
    p["speaker/speaker_embed"] = rs.uniform(-2.0, 2.0, size=p["speaker/speaker_embed"].shape).astype(np.float32)
    for k in p:
        if k.endswith("/dense/bias") and ("highway_" in k or k in ("encoder_cbhg/dense/bias", "decoder/dense/bias")):
            p[k] = rs.uniform(-0.5, 0.5, size=p[k].shape).astype(np.float32)
    m.load_numpy(p, m.numpy_stats())


def _batch(hp, N, Ti, seed):
    inputs, lengths, _, _ = make_batch(hp, N, Ti, 10, seed=seed)
    lengths = np.asarray(lengths).copy()
    lengths[0] = Ti
    if N > 1:
        lengths[-1] = max(2, Ti - 12)              # ragged
    return inputs, lengths


def _run(m, inputs, lengths, spk=None, persistent=True):
    m.use_decode_kernel = persistent
    m.initialize(inputs, lengths, spk)
    m.check_status()
    assert m.last_paths["decode"] == ("persistent" if persistent else "step"), m.last_paths
    torch.cuda.synchronize()
    return {k: getattr(m, k).detach().float().cpu().numpy().copy()
            for k in ("decoder_outputs", "mel_outputs", "linear_outputs", "alignments")}


def _oracle(m, hp, inputs, lengths, steps, spk=None):
    from oracle import taco1_oracle as O
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in list(m.numpy_params().items()) + list(m.numpy_stats().items())}
    with torch.no_grad():
        out = O.taco1_forward(p, hp.values(), torch.tensor(inputs), torch.tensor(lengths), max_iters=steps,
                              speaker_ids=None if spk is None else torch.tensor(spk))
    return {k: out[k].numpy() for k in ("mel_outputs", "linear_outputs", "alignments")}


def _check_rows(al, lengths):
    # alignments [N, Ti, S]: every step's weights sum to 1 over the valid positions, zero past the length
    s = al.sum(axis=1)
    assert np.abs(s - 1.0).max() < 1e-4, np.abs(s - 1.0).max()
    for n, L in enumerate(lengths):
        assert np.abs(al[n, L:]).max(initial=0.0) == 0.0


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("mode", ["fp32", "mixed", "bf16x3", "bf16"])
def test_persistent_matches_step_loop(dev, mode, N):
    from nspeech_amd.models import create_model
    hp = _hp(40)
    m = create_model("taco1", hp, device="cuda:0", dtype=mode, seed=3)
    inputs, lengths = _batch(hp, N, 37, seed=N + 50)
    a = _run(m, inputs, lengths, persistent=True)
    b = _run(m, inputs, lengths, persistent=False)
    errs = {k: rel_max(a[k], b[k]) for k in ("decoder_outputs", "mel_outputs", "alignments")}
    print("\ntaco1 decode %s N=%d: persistent vs step %s" % (mode, N, {k: float("%.2e" % v) for k, v in errs.items()}))
    for k, v in errs.items():
        assert v < LOOP_BOUNDS[mode], (k, v)
    assert all(np.isfinite(x).all() for x in a.values())
    _check_rows(a["alignments"], lengths)


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("mode", ["fp32", "mixed"])
def test_persistent_matches_oracle(dev, mode, N):
    from nspeech_amd.models import create_model
    hp = _hp(40)
    m = create_model("taco1", hp, device="cuda:0", dtype=mode, seed=4)
    inputs, lengths = _batch(hp, N, 37, seed=N + 60)
    a = _run(m, inputs, lengths, persistent=True)
    want = _oracle(m, hp, inputs, lengths, 40)
    errs = {k: rel_max(a[k], want[k]) for k in want}
    print("\ntaco1 decode %s N=%d: persistent vs oracle %s" % (mode, N, {k: float("%.2e" % v) for k, v in errs.items()}))
    for k, v in errs.items():
        assert v < ORACLE_BOUNDS[mode], (k, v)


def test_persistent_with_speakers(dev):
    from nspeech_amd.models import create_model
    hp = _hp(40, speakers=3)
    m = create_model("taco1", hp, device="cuda:0", dtype="fp32", seed=7)
    _spread_speaker_path(m)
    inputs, lengths = _batch(hp, 2, 37, seed=71)
    spk = np.array([2, 1], np.int32)
    a = _run(m, inputs, lengths, spk, persistent=True)
    b = _run(m, inputs, lengths, spk, persistent=False)
    want = _oracle(m, hp, inputs, lengths, 40, spk)
    loop = {k: rel_max(a[k], b[k]) for k in ("mel_outputs", "alignments")}
    orc = {k: rel_max(a[k], want[k]) for k in want}
    print("\ntaco1 decode speakers: vs step %s, vs oracle %s" % (loop, orc))
    assert max(loop.values()) < LOOP_BOUNDS["fp32"], loop
    assert max(orc.values()) < ORACLE_BOUNDS["fp32"], orc
    c = _run(m, inputs, lengths, np.array([0, 0], np.int32), persistent=True)
    assert np.abs(c["mel_outputs"] - a["mel_outputs"]).max() > 1e-4      # the speaker changes the output


def test_persistent_full_length(dev):
    """The shipped max_iters = 300 at T_in = 160: the only check of a long feedback chain."""
    from nspeech_amd.models import create_model
    hp = _hp(300)
    m = create_model("taco1", hp, device="cuda:0", dtype="mixed", seed=9)
    inputs, lengths = _batch(hp, 2, 160, seed=81)
    a = _run(m, inputs, lengths, persistent=True)
    b = _run(m, inputs, lengths, persistent=False)
    assert a["mel_outputs"].shape == (2, 300 * hp.outputs_per_step, hp.num_mels)
    assert all(np.isfinite(x).all() for x in a.values())
    errs = {k: rel_max(a[k], b[k]) for k in ("decoder_outputs", "mel_outputs", "alignments")}
    print("\ntaco1 decode full length: persistent vs step %s" % errs)
    for k, v in errs.items():
        assert v < LOOP_BOUNDS["mixed"], (k, v)


def test_persistent_repeatable(dev):
    from nspeech_amd.models import create_model
    hp = _hp(40)
    m = create_model("taco1", hp, device="cuda:0", dtype="mixed", seed=5)
    inputs, lengths = _batch(hp, 2, 37, seed=91)
    m.use_decode_kernel = True
    outs = []
    for _ in range(3):
        m.initialize(inputs, lengths)
        m.check_status()
        assert m.last_paths["decode"] == "persistent"
        outs.append([getattr(m, k).clone() for k in ("decoder_outputs", "mel_outputs", "alignments")])
    for o in outs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(outs[0], o))


def test_unsupported_shape_takes_the_step_loop(dev):
    """T_in > 256 does not fit the clusters' LDS images: the step loop runs and still matches the oracle."""
    from nspeech_amd.models import create_model
    hp = _hp(3)
    m = create_model("taco1", hp, device="cuda:0", dtype="fp32", seed=6)
    inputs, lengths = _batch(hp, 1, 260, seed=95)
    a = _run(m, inputs, lengths, persistent=False)
    m.use_decode_kernel = True
    m.initialize(inputs, lengths)
    assert m.last_paths["decode"] == "step"
    want = _oracle(m, hp, inputs, lengths, 3)
    assert rel_max(m.mel_outputs.cpu().numpy(), want["mel_outputs"]) < 2e-3
    assert np.array_equal(m.mel_outputs.cpu().numpy(), a["mel_outputs"])
