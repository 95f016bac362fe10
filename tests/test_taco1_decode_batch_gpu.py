"""Tacotron-1 free-running synthesis above two utterances: ns_taco1_decode runs the rows of a batch as groups of two,
every group with its own 16 decoder workgroups in one grid, and splits a batch above ns_taco1_decode_max_rows() into
balanced launches (csrc/attn_gru.hip "free-running synthesis").  At the shipped widths of hparams/taco1.yaml, T_in = 37
with lengths that differ within and across the groups, 12 decoder steps unless stated.  The per-row arithmetic is that
of the N <= 2 kernel, so the bounds are those of test_taco1_decode_gpu.py, unchanged.  Every test takes the persistent
path (`_run` asserts last_paths["decode"]) and reads the status word."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_taco1_decode_gpu import LOOP_BOUNDS, ORACLE_BOUNDS, _check_rows, _hp, _oracle, _run, _spread_speaker_path
from util import rel_max

pytestmark = pytest.mark.gpu

STEPS, TI = 12, 37


def _ragged(N, Ti, seed):
    """N texts of Ti ids; lengths Ti, Ti - 5, Ti - 10, ... (mod 29): no two rows of a group, and no two neighbouring
    groups, share a length."""
    rng = np.random.RandomState(seed)
    lengths = np.array([max(2, Ti - (5 * n) % 29) for n in range(N)], np.int32)
    inputs = np.zeros((N, Ti), np.int32)
    for n in range(N):
        inputs[n, :lengths[n] - 1] = rng.randint(2, 64, size=lengths[n] - 1)
        inputs[n, lengths[n] - 1] = 1
    return inputs, lengths


@functools.lru_cache(maxsize=None)
def _model(mode, steps=STEPS, speakers=1, seed=3):
    from nspeech_amd.models import create_model
    m = create_model("taco1", _hp(steps, speakers), device="cuda:0", dtype=mode, seed=seed)
    if speakers > 1:
        _spread_speaker_path(m)
    return m


def _max_rows():
    from nspeech_amd import _lib
    fn = _lib.lib().ns_taco1_decode_max_rows
    fn.restype, fn.argtypes = ctypes.c_int, []
    return int(fn())


def _against_step_loop(m, mode, inputs, lengths, what, spk=None):
    a = _run(m, inputs, lengths, spk, persistent=True)
    b = _run(m, inputs, lengths, spk, persistent=False)
    errs = {k: rel_max(a[k], b[k]) for k in ("decoder_outputs", "mel_outputs", "alignments")}
    print("\ntaco1 batched decode %s %s: persistent vs step %s" % (what, mode, {k: float("%.2e" % v) for k, v in errs.items()}))
    for k, v in errs.items():
        assert v < LOOP_BOUNDS[mode], (k, v)
    assert all(np.isfinite(x).all() for x in a.values())
    _check_rows(a["alignments"], lengths)
    return a, b


@pytest.mark.parametrize("N", [3, 4, 5])
@pytest.mark.parametrize("mode", ["fp32", "mixed", "bf16"])
def test_groups_match_step_loop(dev, mode, N):
    """N = 3: a full group and a one-row tail group; 4: two full groups; 5: both."""
    inputs, lengths = _ragged(N, TI, seed=N + 100)
    _against_step_loop(_model(mode), mode, inputs, lengths, "N=%d" % N)


@pytest.mark.parametrize("mode", ["fp32", "mixed"])
def test_groups_match_oracle(dev, mode):
    m = _model(mode)
    inputs, lengths = _ragged(5, TI, seed=111)
    a = _run(m, inputs, lengths, persistent=True)
    want = _oracle(m, _hp(STEPS), inputs, lengths, STEPS)
    errs = {k: rel_max(a[k], want[k]) for k in want}
    print("\ntaco1 batched decode %s N=5: persistent vs oracle %s" % (mode, {k: float("%.2e" % v) for k, v in errs.items()}))
    for k, v in errs.items():
        assert v < ORACLE_BOUNDS[mode], (k, v)


@pytest.mark.parametrize("extra", [0, 1])
def test_full_launch_and_split(dev, extra):
    """N = max_rows: one launch (on 256 CUs: 256 workgroups, one per CU); N = max_rows + 1: two balanced launches that
    share the status word."""
    cap = _max_rows()
    assert cap > 0 and cap % 2 == 0
    N = cap + extra
    inputs, lengths = _ragged(N, TI, seed=120 + extra)
    _against_step_loop(_model("mixed"), "mixed", inputs, lengths, "N=%d (max_rows %d)" % (N, cap))


def test_speakers_in_groups(dev):
    m = _model("fp32", speakers=3, seed=7)
    hp = _hp(STEPS, speakers=3)
    inputs, lengths = _ragged(3, TI, seed=131)
    spk = np.array([2, 0, 1], np.int32)
    a, _ = _against_step_loop(m, "fp32", inputs, lengths, "speakers", spk)
    want = _oracle(m, hp, inputs, lengths, STEPS, spk)
    orc = {k: rel_max(a[k], want[k]) for k in want}
    print("\ntaco1 batched decode speakers: vs oracle %s" % orc)
    assert max(orc.values()) < ORACLE_BOUNDS["fp32"], orc
    # another speaker in the tail group (row 2, a group of its own): that row's mel changes, the first group's does not
    c = _run(m, inputs, lengths, np.array([2, 0, 0], np.int32), persistent=True)
    assert np.array_equal(c["mel_outputs"][:2], a["mel_outputs"][:2])
    assert np.abs(c["mel_outputs"][2] - a["mel_outputs"][2]).max() > 1e-4


def test_no_leakage_across_groups(dev):
    m = _model("mixed")
    inputs, lengths = _ragged(2, TI, seed=141)
    inputs, lengths = np.concatenate([inputs, inputs]), np.concatenate([lengths, lengths])
    m.use_decode_kernel = True
    m.initialize(inputs, lengths)
    m.check_status()
    assert m.last_paths["decode"] == "persistent"
    Pi = m.dims["Pi"]
    mem = m._bufs["a:enc_out"][:4 * Pi * 256].view(4, Pi, 256)
    assert torch.equal(mem[:2], mem[2:])            # the encoder is row-independent: the two groups read the same memory
    for k in ("decoder_outputs", "alignments"):
        x = getattr(m, k)
        assert torch.equal(x[:2], x[2:]), k


def test_repeated_calls_are_bit_equal(dev):
    m = _model("mixed")
    inputs, lengths = _ragged(5, TI, seed=151)
    m.use_decode_kernel = True
    outs = []
    for _ in range(3):
        m.initialize(inputs, lengths)
        m.check_status()
        assert m.last_paths["decode"] == "persistent"
        outs.append([getattr(m, k).clone() for k in ("decoder_outputs", "mel_outputs", "alignments")])
    for o in outs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(outs[0], o))


def test_long_chain_across_groups(dev):
    """The shipped max_iters = 300 at T_in = 160 over two groups.  Measured on one MI355X: mel 4.3e-5, align 4.7e-7
    (N = 2 in test_taco1_decode_gpu.py: 3.5e-5) against the bound 1e-4."""
    m = _model("mixed", steps=300, seed=9)
    inputs, lengths = _ragged(4, 160, seed=161)
    a, _ = _against_step_loop(m, "mixed", inputs, lengths, "300 steps N=4")
    assert a["mel_outputs"].shape == (4, 300 * _hp(300).outputs_per_step, _hp(300).num_mels)


def test_synthesize_batch_takes_the_persistent_path(dev):
    from nspeech_amd.synthesizer import Synthesizer
    synth = Synthesizer(_hp(STEPS), dtype="mixed").load(None, "taco1")
    texts = ["Hello, World.", "Dr. Jones arrived at 9 o'clock.", "Yes.", "The quick brown fox.", "No, thank you."]
    one = synth.synthesize(texts[0])
    got = synth.synthesize_batch(texts)
    synth.model.check_status()
    assert synth.model.last_paths["decode"] == "persistent"
    assert len(got) == 5
    for wav, mel, lin in got:
        assert wav.ndim == 1 and wav.dtype == one[0].dtype and np.isfinite(wav).all()
        assert mel.shape == one[1].shape and mel.dtype == one[1].dtype
        assert lin.shape == one[2].shape and lin.dtype == one[2].dtype
