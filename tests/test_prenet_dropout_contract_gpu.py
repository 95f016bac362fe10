"""Prenet dropout inside the attention recurrences (ns_taco2_attn_params.drop_* / ns_taco1_attn_params.drop_*) and
ns_dropout_rows, through nspeech_amd.ops against tests/prenet_dropout_ref.py only (itself proven by
tests/test_prenet_dropout_ref_cpu.py, which also shows that every planted error of that module moves a buffer compared
here by more than ten of its bounds - on the cases, data seeds and mask seeds below).

  cluster2  ns_taco2_attn_cluster_fwd / _bwd (csrc/attn_cluster.hip), A = 64 and 256, fp32 and bf16 storage
  cluster1  ns_taco1_attn_cluster_fwd / _bwd (csrc/attn_gru.hip), fp32 and bf16 storage
  step2     ns_taco2_attn_fwd / _bwd (csrc/attn.hip: ns_dropout_rows between the step launches), plain and
            projected-memory form at the small widths of tests/test_attn_contract_gpu.py, fp32, F32_PASSES 0
each at rate 0.5 (scale exactly 2) and 0.1 (scale inexact in fp32) on the shapes, by their names there: n3s4t9, n1s1t1,
n4s9t20-spk-clip (speaker rows between p2 and h), n33s2t9 / n32s2t9 (a second launch group: n is the row of the batch)
and n2s5t70-kw8.

Everything around a launch is tests/test_attn_contract_gpu.py's own run_recurrence() (padded memory rows, frozen inputs,
slot 0 zero, two launches of a persistent kernel on one work buffer with status word 0, every valid element compared),
with the four drop_* fields added to every parameter block it builds.  The tolerances are that module's fp32 rule and
bf16 rule, unchanged: its _references() is evaluated on this module's inputs with the dropout reference in the place of
attn_ref's, so every bound is computed per case from the float32 / storage-exact emulations of the reference WITH the
masks.  Every case walks its data seed until no prenet pre-activation lies within 100 bounds of zero, as there.

Exact checks on top: the stored p1 and xa[:, :, :D2] are 0 at every dropped unit and nowhere else where the reference is
positive; the two launches of a persistent kernel give bit-identical buffers; other seeds give the zero pattern the
generator states for them; drop_thr = 0 beside non-zero seeds and scale is bit-identical to a block that never set the
fields; both decode entry points refuse a block with drop_thr != 0."""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

import prenet_dropout_ref as PR
import test_attn_contract_gpu as TC

pytestmark = pytest.mark.gpu

f32, bf = torch.float32, torch.bfloat16
RATES = (0.5, 0.1)
SEED1, SEED2 = 0x243F6A88, 0x85A308D3             # the two layers' streams in every case below
OTHER1, OTHER2 = 0x13198A2E, 0x03707344           # "another seed"
SHAPE_NAMES = ("n3s4t9", "n1s1t1", "n4s9t20-spk-clip", "n33s2t9", "n2s5t70-kw8")
SHAPE_NAMES1 = tuple("n32s2t9" if n == "n33s2t9" else n for n in SHAPE_NAMES)      # the Tacotron-1 launch holds 32 rows

DCase = namedtuple("DCase", "c rate")


def drop_of(rate, seed1=SEED1, seed2=SEED2):
    return dict(thr=PR.threshold(rate), scale=PR.scale_of(rate), seed1=seed1, seed2=seed2)


def _shape(pool, name):
    return next(s for s in pool if s.name == name)


def _dcases():
    out = []
    for rate in RATES:
        for A in (64, 256):
            for dtype in (f32, bf):
                for n in SHAPE_NAMES:
                    out.append(DCase(TC.Case("cluster2", "A%d-%s" % (A, "f32" if dtype == f32 else "bf16"), A, 16, 256, 128, dtype, 0, 0,
                                             True, _shape(TC.SHAPES, n)), rate))
        for dtype in (f32, bf):
            for n in SHAPE_NAMES1:
                out.append(DCase(TC.Case("cluster1", "f32" if dtype == f32 else "bf16", 256, 16, 256, 128, dtype, 0, 0, True,
                                         _shape(TC.SHAPES1, n)), rate))
        for pv in (False, True):
            for n in SHAPE_NAMES:
                out.append(DCase(TC.Case("step2", "%s-f32x00" % ("pv" if pv else "plain"), 8 if n == "n1s1t1" else 24, 8, 16, 8, f32, 0, 0,
                                         pv, _shape(TC.SHAPES, n)), rate))
    return out


ALL_DCASES = _dcases()


def dcase_id(dc):
    return "%s-rate%g" % (TC.case_id(dc.c), dc.rate)


def ref_fn(dc, drop=None):
    fn = PR.taco1 if dc.c.family == "cluster1" else PR.taco2
    return functools.partial(fn, drop=drop_of(dc.rate) if drop is None else drop)


@functools.lru_cache(maxsize=None)
def _dinputs(key, rate):
    """As test_attn_contract_gpu._inputs, with the masks in the reference: (x, dhc, pure, seed, emu32)."""
    dc = next(d for d in ALL_DCASES if TC._data_key(d.c) == key and d.rate == rate)
    c = dc.c
    fn = ref_fn(dc)
    base = 1000 * c.A + 17 * c.shape.N + 3 * c.shape.S + c.shape.Ti + c.shape.kw
    for seed in range(base, base + 64):
        x, dhc = TC._draw(c, seed)
        pure = fn(x, dhc)
        emu32 = fn(x, dhc, dtype=torch.float32, perm_seed=c.shape.N + c.shape.Ti)
        if all(got >= need for got, need in TC.kink_margin(c, pure, emu32).values()):
            return x, dhc, pure, seed, emu32
    raise AssertionError("no seed keeps the prenet pre-activations of %s away from zero" % dcase_id(dc))


def dinputs(dc):
    return _dinputs(TC._data_key(dc.c), dc.rate)


_REFS = {}


def dreferences(dc, monkeypatch):
    """test_attn_contract_gpu._references (the two rules, unchanged and uncached) on this module's inputs and reference."""
    key = (TC._data_key(dc.c), TC.rule_of(dc.c)["grad"], dc.c.pv, dc.rate)
    if key not in _REFS:
        monkeypatch.setattr(TC, "inputs", lambda c: dinputs(dc))
        monkeypatch.setattr(TC, "_ref_fn", lambda c: ref_fn(dc))
        _REFS[key] = TC._references.__wrapped__(*key[:3])
    return _REFS[key]


HIST_OUT = ("p1", "xa", "xc", "hc", "ca", "ga", "ru", "cc", "q", "align")
GRAD_OUT = ("df1", "dp2", "dga", "dzg", "dzc", "dq", "de")


def run_with(monkeypatch, c, fields, inputs=None):
    """TC.run_recurrence(c) with `fields` (drop_* of the parameter blocks, or {}) in every block it builds and, with
    `inputs`, on those operands instead of the module's own.  Returns (got, launches): the outputs, and for a persistent
    kernel {direction: [snapshot of every buffer the launch writes, one per launch]}."""
    from nspeech_amd import ops
    dev = torch.device("cuda:0")
    if inputs is not None:
        monkeypatch.setattr(TC, "inputs", lambda c_: inputs)
    for name in ("_attn_params", "_taco1_attn_params"):
        orig = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda kw, orig=orig: orig(dict(kw, **fields)))
    launches = {"fwd": [], "bwd": []}
    for name in ("taco2_attn_cluster", "taco1_attn_cluster"):
        orig = getattr(ops, name)

        def run(direction, cluster_work, _orig=orig, **kw):          # (kw holds the step forms' own `work`)
            _orig(direction, cluster_work, **kw)
            torch.cuda.synchronize()
            names = HIST_OUT if direction == "fwd" else GRAD_OUT
            launches[direction].append({k: kw[k].clone() for k in names if kw.get(k) is not None})
        monkeypatch.setattr(ops, name, run)
    got = TC.run_recurrence(c, dev)
    monkeypatch.undo()
    return got, launches


def fields_of(drop):
    return dict(drop_thr=drop["thr"], drop_scale=drop["scale"], drop_seed1=drop["seed1"], drop_seed2=drop["seed2"])


def check_zero_pattern(c, got, ref):
    """p1 / p2 are exactly 0 at every dropped unit, and nowhere else where the reference is positive."""
    for buf, keep, width in (("p1", "keep1", c.D1), ("xa", "keep2", c.D2)):
        g, r, k = got[buf][..., :width], TC._cut(c, buf, ref[buf])[..., :width], ref[keep]
        assert k.shape == g.shape, (k.shape, g.shape)
        assert float(g[~k].abs().max() if bool((~k).any()) else 0.0) == 0.0, "%s: a dropped unit is not 0" % buf
        live = k & (r > 0)
        assert bool((g[live] > 0).all()), "%s: a kept unit with a positive reference is 0" % buf
        assert bool(live.any()) and bool((~k).any()) or c.shape.name == "n1s1t1", "%s: the case drops or keeps nothing" % buf


def check_dcase(monkeypatch, dc):
    c = dc.c
    refs = dreferences(dc, monkeypatch)
    monkeypatch.undo()
    drop = drop_of(dc.rate)
    got, launches = run_with(monkeypatch, c, fields_of(drop), inputs=dinputs(dc))
    print("%s: data seed %d, dropped share p1 %.3f p2 %.3f" % (dcase_id(dc), dinputs(dc)[3], 1 - float(refs["pure"]["keep1"].float().mean()),
                                                               1 - float(refs["pure"]["keep2"].float().mean())))
    TC.check(c, got, refs, TC.hist_names(c) + TC.grad_names(c), dcase_id(dc))
    check_zero_pattern(c, got, refs["pure"])
    if c.family != "step2":
        for direction, snaps in launches.items():
            assert len(snaps) == 2, (direction, len(snaps))
            for k in snaps[0]:
                assert TC._same(snaps[0][k], snaps[1][k]), "%s %s: the second launch on the same work buffer differs" % (direction, k)


@pytest.mark.parametrize("dc", [d for d in ALL_DCASES if d.c.family == "cluster2"], ids=dcase_id)
def test_taco2_cluster_with_dropout_meets_the_contract(dev, monkeypatch, dc):
    check_dcase(monkeypatch, dc)


@pytest.mark.parametrize("dc", [d for d in ALL_DCASES if d.c.family == "cluster1"], ids=dcase_id)
def test_taco1_cluster_with_dropout_meets_the_contract(dev, monkeypatch, dc):
    check_dcase(monkeypatch, dc)


@pytest.mark.parametrize("dc", [d for d in ALL_DCASES if d.c.family == "step2"], ids=dcase_id)
def test_step_kernels_with_dropout_meet_the_contract(dev, monkeypatch, dc):
    check_dcase(monkeypatch, dc)


def _first(family, form, shape, rate=0.5):
    return next(d for d in ALL_DCASES if d.c.family == family and d.c.form == form and d.c.shape.name == shape and d.rate == rate)


SMALL = [_first("cluster2", "A64-f32", "n3s4t9"), _first("cluster1", "f32", "n3s4t9"), _first("step2", "pv-f32x00", "n3s4t9")]


@pytest.mark.parametrize("dc", SMALL, ids=dcase_id)
def test_another_seed_gives_another_zero_pattern(dev, monkeypatch, dc):
    """The zeros follow the seeds: with other seeds p1 / p2 are zero exactly where the generator says for THOSE seeds, and
    that is another pattern."""
    c = dc.c
    x, dhc = dinputs(dc)[:2]
    other = drop_of(dc.rate, OTHER1, OTHER2)
    ref = ref_fn(dc, other)(x, dhc)
    got, _ = run_with(monkeypatch, c, fields_of(other), inputs=dinputs(dc))
    check_zero_pattern(c, got, ref)
    first = dinputs(dc)[2]
    assert not torch.equal(ref["keep1"], first["keep1"]) and not torch.equal(ref["keep2"], first["keep2"])
    assert not torch.equal(got["p1"] == 0, TC._cut(c, "p1", first["p1"]) == 0)


@pytest.mark.parametrize("dc", SMALL, ids=dcase_id)
def test_threshold_zero_is_bit_identical_to_unset_fields(dev, monkeypatch, dc):
    """drop_thr = 0 is off whatever the seeds and the scale hold: every output equals, bit for bit, that of parameter
    blocks whose four fields were never set (on the operands of tests/test_attn_contract_gpu.py's own case)."""
    c = dc.c
    plain, _ = run_with(monkeypatch, c, {})
    off, _ = run_with(monkeypatch, c, dict(drop_thr=0, drop_scale=2.0, drop_seed1=SEED1, drop_seed2=SEED2))
    assert sorted(plain) == sorted(off)
    for k in plain:
        assert torch.equal(plain[k], off[k]), k


# ------------------------------------------------------------------------------------------------------ ns_dropout_rows
# N, T, U, row stride sn, step stride st (elements), column offset of the block, dtype, t0, n0, rate, in place
Rows = namedtuple("Rows", "N T U sn st off dtype t0 n0 rate inplace")
ROWS = [Rows(3, 5, 128, 5 * 128, 128, 0, f32, 0, 0, 0.5, True),           # contiguous, vector path, in place
        Rows(3, 5, 128, 5 * 128, 128, 0, bf, 0, 0, 0.5, False),
        Rows(4, 3, 37, 3 * 53, 53, 8, f32, 7, 33, 0.1, True),             # U no multiple of the vector width, odd strides, margins
        Rows(4, 3, 37, 3 * 53, 53, 8, bf, 7, 33, 0.1, False),
        Rows(35, 1, 24, 2 * 40, 0, 8, f32, 4, 32, 0.5, True),             # one step's rows of a slot layout (the step forms' call)
        Rows(2, 6, 16, 6 * 24, 24, 4, bf, 2, 0, 0.1, True),               # vector width met inside a wider row, bf16 in place
        Rows(2, 300, 256, 300 * 256, 256, 0, f32, 0, 0, 0.5, False)]      # more than one pass of the grid-stride loop


def rows_id(r):
    return "N%d-T%d-U%d-sn%d-st%d-off%d-%s-t%d-n%d-rate%g%s" % (r.N, r.T, r.U, r.sn, r.st, r.off, "f32" if r.dtype == f32 else "bf16", r.t0,
                                                                r.n0, r.rate, "-inplace" if r.inplace else "")


def rows_inputs(r):
    g = torch.Generator().manual_seed(r.N * 1000 + r.T * 10 + r.U)
    x = torch.randn(r.N, r.T, r.U, generator=g)
    x = torch.where(x >= 0, 1.0, -1.0) * (0.25 + x.abs())           # no input is 0: a zero in the output is a dropped unit
    return x.to(r.dtype).float()


def rows_layout(r, x, dev):
    """x [N, T, U] inside a buffer of sentinels at element n * sn + t * st + off + u (st = 0: T = 1)."""
    size = (r.N - 1) * r.sn + (r.T - 1) * r.st + r.off + r.U + TC.MARGIN
    full = torch.full((size,), TC.SENTINEL, dtype=torch.float32)
    idx = (torch.arange(r.N)[:, None, None] * r.sn + torch.arange(r.T)[None, :, None] * r.st + r.off + torch.arange(r.U)[None, None, :])
    full[idx.reshape(-1)] = x.reshape(-1)
    return full.to(r.dtype).to(dev), idx


@pytest.mark.parametrize("r", ROWS, ids=rows_id)
def test_dropout_rows_meets_its_contract(dev, r):
    from nspeech_amd import ops
    x = rows_inputs(r)
    thr, scale = PR.threshold(r.rate), PR.scale_of(r.rate)
    want, keep = PR.dropout_rows(x, SEED1, thr, scale, t0=r.t0, n0=r.n0)
    src, idx = rows_layout(r, x, dev)
    before = src.clone()
    dst = src if r.inplace else torch.full_like(src, TC.SENTINEL)
    ops.dropout_rows(src, r.N, r.T, r.U, r.sn, r.st, thr, SEED1, scale, t0=r.t0, n0=r.n0, x_off=r.off, y=None if r.inplace else dst,
                     y_off=r.off)
    torch.cuda.synchronize()
    if not r.inplace:
        assert TC._same(src, before), "the input changed"
    out = dst.float().cpu()
    got = out[idx.reshape(-1)].view(r.N, r.T, r.U)
    rest = torch.ones(out.numel(), dtype=torch.bool)
    rest[idx.reshape(-1)] = False
    assert bool((out[rest] == (TC.SENTINEL if not r.inplace else before.float().cpu()[rest])).all()), "written outside the U columns"
    # zeros exactly where the restated generator says
    assert torch.equal(got == 0, ~keep), "the zero pattern is not the generator's"
    assert 0 < int((~keep).sum()) < keep.numel()
    # one fp32 multiplication, rounded once to the storage type
    exact = (x * torch.tensor(scale, dtype=torch.float32)).to(r.dtype).float() * keep.float()
    assert torch.equal(got, exact), float((got - exact).abs().max())
    assert float((got.double() - want).abs().max()) <= (2.0 ** -8 if r.dtype == bf else 2.0 ** -23) * float(want.abs().max())
    # forward = backward: the same call on a gradient of the same layout gives the same mask and scale
    gsrc, _ = rows_layout(r, torch.ones(r.N, r.T, r.U), dev)
    ops.dropout_rows(gsrc, r.N, r.T, r.U, r.sn, r.st, thr, SEED1, scale, t0=r.t0, n0=r.n0, x_off=r.off)
    torch.cuda.synchronize()
    gg = gsrc.float().cpu()[idx.reshape(-1)].view(r.N, r.T, r.U)
    assert torch.equal(gg, keep.float() * torch.tensor(scale, dtype=torch.float32).to(r.dtype).float())


# ------------------------------------------------------------------------------------------------------ decode refusal
def test_both_decode_entry_points_refuse_a_dropout_block(dev, monkeypatch):
    """Dropout is a training option: ns_taco2_decode / ns_taco1_decode answer NS_ERR_BAD_ARG to att.drop_thr != 0 and
    launch nothing (the same synthesis call goes through the persistent decoder when the fields are unset)."""
    from nspeech_amd import _lib as L
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd import ops
    from nspeech_amd.models import create_model
    from util import make_batch, small_hparams
    hp2 = small_hparams(max_iters=3)
    hp1 = hparams_mod.load("taco1")
    hp1.max_iters = 3
    for kind, hp, fn in (("taco2", hp2, "_attn_params"), ("taco1", hp1, "_taco1_attn_params")):
        m = create_model(kind, hp, device="cuda:0", dtype="fp32", seed=1)
        inputs, lengths, _, _ = make_batch(hp, 2, 9, 10, seed=3)
        m.initialize(inputs, lengths)
        assert m.last_paths["decode"] == "persistent", m.last_paths
        m.check_status()
        orig = getattr(ops, fn)
        monkeypatch.setattr(ops, fn, lambda kw, orig=orig: orig(dict(kw, **fields_of(drop_of(0.5)))))
        with pytest.raises(L.NSError, match=r"\(-1\).*prenet dropout"):
            m.initialize(inputs, lengths)
        monkeypatch.undo()
