"""Every kernel of csrc/wavenet.hip and every generator engine against the float64 contract of tests/wavenet_ref.py
(itself proven by tests/test_wavenet_ref_cpu.py), through nspeech_amd.ops and the models.  Errors are measured against
the references, never against another kernel; every element is compared; no draw is excused.

Pieces (ns_wavenet_input forward / backward, ns_wavenet_gate forward / backward, ns_wavenet_softmax_ce,
ns_wavenet_softmax), called directly: outputs sit between sentinel margins (MARGIN elements of SENTINEL on either side,
and in the columns a stride leaves out), `+=` outputs are prefilled, inputs are bit-identical afterwards.

Generator forms, through model.generate: the returned ids equal the reference's free run EXACTLY - the uniform numbers
of a case keep 2 x the case's CDF bound away from every CDF edge of the reference (wavenet_ref.safe_uniforms; the CPU
module asserts the margin) - last_probs is within the bounds below, the seeds are untouched and a second call gives the
same bits.  Every case runs B = 3 waveforms (engine 3 also B = 1) from seeds of rf + 1 and of rf + 5 samples, 24 draws;
last_probs is read behind draws 8, 16 and 24 (one call each on the same uniform numbers: three distributions per waveform
decide more than one).  Parameters: wavenet_ref.init_params (its gains by depth keep the distributions structured and the
margins possible); the 66-layer cases (33 x dilations 1, 2: receptive field 101) reach the ring rows of layers 64 and 65.

bf16 training pass (simple_wavenet, and wavenet with biases and a held local condition): the logits, the loss and every
gradient, over every element, against `train_bf16` and `pure` by the bf16 rule.

Tolerances (all from the references or from the project's existing fp32 tests, none from a kernel's output):
  fp32 rule  - fp32 storage, unrounded computed operands.  gate and input forward 1e-6 absolute (x the largest |dout| in
               the gate's backward: the same arithmetic times dout); probabilities 1e-5; loss 1e-5 max(1, |loss|);
               atomically summed dw and fp32 gradients 1e-4 x the variable's largest reference value.  Against `pure` for
               the fp32 forms, against `w_bf16` for the per-layer kernel on the bf16 shadow and engine 1.  CDF bound:
               Q / 2 x 1e-5 (a CDF value is a sum of at most Q probabilities whose errors sum to zero).
  bf16 store - a single value stored as bf16 equals bf16(reference), or the neighbouring bf16 value where the float64
               reference lies within the buffer's fp32-rule bound (the band) of a rounding boundary: the value lies
               between bf16(reference - band) and bf16(reference + band).  At most 1 % neighbours, COUNTED WHERE bf16 IS
               COARSER THAN THE BAND (spacing at the reference >= 4 x band, bf16_coarse()): the bands are absolute, and
               below that magnitude (1e-3 at 1e-6) most references lie within the band of some boundary, so a count would
               say nothing - there a value is held to the band plus the bf16 step it is stored with.  The CPU module shows
               that fewer than 1 % of the references of 2^-5 and more lie inside the band.
  bf16 rule  - engines 2 and 3, the rule of test_lstm_contract_gpu.py: against the storage-exact preset (`mfma`)
               max <= 2 x and mean <= 10 x what a float32 emulation of the arrangement with every product summed in a
               permuted order differs from it by at this case; floors: 2 x one_flip() (max) and the fp32 rule (mean).
               Against `pure`: max <= 4 x and mean <= 2 x the storage-exact preset's own distance.  one_flip() below: the
               largest change of the compared quantity when the largest-magnitude rounded value at a rounding point (the
               filter | gate operand, the dense operand) of the first, a middle and the last layer moves to its bf16
               neighbour.  The CDF bound is the same rule on max_j |cdf(j)| over all 24 draws.
  ns_wavenet_softmax: float32(reference) or its float32 neighbour.

Worst error / bound on the MI355X (every test prints its own, `pytest -s`):
  pieces, fp32 storage      input fwd x 0.24   input bwd dw < 0.01   gate out 0.12  dz 0.09   softmax_ce loss 0.10
                            dlogits < 0.01
  pieces, bf16 storage      neighbours / values: input fwd x 0 / 3808   gate out 0 / 18336  dz 1 / 36672
                            softmax_ce dlogits 0 / 37761 (every other value is bf16(reference))
  ns_wavenet_softmax        0 of 876 values are the float32 neighbour: all are float32(reference)
  generator, fp32 rule      exact (pure) 0.06   per-layer bf16 shadow (w_bf16) 0.03   engine 1 (w_bf16) 0.12
  generator, bf16 rule      max / mean against mfma;  max / mean against pure
    engine 2                0.16 / 0.31;  0.25 / 0.51        conditioned 0.15 / 0.18;  0.25 / 0.50
    engine 2, 66 layers     0.03 / 0.17;  0.27 / 0.55        with biases (S 512, Q 256) 0.42 / 0.16;  0.25 / 0.52
    engine 3                0.32 / 0.82;  0.30 / 0.55        66 layers 0.55 / 0.80;  0.29 / 0.53
                            (chain and helpers in one grid; the two-kernel form before it: the same figures, and the
                            same bits in ids and last_probs on every engine-3 case)
  every id of every run equals the reference's (34 cases x 2 seed lengths x 3 waveforms x 24 draws; engine 3 runs on
  every runtime configuration)
  bf16 training pass        max / mean against train_bf16;  against pure at most 0.27 / 0.50 throughout
    simple_wavenet          logits, loss < 0.01;  gradients at most 0.02 / 0.06 (filter)
    wavenet, biases + lc    logits 0.12 / 0.02   loss 0.11   gradients at most 0.25 / 0.08 (postprocess2_bias / gate)
0.25 / 0.50 against the pure reference is a kernel exactly as far from it as its arrangement is (the bounds are 4 x and
2 x that distance).
"""
import functools
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

import wavenet_ref as R

pytestmark = pytest.mark.gpu

f32, bf = torch.float32, torch.bfloat16
MARGIN = 8
SENTINEL = 7.0
N_DRAW = 24
SEED_EXTRA = (1, 5)                      # seeds of rf + 1 and rf + 5 samples
PROBES = (8, 16, 24)                     # last_probs is read behind these draws (one call each on the same uniforms)
PIDX = [n - 1 for n in PROBES]
HOLD = 3
DELTA_FACTOR = 3.0                       # the band safe_uniforms() keeps clear / the CDF bound of a first run without a band

# form -> (preset, rule, generate() keywords, last_engine)
FORMS = {
    "exact": ("pure", "f32", dict(exact=True), 0),
    "layer_bf16": ("w_bf16", "f32", dict(fast=False), 0),
    "engine1": ("w_bf16", "f32", dict(engine=1), 1),
    "engine2": ("mfma", "bf16", dict(engine=2), 2),
    "engine3": ("mfma", "bf16", dict(), 3),
}
Gen = namedtuple("Gen", "form R S Q depth length opts B")
Gen.__new__.__defaults__ = ("", 3)
GEN_CASES = (
    [Gen("exact", 16, 32, 64, 2, 3), Gen("exact", 32, 64, 64, 1, 5)] +
    [Gen("layer_bf16", 16, 32, 64, 2, 3), Gen("layer_bf16", 32, 64, 64, 1, 5), Gen("layer_bf16", 32, 64, 64, 2, 3, "biases+gc+lc")] +
    [Gen("engine1", C, 2 * C, 64, 1, L) for C in (16, 32) for L in (1, 2, 3, 4, 7)] +      # three layers of weights in flight
    [Gen("engine2", 32, S, 64, d, n) for S in (64, 512) for d, n in ((1, 1), (1, 2), (1, 3), (1, 5), (2, 4))] +
    [Gen("engine2", 32, 64, 64, 33, 2)] +                                                  # layers 64, 65: rr1 / MF_RROW
    [Gen("engine2", 32, 64, 64, 2, 4, o) for o in ("biases", "gc", "lc")] +
    [Gen("engine2", 32, 512, 256, 33, 2, "biases")] +
    [Gen("engine3", 32, 512, 256, d, n, "", B) for d, n in ((2, 4), (33, 2)) for B in (1, 3)])


def gen_id(c):
    return "%s-R%d-S%d-Q%d-%dx%d%s-B%d" % (c.form, c.R, c.S, c.Q, c.depth, c.length, "-" + c.opts if c.opts else "", c.B)


def hp_of(c):
    o = c.opts.split("+")
    return dict(dilations_depth=c.depth, dilations_length=c.length, quantization_channels=c.Q, residual_channels=c.R,
                dilation_channels=c.R, skip_channels=c.S, use_biases="biases" in o, gc_channels=4 if "gc" in o else 0,
                gc_category_cardinality=3 if "gc" in o else 0, lc_channels=5 if "lc" in o else 0, filter_width=2,
                scalar_input=False, initial_filter_width=32)


@functools.lru_cache(maxsize=None)
def gen_data(c, extra):
    """What the reference and model.generate are both given: parameters (float32), seeds, conditions."""
    hp = hp_of(c)
    rf = R.receptive_field(hp)
    rng = np.random.RandomState(1000 * c.R + 10 * c.depth + c.length + c.S + extra)
    n_seed = rf + extra
    d = dict(hp=hp, rf=rf, n_seed=n_seed, params=R.init_params(hp, 8), gc=None, lc=None, hold=1, t0=0,
             seeds=rng.randint(0, c.Q, size=(c.B, n_seed)).astype(np.int32))
    d["seeds"][0, -1], d["seeds"][-1, -2] = 0, c.Q - 1
    if hp["gc_channels"]:
        d["gc"] = rng.randint(0, 3, size=c.B)
    if hp["lc_channels"]:
        d["hold"], d["t0"] = HOLD, -(rf - 1)          # the seed's first rf - 1 positions stand in front of row 0
        rows = max(0, n_seed + N_DRAW - 1 + d["t0"]) // HOLD + 1
        d["lc"] = rng.randn(c.B, rows, hp["lc_channels"]).astype(np.float32)
    return d


def ref_kw(c, d, preset):
    p = R.as_params(d["params"])
    return p, dict(preset=preset, cond=R.cond_terms(p, d["hp"], preset, d["gc"], d["lc"]), hold=d["hold"], t0=d["t0"])


def _dist(a, b):
    x = (a.double() - b.double()).abs()
    return float(x.max()), float(x.mean())


FLIP_POINTS = ("x", "out")


def one_flip(p, hp, ids, probs, n_seed, L, kw):
    """The most that ONE rounded value moving to its bf16 neighbour changes the compared quantities: the largest-magnitude
    value at each rounding point (the filter | gate operand "x", the dense operand "out") of the first, a middle and the
    last layer is flipped in turn.  Returns (largest change of a probed distribution - the flipped value sits on the last
    row of that draw's window -, largest change of a CDF value over all draws - the value sits on any draw's row)."""
    rf = R.receptive_field(hp)
    flip_p = flip_c = 0.0
    for l in sorted({0, L // 2, L - 1}):
        for pt in FLIP_POINTS:
            for n in PROBES:
                end = n_seed + n - 1
                one = R.network(p, hp, torch.as_tensor(ids[:, end - rf:end]).long(), pos0=end - rf, flip=(l, pt), **kw)
                flip_p = max(flip_p, _dist(R.softmax64(one[:, -1]), probs[:, n - 1])[0])
            run = R.run_probs(p, hp, ids, N_DRAW, flip=(l, pt), **kw)
            flip_c = max(flip_c, _dist(run.cumsum(2), probs.cumsum(2))[0])
    return flip_p, flip_c


@functools.lru_cache(maxsize=None)
def references(c, extra, delta=None):
    """The reference's free run of a case and its bounds, all from the CPU: uniforms, ids, the distribution behind the
    last draw under the case's preset (`exact`) and under `pure`, BOUNDS = [(against, max bound, mean bound or None)],
    the CDF bound and the band the uniforms keep clear: DELTA_FACTOR x the CDF bound of a first run whose uniforms keep
    no band (the CPU module asserts that the band is at least 2 x the CDF bound of the run that is used)."""
    preset, rule = FORMS[c.form][:2]
    d = gen_data(c, extra)
    hp, Q = d["hp"], c.Q
    p, kw = ref_kw(c, d, preset)
    if delta is None:
        if rule == "f32":
            return references(c, extra, DELTA_FACTOR * (Q / 2) * 1e-5)
        worst, delta = 0.0, 0.0
        for _ in range(6):                  # (the bound is measured on the run, and the run depends on the band)
            res = references(c, extra, delta)
            if delta >= 2 * res["cdf_bound"]:
                return res
            worst = max(worst, res["cdf_bound"])
            delta = DELTA_FACTOR * worst
        raise AssertionError("no band holds 2 x the CDF bound of its own run: %s" % gen_id(c))
    un = R.safe_uniforms(p, hp, d["seeds"], N_DRAW, 77 + extra, delta, **kw)
    ids, probs = R.generate(p, hp, d["seeds"], un, **kw)
    _, kwp = ref_kw(c, d, "pure")
    pure = R.run_probs(p, hp, ids, N_DRAW, **kwp)
    res = dict(un=un, ids=ids, probs=probs, exact=probs[:, PIDX], pure=pure[:, PIDX], delta=delta, figures={}, kw=kw, p=p)
    if rule == "f32":
        res["bounds"] = [("exact", 1e-5, None)]
        res["cdf_bound"] = (Q / 2) * 1e-5
        return res
    emu = R.run_probs(p, hp, ids, N_DRAW, dtype=f32, perm=R.Perm(c.S + c.length), **kw).double()
    flip_p, flip_c = one_flip(p, hp, ids, probs, d["n_seed"], c.depth * c.length, kw)
    emax, emean = _dist(emu[:, PIDX], probs[:, PIDX])
    dmax, dmean = _dist(probs[:, PIDX], pure[:, PIDX])
    res["figures"] = dict(emu_max=emax, emu_mean=emean, storage_max=dmax, storage_mean=dmean, one_flip=flip_p, one_flip_cdf=flip_c)
    res["bounds"] = [("exact", max(2 * emax, 2 * flip_p, 1e-5), max(10 * emean, 1e-5)),
                     ("pure", max(4 * dmax, 1e-5), max(2 * dmean, 1e-5))]
    res["cdf_bound"] = max(2 * _dist(emu.cumsum(2), probs.cumsum(2))[0], 2 * flip_c, (Q / 2) * 1e-5)
    return res


def accepts(ref, ids, last_probs):
    """What the GPU test asserts of a generator's output, ids [B, total] and last_probs [B, len(PROBES), Q] (the CPU
    module applies it to planted errors)."""
    if not np.array_equal(np.asarray(ids), ref["ids"]):
        return False
    for against, bmax, bmean in ref["bounds"]:
        emax, emean = _dist(last_probs, ref[against])
        if emax > bmax or (bmean is not None and emean > bmean):
            return False
    return True


# ------------------------------------------------------------------------------------------------------------ the GPU side
WORST = {}


def _note(key, name, err, bound):
    print("  %-44s %-22s %.3e / %.3e = %.2f" % (key, name, err, bound, err / bound if bound else 0.0))
    WORST[(key, name)] = max(WORST.get((key, name), 0.0), err / bound if bound else 0.0)


def _hp_object(hp):
    from nspeech_amd import hparams as hparams_mod
    h = hparams_mod.load("wavenet")
    for k, v in hp.items():
        setattr(h, k, v)
    return h


def _model(c, dev):
    from nspeech_amd.models import create_model
    return create_model("wavenet" if c.opts else "simple_wavenet", _hp_object(hp_of(c)), device=str(dev), dtype="bf16", seed=1)


@pytest.mark.parametrize("c", GEN_CASES, ids=gen_id)
def test_generator_draws_the_reference_run(dev, c):
    preset, rule, gkw, engine = FORMS[c.form]
    m = _model(c, dev)
    for extra in SEED_EXTRA:
        d = gen_data(c, extra)
        ref = references(c, extra)
        m.load_numpy_params(d["params"])
        kw = dict(gkw)
        if d["gc"] is not None:
            kw["global_conditions"] = d["gc"]
        if d["lc"] is not None:
            kw.update(local_conditions=d["lc"], hold=d["hold"], t0=d["t0"])
        seeds, un = d["seeds"].copy(), ref["un"].copy()
        lps = []
        for n in PROBES:
            got = m.generate(seeds, n, uniforms=un[:, :n], **kw).cpu().numpy()
            lps.append(m.last_probs.clone().view(c.B, c.Q).cpu())
            assert m.last_engine == engine, m.last_engine
            if engine == 3:
                assert int(m.last_status.item()) == 0
            wrong = np.argwhere(got != ref["ids"][:, :d["n_seed"] + n])
            assert wrong.size == 0, "first differing draw (waveform, index) %s: %d, reference %d" % (
                wrong[0], got[tuple(wrong[0])], ref["ids"][tuple(wrong[0])])
        lp = torch.stack(lps, dim=1)
        assert np.array_equal(seeds, d["seeds"]) and np.array_equal(un, ref["un"]) and np.array_equal(got[:, :d["n_seed"]], d["seeds"])
        key = gen_id(c) + " +%d" % extra
        for against, bmax, bmean in ref["bounds"]:
            emax, emean = _dist(lp, ref[against])
            _note(key, "probs max vs " + against, emax, bmax)
            if bmean is not None:
                _note(key, "probs mean vs " + against, emean, bmean)
        assert abs(float(lp.sum()) - c.B * len(PROBES)) < 1e-4 * len(PROBES)
        assert accepts(ref, got, lp), (ref["bounds"], ref["figures"])
        again = m.generate(seeds, N_DRAW, uniforms=un, **kw).cpu().numpy()
        assert np.array_equal(again, got) and torch.equal(m.last_probs.view(c.B, c.Q).cpu(), lps[-1])
        if engine == 3:
            assert int(m.last_status.item()) == 0


@pytest.mark.parametrize("c", [c for c in GEN_CASES if c.form == "engine3"], ids=gen_id)
def test_engine_3_under_any_current_stream(dev, c):
    """Chain and helpers are one grid on the call's stream, so engine 3 is chosen and meets its hand-overs under whatever
    stream is current: the default one, then two fresh ones, on ONE model with the same seeds and uniforms.  Every run
    reports engine 3 and status 0, draws the reference's ids, and ids and last_probs are bit-identical across the three
    (the arithmetic does not depend on the stream)."""
    m = _model(c, dev)
    for extra in SEED_EXTRA:
        d, ref = gen_data(c, extra), references(c, extra)
        m.load_numpy_params(d["params"])
        runs = []
        for s in (None, torch.cuda.Stream(dev), torch.cuda.Stream(dev)):
            if s is not None:
                s.wait_stream(torch.cuda.current_stream(dev))     # the parameters were loaded on the default stream
            with torch.cuda.stream(s):
                ids = m.generate(d["seeds"].copy(), N_DRAW, uniforms=ref["un"].copy())
                assert m.last_engine == 3 and int(m.last_status.item()) == 0, (s, m.last_engine)
                runs.append((ids.cpu(), m.last_probs.cpu()))
            torch.cuda.synchronize(dev)
        assert np.array_equal(runs[0][0].numpy(), ref["ids"])
        for ids, probs in runs[1:]:
            assert torch.equal(ids, runs[0][0]) and torch.equal(probs, runs[0][1])


def test_engine_3_at_the_residency_bound(dev):
    """The largest batch engine 3 accepts, B = CUs // 5: a grid of 5 B workgroups, the CU count or up to four short of it,
    every one resident.  generate() takes engine 3 by itself, the status stays 0 and 6 draws coincide with engine 2's in
    the share of rows test_wavenet_helper_engine_equals_the_chain_engine demands (0.6: a draw on a CDF edge may fall the
    other way, the histories part there); one waveform more runs on engine 2 by itself."""
    c = Gen("engine3", 32, 512, 256, 2, 4)
    d = gen_data(c, 5)
    m = _model(c, dev)
    m.load_numpy_params(d["params"])
    B = torch.cuda.get_device_properties(dev).multi_processor_count // 5
    rng = np.random.RandomState(9)
    seeds = rng.randint(0, c.Q, size=(B + 1, d["n_seed"])).astype(np.int32)
    un = np.random.default_rng(3).random((B + 1, 6))
    a = m.generate(seeds[:B], 6, uniforms=un[:B]).cpu().numpy()
    assert m.last_engine == 3 and int(m.last_status.item()) == 0, m.last_engine
    b = m.generate(seeds[:B], 6, uniforms=un[:B], engine=2).cpu().numpy()
    assert m.last_engine == 2
    agree = (a == b).all(axis=1)
    assert agree.mean() >= 0.6, agree
    m.generate(seeds, 6, uniforms=un)
    assert m.last_engine == 2, m.last_engine


# ------------------------------------------------------------------------------------------------------------ bf16 training
Train = namedtuple("Train", "model R S Q depth length N extra opts")
TRAIN_CASES = [Train("simple_wavenet", 32, 64, 64, 2, 3, 2, 24, ""), Train("wavenet", 32, 64, 64, 2, 3, 2, 24, "biases+lc")]
TRAIN_FLIPS = ("xs", "dz")


def train_id(c):
    return "%s-R%d-S%d-Q%d-%dx%d-N%d%s" % (c.model, c.R, c.S, c.Q, c.depth, c.length, c.N, "-" + c.opts if c.opts else "")


@functools.lru_cache(maxsize=None)
def train_data(c):
    hp = hp_of(c)
    rf = R.receptive_field(hp)
    rng = np.random.RandomState(31 + len(c.opts))
    d = dict(hp=hp, rf=rf, params=R.init_params(hp, 12), ids=rng.randint(0, c.Q, size=(c.N, rf + c.extra)).astype(np.int32),
             lc=None, hold=1, t0=None)
    if hp["lc_channels"]:
        d["hold"], d["t0"] = HOLD, [(-4, 2)[n % 2] for n in range(c.N)]
        rows = max(0, rf + c.extra - 2 + max(d["t0"])) // HOLD + 1
        d["lc"] = rng.randn(c.N, rows, hp["lc_channels"]).astype(np.float32)
    return d


def train_one_flip(p, hp, ids, exact, L, kw):
    """one_flip() of the training pass, per compared quantity: the largest-magnitude stored value of xs (forward) and of dz
    (backward) at the first, a middle and the last layer is flipped in turn."""
    out = {k: 0.0 for k in exact}
    for b in TRAIN_FLIPS:
        for l in sorted({0, L // 2, L - 1}):
            fl = _quantities(R.train(p, hp, ids, "train_bf16", flip=(b, l), **kw))
            for k in exact:
                out[k] = max(out[k], _dist(fl[k], exact[k])[0])
    return out


def _quantities(res):
    q = {"logits": res["logits"], "loss": res["loss"].reshape(1)}
    q.update(res["grads"])
    return q


@functools.lru_cache(maxsize=None)
def train_references(c):
    """pure, storage-exact (`train_bf16`) and BOUNDS[quantity] = [(against, max bound, mean bound)] for the logits, the
    loss and every gradient: the bf16 rule (module docstring) with train_one_flip().  The loss is one number: the mean over
    one element is that element, so the maximum's rule with its one-flip floor is the rule for it (one flipped value of
    one row moves the loss by that row's share, whatever the emulation's single draw was).
    Floors: logits 5e-5 max(1, |logits|) (test_wavenet_gpu.py), loss 1e-5 max(1, |loss|), a gradient 1e-4 x
    its largest reference value."""
    d = train_data(c)
    p = R.as_params(d["params"])
    kw = dict(lc=d["lc"], hold=d["hold"], t0=d["t0"])
    ids = torch.as_tensor(d["ids"])
    with torch.no_grad():
        pure = _quantities(R.train(p, d["hp"], ids, "pure", **kw))
        exact = _quantities(R.train(p, d["hp"], ids, "train_bf16", **kw))
        emu = _quantities(R.train(p, d["hp"], ids, "train_bf16", dtype=f32, perm=R.Perm(5), **kw))
        flips = train_one_flip(p, d["hp"], ids, exact, c.depth * c.length, kw)
    bounds, figures = {}, {}
    for k in exact:
        scale = float(pure[k].abs().max())
        floor = 5e-5 * max(1.0, scale) if k == "logits" else 1e-5 * max(1.0, scale) if k == "loss" else 1e-4 * scale
        emax, emean = _dist(emu[k], exact[k])
        dmax, dmean = _dist(exact[k], pure[k])
        flip = flips[k]
        figures[k] = dict(scale=scale, emu_max=emax, emu_mean=emean, storage_max=dmax, storage_mean=dmean, one_flip=flip)
        bounds[k] = [("exact", max(2 * emax, 2 * flip, floor), max(10 * emean, floor)), ("pure", max(4 * dmax, floor), max(2 * dmean, floor))]
        if exact[k].numel() == 1:            # the loss: the mean over one element is that element - the maximum's rule is the rule
            bounds[k] = [(a, bmax, bmax) for a, bmax, _ in bounds[k]]
    return dict(pure=pure, exact=exact, bounds=bounds, figures=figures)


def train_accepts(ref, got, report=None):
    ok = True
    for k, bs in ref["bounds"].items():
        for against, bmax, bmean in bs:
            emax, emean = _dist(torch.as_tensor(np.asarray(got[k])).reshape(ref[against][k].shape), ref[against][k])
            if report:
                report(k + " max vs " + against, emax, bmax)
                report(k + " mean vs " + against, emean, bmean)
            ok = ok and emax <= bmax and emean <= bmean
    return ok


@pytest.mark.parametrize("c", TRAIN_CASES, ids=train_id)
def test_bf16_training_pass(dev, c):
    from nspeech_amd.models import create_model
    d, ref = train_data(c), train_references(c)
    m = create_model(c.model, _hp_object(d["hp"]), device=str(dev), dtype="bf16", seed=1)
    m.load_numpy_params(d["params"])
    ids = torch.from_numpy(d["ids"].copy())
    if d["lc"] is not None:
        m.initialize_ids(ids, local_conditions=d["lc"].copy(), hold=d["hold"], t0=d["t0"])
    else:
        m.initialize_ids(ids)
    m.backward()
    got = dict(m.numpy_grads())
    got["loss"] = np.asarray([m.read_losses()])
    got["logits"] = m.raw_output.float().cpu().numpy()
    assert np.array_equal(ids.numpy(), d["ids"]) and set(got) == set(ref["exact"])
    worst = {}

    def report(name, err, bound):
        fam = name.split("/")[-1]
        worst[fam] = max(worst.get(fam, 0.0), err / bound if bound else 0.0)
    ok = train_accepts(ref, got, report)
    for fam in sorted(worst):
        _note(train_id(c), fam, worst[fam], 1.0)
    assert ok, {k: v for k, v in worst.items() if v > 1.0}


# ------------------------------------------------------------------------------------------------------------ the pieces
def _framed(x, dev, dtype=f32, fill=SENTINEL):
    """x (CPU, flat) between MARGIN sentinels on the device -> (whole buffer, offset of x)."""
    full = torch.full((x.numel() + 2 * MARGIN,), fill, dtype=torch.float32)
    full[MARGIN:MARGIN + x.numel()] = x.reshape(-1).float()
    return full.to(dtype).to(dev), MARGIN


def _margins_intact(buf, n):
    b = buf.float().cpu()
    return bool((b[:MARGIN] == SENTINEL).all() and (b[MARGIN + n:] == SENTINEL).all())


def bf16_coarse(ref, band):
    """Where bf16 is coarser than the band: its spacing at ref is at least 4 x band (elsewhere the band - the fp32 rule -
    is the tighter statement, and being within it is all that is asked)."""
    a = ref.double().abs().clamp(min=1e-300)
    return 2.0 ** (torch.floor(torch.log2(a)) - 7) >= 4 * band


def bf16_store_ok(got, ref, band):
    """(ok, neighbours): got (values stored as bf16) lies between bf16(ref - band) and bf16(ref + band): it is bf16(ref),
    or the neighbour where ref is within band of a rounding boundary.  neighbours: the values that are not bf16(ref),
    counted where bf16_coarse()."""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    ok = (R.bf16(ref - band) <= got) & (got <= R.bf16(ref + band))
    neigh = (got != R.bf16(ref)) & bf16_coarse(ref, band)
    return bool(ok.all()), int(neigh.sum())


def _check_store(key, name, got, ref, dtype, band):
    """fp32: within band; bf16: the single-stored-value rule with at most 1 % neighbours."""
    if dtype == f32:
        err = float((got.double() - ref.double()).abs().max()) if ref.numel() else 0.0
        _note(key, name, err, band)
        assert err <= band, (key, name, err, band)
        return
    ok, n = bf16_store_ok(got, ref, band)
    print("  %-44s %-22s bf16 neighbours %d of %d" % (key, name, n, ref.numel()))
    WORST[(key, name + " neighbours")] = max(WORST.get((key, name + " neighbours"), 0.0), n / max(1, ref.numel()) / 0.01)
    assert ok, (key, name, "a stored value is neither bf16(reference) nor its neighbour inside the band")
    assert n <= 0.01 * ref.numel(), (key, name, n)


# 2 Q C 4 bytes: 8 KB, 64 KB (LDS table), 96 KB (atomics); the last shape has N T >= Q, so that its "cover" ids are ALL of Q
INPUT_SHAPES = [(1, 2, 16, 64), (3, 9, 32, 256), (2, 17, 48, 256), (2, 40, 16, 64)]


def input_data(N, T, C, Q, ids_kind="random"):
    g = torch.Generator().manual_seed(N * 100 + T * 10 + C + Q)
    if ids_kind == "equal":
        ids = torch.full((N, T), Q // 3, dtype=torch.int32)
    elif ids_kind == "cover":                       # ids from 0 to Q - 1: every one of Q where N T >= Q, no collisions below
        ids = torch.linspace(0, Q - 1, N * T).round().to(torch.int32).reshape(N, T)
        assert len(set(ids.reshape(-1).tolist())) == min(Q, N * T)
    else:
        ids = torch.randint(0, Q, (N, T), generator=g, dtype=torch.int32)
        ids.reshape(-1)[0], ids.reshape(-1)[-1] = 0, Q - 1
    w = torch.randn(2, Q, C, generator=g)
    dx = torch.randn(N, T, C, generator=g)
    dw0 = torch.randn(2, Q, C, generator=g)
    return ids, w, dx, dw0


@pytest.mark.parametrize("dtype", [f32, bf], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", INPUT_SHAPES, ids=str)
def test_input_forward(dev, shape, dtype):
    from nspeech_amd import ops
    N, T, C, Q = shape
    ids, w, _, _ = input_data(*shape)
    ref = R.input_fwd(ids, w.double())
    wb, woff = _framed(w, dev)
    xb, xoff = _framed(torch.zeros(N * T * C), dev, dtype, fill=SENTINEL)
    xb[xoff:xoff + N * T * C] = 3.0
    idd = ids.to(dev)
    ops.wavenet_input(idd, wb, xb[xoff:], N, T, C, Q, w_off=woff)
    got = xb[xoff:xoff + N * T * C].float().cpu().reshape(N, T, C)
    assert _margins_intact(xb, N * T * C) and torch.equal(idd.cpu(), ids) and torch.equal(wb.cpu()[woff:woff + w.numel()], w.reshape(-1))
    assert bool((got[:, 0] == 0).all())
    _check_store("input fwd %s" % (shape,), "x", got, ref, dtype, 1e-6)


@pytest.mark.parametrize("ids_kind", ["random", "equal", "cover"])
@pytest.mark.parametrize("start", [0, 1, 5])
@pytest.mark.parametrize("dtype", [f32, bf], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", INPUT_SHAPES, ids=str)
def test_input_backward(dev, shape, dtype, start, ids_kind):
    from nspeech_amd import ops
    N, T, C, Q = shape
    ids, _, dx, dw0 = input_data(*shape, ids_kind=ids_kind)
    dx = dx.to(dtype).float()                      # the values the kernel reads
    s = max(1, start)
    dx_dev = dx.clone()
    dx_dev[:, :s] = 1e30                           # rows the sum must not touch
    ref = R.input_bwd(ids, dx, dw0, start=start)
    dwb, off = _framed(dw0, dev)
    dxd = dx_dev.to(dtype).to(dev)
    keep = dxd.clone()
    idd = ids.to(dev)
    ops.wavenet_input(idd, None, None, N, T, C, Q, dx=dxd, dw=dwb, dw_off=off, start=start)
    got = dwb[off:off + dw0.numel()].cpu().reshape(2, Q, C)
    assert _margins_intact(dwb, dw0.numel()) and torch.equal(dxd, keep) and torch.equal(idd.cpu(), ids)
    assert bool(torch.isfinite(got).all())
    _check_store("input bwd %s %s start %d" % (shape, ids_kind, start), "dw", got, ref, f32, 1e-4 * float(ref.abs().max()))


GATE_SHAPES = [(1, 16, 5), (3, 32, 11), (2, 24, 40)]          # (N, C, T): rows = N * T


def gate_data(N, C, T, start, with_cond):
    g = torch.Generator().manual_seed(N * 1000 + C * 10 + T + start)
    z = torch.randn(N, T, 2 * C, generator=g) * 2.0
    sp = torch.tensor([50.0, -50.0, 100.0, -100.0, 0.0])
    for i, v in enumerate(sp):                       # the last row is valid for every start < T
        z[0, T - 1, i], z[0, T - 1, 2 * C - 1 - i], z[N - 1, T - 1, C - 1 - i], z[N - 1, T - 1, C + i] = v, -v, v, v
    big = torch.where(torch.rand(N, T, 2 * C, generator=g) < 0.5, torch.tensor(1e30), torch.tensor(-1e30))
    z[:, :start] = big[:, :start]
    dout = torch.randn(N, T, C, generator=g) * 0.5
    cond = t0 = None
    rows = 4
    if with_cond:
        cond = torch.randn(N, rows, 2 * C + 5, generator=g)
        t0 = torch.tensor([(-3, 2, 7)[n % 3] for n in range(N)], dtype=torch.int32)      # clamped in front of row 0 / past the last row
    return z.reshape(N * T, 2 * C), dout.reshape(N * T, C), cond, t0, rows


@pytest.mark.parametrize("with_cond", [False, True], ids=["plain", "cond"])
@pytest.mark.parametrize("start_kind", ["0", "4", "T"])
@pytest.mark.parametrize("dtype", [f32, bf], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", GATE_SHAPES, ids=str)
def test_gate_forward_and_backward(dev, shape, dtype, start_kind, with_cond):
    from nspeech_amd import ops
    N, C, T = shape
    start = T if start_kind == "T" else int(start_kind)
    rows = N * T
    z, dout, cond, t0, crows = gate_data(N, C, T, start, with_cond)
    dout = dout.to(dtype).float()
    hold = 3
    ckw, rkw = {}, {}
    if with_cond:
        cd, t0d = cond.reshape(-1).to(dev), t0.to(dev)
        ckw = dict(cond=cd, ld_cond=2 * C + 5, cond_rows=crows, cond_hold=hold, cond_t0=t0d)
        rkw = dict(cond=cond, hold=hold, t0=t0)
    key = "gate %s start %d %s" % (shape, start, "cond" if with_cond else "plain")
    zd = z.to(dev)
    zkeep = zd.clone()
    # forward into a column block of a wider buffer
    ld, off = 3 * C + 8, C + 3
    ob = torch.full((MARGIN + rows * ld + MARGIN,), SENTINEL, dtype=torch.float32).to(dtype).to(dev)
    ops.wavenet_gate(zd, rows, C, T, start, out=ob, out_off=MARGIN + off, ld_out=ld, **ckw)
    body = ob.float().cpu()[MARGIN:MARGIN + rows * ld].reshape(rows, ld)
    got = body[:, off:off + C]
    ref = R.gate_fwd(z, T, start, **rkw)
    rest = torch.cat([body[:, :off], body[:, off + C:]], dim=1)
    assert bool((rest == SENTINEL).all()) and _margins_intact(ob, rows * ld) and torch.equal(zd, zkeep)
    inval = (torch.arange(rows) % T) < start
    assert bool((got[inval] == 0).all())
    _check_store(key, "out", got, ref, dtype, 1e-6)
    # backward
    ldd, doff = C + 3, 2
    db = torch.full((rows * ldd + MARGIN,), 0.25, dtype=torch.float32)
    db[:rows * ldd].reshape(rows, ldd)[:, doff:doff + C] = dout
    dbd = db.to(dtype).to(dev)
    dkeep = dbd.clone()
    dzb, zoff = _framed(torch.zeros(rows * 2 * C), dev, dtype)
    ops.wavenet_gate(zd, rows, C, T, start, dout=dbd, dout_off=doff, ld_dout=ldd, dz=dzb[zoff:], **ckw)
    gdz = dzb[zoff:zoff + rows * 2 * C].float().cpu().reshape(rows, 2 * C)
    rdz = R.gate_bwd(z, dout, T, start, **rkw)
    assert _margins_intact(dzb, rows * 2 * C) and torch.equal(zd, zkeep) and torch.equal(dbd, dkeep)
    assert bool((gdz[inval] == 0).all())
    _check_store(key, "dz", gdz, rdz, dtype, 1e-6 * max(1.0, float(dout.abs().max())))


CE_SHAPES = [(1, 64), (5, 100), (7, 7), (4100, 7), (33, 256)]        # 4100 rows: more than 1024 blocks x 4 rows


def ce_data(rows, Q):
    g = torch.Generator().manual_seed(rows * 7 + Q)
    ld = Q + 3
    lg = torch.randn(rows, ld, generator=g) * 3.0
    lg[0, :Q] += 80.0
    lg[rows - 1, 1:Q:2] = -1e30
    tg = torch.randint(0, Q, (rows,), generator=g, dtype=torch.int32)
    tg[0], tg[rows - 1] = Q - 1, 0
    return lg, tg, ld


@pytest.mark.parametrize("dmode", ["f32", "bf16", "none"])
@pytest.mark.parametrize("shape", CE_SHAPES, ids=str)
def test_softmax_cross_entropy(dev, shape, dmode):
    from nspeech_amd import ops
    rows, Q = shape
    lg, tg, ld = ce_data(rows, Q)
    scale = 1.0 / rows
    loss, dref = R.softmax_ce(lg[:, :Q], tg, scale)
    lgd, tgd = lg.reshape(-1).to(dev), tg.to(dev)
    keep = lgd.clone()
    acc = torch.tensor([0.0, 1.5, SENTINEL, SENTINEL], dtype=f32).to(dev)
    ld_d = Q + 5
    dtype = bf if dmode == "bf16" else f32
    db = None if dmode == "none" else torch.full((MARGIN + rows * ld_d + MARGIN,), SENTINEL, dtype=f32).to(dtype).to(dev)
    for _ in range(2):                              # two launches accumulate
        ops.wavenet_softmax_ce(lgd, ld, tgd, rows, Q, scale, acc, acc_off=1, dlogits=None if db is None else db[MARGIN:], ld_d=ld_d)
    a = acc.cpu()
    key = "softmax_ce %s %s" % (shape, dmode)
    want = 1.5 + 2 * float(loss)
    _note(key, "loss", abs(float(a[1]) - want), 1e-5 * max(1.0, abs(want)))
    assert abs(float(a[1]) - want) <= 1e-5 * max(1.0, abs(want)) and float(a[0]) == 0.0 and float(a[2]) == SENTINEL
    assert torch.equal(lgd, keep) and torch.equal(tgd.cpu(), tg)
    if db is not None:
        body = db.float().cpu()[MARGIN:MARGIN + rows * ld_d].reshape(rows, ld_d)
        assert bool((body[:, Q:] == SENTINEL).all()) and _margins_intact(db, rows * ld_d)
        _check_store(key, "dlogits", body[:, :Q], dref, dtype, 1e-4 * float(dref.abs().max()))


@pytest.mark.parametrize("shape", [(1, 64, 64), (3, 100, 104), (2, 256, 300)], ids=str)
def test_softmax_float64(dev, shape):
    from nspeech_amd import ops
    rows, Q, ld = shape
    g = torch.Generator().manual_seed(rows + Q)
    lg = torch.randn(rows, ld, generator=g) * 3.0
    lg[0, :Q] += 80.0
    lg[rows - 1, 1:Q:2] = -1e30
    ref = R.softmax64(lg[:, :Q]).float()
    lgb, off = _framed(lg, dev)
    pb, poff = _framed(torch.zeros(rows * Q), dev)
    keep = lgb.clone()
    ops.wavenet_softmax(lgb, ld, rows, Q, pb[poff:], logits_off=off)
    got = pb[poff:poff + rows * Q].cpu().reshape(rows, Q)
    assert _margins_intact(pb, rows * Q) and torch.equal(lgb, keep)
    up, down = torch.nextafter(ref, torch.tensor(2.0)), torch.nextafter(ref, torch.tensor(-1.0))
    ok = (got == ref) | (got == up) | (got == down)
    print("  softmax %s: %d of %d values are the float32 neighbour" % (shape, int((got != ref).sum()), ref.numel()))
    assert bool(ok.all())


def test_worst_ratios_are_reported():
    for k in sorted(WORST):
        print("%-70s %-26s %.2f" % (k[0], k[1], WORST[k]))
    assert all(math.isfinite(v) for v in WORST.values())
