"""The persistent whole-sequence GRU kernels (csrc/gru.hip: ns_gru_seq_fwd / ns_gru_seq_bwd, twelve instantiations: H 128
- one workgroup per chain - and H 256 - clusters of four with the tagged-granule exchange and the K split -, fp32 storage
with three split-bf16 passes or one pass, bf16 storage, forward and backward) against the float64 contract of
ns_gru_seq_params (tests/gru_ref.py, itself proven by tests/test_gru_ref_cpu.py), through nspeech_amd.ops.  Errors are
measured against the references, never against another kernel; every valid (n, t, u) of h, ru (un-permuted from the
kernels' private order), c, rh, dzg, dzc and every (n, u) of dh_init is compared.

Forms: f32x3, f32x1, bf16 and `mixed` - the models' mode of that name: the forward call at f32_passes 3, the backward
call at f32_passes 1 on the forward's saved gates.  CASES says in one line per case what it is for.  One case per
(H, form) runs T = 11 as three launches over [0, 3), [3, 4), [4, 11) exactly as models/tacotron.py: _gru_pair forms its
windows (padl moved to padl + t0, ru / c offset by N16 t0 2H / N16 t0 H, h_init a copy of the history row in front,
backward in reverse order with dh_init added to that row's dh) and is compared with the reference of the whole 11 steps;
with bf16 storage that arrangement rounds the state at a window edge and the storage-exact reference says so.

Layout of every case: h and dh are column blocks of wider buffers (8 columns of margin on either side), so are xg, xc,
h_init and dh_init (ld_xg > 2H, ld_xc > H, ld_hi, ld_dhi > H), the backward weights have padded rows, rows are padded
(padl 2, P = padl + T + 3) and every output buffer has a guard tail (16 further batch rows; 4096 floats behind ru and c).
Afterwards: margins, pad rows and guard tails still hold their sentinels (h, dzg, dzc: the pad rows their zeros) - which
covers rows n >= N of a ragged row group, written nowhere but in ru and c (whole groups by contract); every input is
bit-identical; h, dzg and dzc - prefilled with a sentinel - are exactly 0 from each row's length on although dh holds
non-zero values there; ru, c and rh are finite and written everywhere; dh_init, prefilled with a sentinel, holds the
reference (overwritten, not added to); every launch runs twice on the same work buffer with the status word 0 after
each, and the second result is the one compared.  A case ns_gru_seq_supported declines fails.

Tolerances, relative to scale = max |reference| of the buffer over the valid entries, computed on the CPU per case
(references() below); S = T:
  fp32 rule  - f32x3, and the forward buffers of `mixed`: against the pure reference,
               max <= max(c sqrt(S), 4 x the distance between the pure reference evaluated in float32 with a permuted
               summation order and in float64) x scale, c = 2e-5 for h, ru, c, rh and 5e-5 for dzg, dzc, dh_init (the
               constants of test_gru_seq_gpu.py and the LSTM module; the rule of the attention module).
  bf16 rule  - f32x1, the backward buffers of `mixed`, bf16 (the rule of test_lstm_contract_gpu.py, with its floors):
               against the storage-exact reference of the arrangement: max <= 2 x and mean <= 10 x what a float32
               emulation of the same arrangement, summed in a permuted order, differs from it by;
               against the pure reference: max <= 4 x and mean <= 2 x the storage-exact reference's own distance.
               None of the four is tighter than the fp32 rule's bound, and the maximum against the storage-exact
               reference is never below 2 x one_flip() (that module's docstring, "One flip": a value within fp32 noise
               of a bf16 rounding boundary rounds the other way in the kernel than in the emulation).
  one_flip() - from the arrangement's rounding points, the buffers' magnitudes and the largest weight alone.  A flipped
               operand of a product moves its sum by one bf16 step of the operand's buffer x the largest weight:
               dzg_pre (h), dzc_pre (r * h) forward, ddh (dzc through Wc^T with r <= 1, [dzr | dzu] through Wg^T)
               backward.  sigmoid' <= 1/4, tanh' <= 1: ru moves by dzg_pre / 4, rh by that x max |state|, c by dzc_pre
               (or by the moved r * h x the largest weight), h' = u h + (1 - u) c by d ru x (max |state| + max |c|) or
               by d c.  The gate gradients and dh_init are dh_total x factors of at most 1, dh_total = carry + dh_out:
               they move by ddh, and a forward flip reaches them through those factors: dh_total_max x (d ru + 2 d c,
               + step(h) / 4 where h_prev is read from a bf16 history).  A buffer stored in bf16 has its own step.
No bound is taken from the kernels' output.

Found by this module: no kernel was found wrong.  All 56 cases met every bound at the first run on the MI355X, the status
word was 0 after each of the 288 launches, and nothing outside the contract's regions was written.  A length of 0 is
handled (the row emits zeros, carries h_init through every step and returns dh_init = 0); the header's sentence on
lengths did not say so, nor that dzg / dzc are exact zeros past the length, nor what the saved gates of masked steps
hold: it does now.  The storage-exact arrangements as first read off csrc/gru.hip needed no correction.

Worst error / bound per H, form and buffer on the MI355X, over all cases of the form (every test prints its own per
buffer, `pytest -s`; "exact" = against the storage-exact reference, "pure" = against the pure one; max, or max / mean).
The constant term of the fp32 rule decided in every case: 4 x the float32 evaluation's distance was smaller everywhere.
  H 128  f32x3  pure:  h 0.09  ru 0.09  c 0.14  rh 0.06  dzg 0.03  dzc 0.03  dh_init 0.04
         f32x1  exact: h 0.11 / 0.04  ru 0.26 / 0.03  c 0.16 / 0.07  rh 0.23 / 0.02  dzg 0.01 / 0.03  dzc 0.03 / 0.04  dh_init 0.02 / 0.14
                pure:  at most 0.26 / 0.50
         mixed  pure:  h 0.08  ru 0.09  c 0.14  rh 0.06;  exact: dzg 0.04 / 0.03  dzc 0.06 / 0.04  dh_init 0.11 / 0.15
                pure:  dzg, dzc, dh_init at most 0.26 / 0.50
         bf16   exact: h 0.25 / 0.03  ru 0.26 / 0.03  c 0.16 / 0.07  rh 0.25 / 0.02  dzg 0.03 / 0.01  dzc 0.07 / 0.01  dh_init 0.01 / 0.06
                pure:  all 0.25 / 0.50
  H 256  f32x3  pure:  h 0.07  ru 0.07  c 0.14  rh 0.07  dzg 0.02  dzc 0.04  dh_init 0.04
         f32x1  exact: h 0.16 / 0.07  ru 0.46 / 0.07  c 0.28 / 0.07  rh 0.32 / 0.07  dzg 0.01 / 0.06  dzc 0.04 / 0.08  dh_init 0.04 / 0.11
                pure:  at most 0.27 / 0.50
         mixed  pure:  h 0.07  ru 0.07  c 0.14  rh 0.07;  exact: dzg 0.04 / 0.02  dzc 0.10 / 0.02  dh_init 0.15 / 0.11
                pure:  dzg, dzc, dh_init at most 0.26 / 0.50
         bf16   exact: h 0.25 / 0.07  ru 0.46 / 0.07  c 0.28 / 0.12  rh 0.25 / 0.07  dzg 0.08 / 0.06  dzc 0.16 / 0.07  dh_init 0.03 / 0.19
                pure:  at most 0.31 / 0.50
0.25 / 0.50 against the pure reference is a kernel exactly as far from it as its operand format is (the bounds are 4 x and
2 x that distance); 0.25 and 0.46 against the storage-exact reference are one flip below the top binade."""
import functools
import math
from collections import namedtuple

import pytest
import torch

import gru_ref as R

pytestmark = pytest.mark.gpu

Case = namedtuple("Case", "H form N T dirs masked h0 opt why")
F, B, FB, FF = (False,), (True,), (False, True), (False, False)      # the directions of a launch (reverse flags)
f32, bf = torch.float32, torch.bfloat16
MARGIN = 8                                        # columns on either side of a block
GUARD_ROWS = 16                                   # batch rows behind every [N * P, .] output
GUARD_F = 4096                                    # floats behind ru and c
SENTINEL = 7.0
PADL, TAIL = 2, 3
WINDOWS = [(0, 3), (3, 4), (4, 11)]
FORMS = {"f32x3": (f32, 3, 3), "f32x1": (f32, 1, 1), "mixed": (f32, 3, 1), "bf16": (bf, 0, 0)}      # storage, f32_passes fwd / bwd
BUFFERS = ("h", "ru", "c", "rh", "dzg", "dzc", "dh_init")
FORWARD = ("h", "ru", "c", "rh")

#          N   T  dirs masked h0  opt
SHAPES = [(1, 1, F, False, False, None, "one row, one step: nothing behind the first prefetch; a single direction"),
          (5, 2, FB, True, True, None, "less than a row group, two slots in flight and no third; reverse with lengths and h_init"),
          (17, 3, B, True, True, None, "one row into the second group; s + 2 < T once; a single reverse direction, lengths 1 and T"),
          (16, 4, FB, False, True, None, "exactly one group; the stage rotation wraps to buffer 0"),
          (33, 13, FB, True, True, None, "three groups with a one-row tail; the rotation four times round"),
          (17, 11, F, False, True, "windows", "three launches over [0, 3), [3, 4), [4, 11) as _gru_pair forms them")]
CASES = [Case(H, form, *s) for H in (128, 256) for form in FORMS for s in SHAPES]
CASES += [Case(128, "f32x3", 5, 40, FB, True, True, None, "T = 40: the sqrt(T) term"),
          Case(256, "f32x1", 5, 40, FB, True, True, None, "T = 40: the sqrt(T) term"),
          Case(128, "mixed", 5, 40, FB, True, True, None, "T = 40: the sqrt(T) term"),
          Case(256, "bf16", 5, 40, FB, True, True, None, "T = 40: the sqrt(T) term"),
          Case(128, "f32x3", 5, 3, FF, False, True, None, "two forward directions with different weights (pair_ok admits it)"),
          Case(256, "bf16", 5, 3, FF, False, True, None, "two forward directions with different weights (pair_ok admits it)"),
          Case(128, "f32x1", 17, 4, FB, True, True, "len0", "a length of 0 beside lengths 1 and T"),
          Case(256, "mixed", 17, 4, FB, True, True, "len0", "a length of 0 beside lengths 1 and T")]


def case_id(c):
    return "H%d-%s-N%d-T%d-%s%s%s%s" % (c.H, c.form, c.N, c.T, "".join("fr"[d] for d in c.dirs), "-len" if c.masked else "",
                                        "-h0" if c.h0 else "", "-%s" % c.opt if c.opt else "")


def windows_of(c):
    return WINDOWS if c.opt == "windows" else None


@functools.lru_cache(maxsize=None)
def inputs(c):
    """The operands of a case, per direction, on the CPU: what both the references and the kernels are given."""
    g = torch.Generator().manual_seed(c.N * 1009 + c.T * 101 + c.H + 7 * len(c.dirs) + 3 * sum(c.dirs))
    lengths = None
    if c.masked:
        lengths = torch.randint(1, c.T + 1, (c.N,), generator=g, dtype=torch.int32)
        lengths[0], lengths[-1] = c.T, 1
        if c.opt == "len0":
            lengths[1], lengths[-2] = 0, 0       # the second and the last row of the first row group
    dirs = []
    for _ in c.dirs:
        Wg, Wc = (torch.randn(c.H, k * c.H, generator=g) / c.H ** 0.5 for k in (2, 1))
        if FORMS[c.form][0] == bf:               # the kernel sees bf16 weights: so does the reference
            Wg, Wc = R.bf16(Wg), R.bf16(Wc)
        dirs.append(dict(xg=torch.randn(c.N, c.T, 2 * c.H, generator=g), xc=torch.randn(c.N, c.T, c.H, generator=g), Wg=Wg, Wc=Wc,
                         dh=torch.randn(c.N, c.T, c.H, generator=g) * 0.3,       # non-zero past the lengths too
                         h0=torch.randn(c.N, c.H, generator=g) * 0.5 if c.h0 else None))
    return lengths, dirs


def rule_of(c, k):
    """"f32" or "bf16" (module docstring), from what the arrangement rounds in front of the buffer."""
    p = R.PRESETS[c.form]
    return "bf16" if p["fwd_product" if k in FORWARD else "bwd_product"] == "bf16" else "f32"


def _valid(ref, k):
    return torch.ones(ref[k].shape[0], 1, dtype=torch.bool) if k == "dh_init" else ref["valid"]


def _dist(a, b, valid):
    """max and mean |a - b| over the valid entries, and max |b| there."""
    a, b = (x.reshape(x.shape[0], valid.shape[1], -1) for x in (a, b))
    v = valid[:, :, None].expand_as(b)
    d = (a.double() - b.double()).abs()[v]
    return float(d.max()), float(d.mean()), float(b.double().abs()[v].max())


def bf16_step(x):
    """The spacing of bf16 (8 significant bits) at magnitude x."""
    return 2.0 ** (math.floor(math.log2(x)) - 7) if x > 0 else 0.0


def one_flip(preset, scale, state_max, wg_max, wc_max, dh_total_max):
    """Per buffer, the most that ONE value rounding to the neighbouring bf16 can move an element (module docstring)."""
    fwd, bwd, st = preset.get("fwd_product") == "bf16", preset.get("bwd_product") == "bf16", "h" in preset
    d_ru = bf16_step(state_max) * wg_max / 4 if fwd else 0.0
    d_rh = max(bf16_step(scale["rh"]) if st else 0.0, d_ru * state_max)
    d_c = max(bf16_step(scale["rh"]) * wc_max if fwd else 0.0, d_rh * wc_max)
    d_h = max(bf16_step(scale["h"]) if st else 0.0, d_ru * (state_max + scale["c"]), d_c)
    ddh = max(bf16_step(scale["dzg"]) * wg_max, bf16_step(scale["dzc"]) * wc_max) if bwd else 0.0
    through = dh_total_max * (d_ru + 2 * d_c + (bf16_step(scale["h"]) / 4 if st else 0.0))
    out = dict(h=d_h, ru=d_ru, c=d_c, rh=d_rh, dh_init=max(ddh, through))
    for k in ("dzg", "dzc"):
        out[k] = max(bf16_step(scale[k]) if st else 0.0, ddh, through)
    return out


@functools.lru_cache(maxsize=None)
def references(c):
    """Per direction: the pure and the storage-exact reference and bounds[buffer] = a list of (against, max bound, mean
    bound or None), all from the CPU; source[buffer] says which term of the fp32 rule decided."""
    lengths, dirs = inputs(c)
    preset = R.PRESETS[c.form]
    out = []
    for reverse, d in zip(c.dirs, dirs):
        run = functools.partial(R.gru_seq, d["xg"], d["xc"], d["Wg"], d["Wc"], lengths=lengths, reverse=reverse, h_init=d["h0"],
                                dh=d["dh"], windows=windows_of(c))
        perm = torch.randperm(c.H, generator=torch.Generator().manual_seed(c.H + c.T))
        pure = run()
        emu32 = run(dtype=torch.float32, perm=perm)                               # the fp32 rule's second term
        res = dict(pure=pure, exact=pure, bounds={}, figures={}, source={})
        if any(rule_of(c, k) == "bf16" for k in BUFFERS):
            res["exact"] = run(rounding=preset)
            emu = run(rounding=preset, dtype=torch.float32, perm=perm)
        scales = {k: _dist(pure[k], pure[k], _valid(pure, k))[2] for k in BUFFERS}
        state_max = max(scales["h"], float(d["h0"].abs().max()) if c.h0 else 0.0)
        flip = one_flip(preset, scales, state_max, float(d["Wg"].abs().max()), float(d["Wc"].abs().max()),
                        res["exact"]["dh_total_max"])
        for k in BUFFERS:
            scale, valid = scales[k], _valid(pure, k)
            const = (2e-5 if k in FORWARD else 5e-5) * math.sqrt(c.T)
            emu_rel = _dist(emu32[k], pure[k], valid)[0] / scale if scale else 0.0
            floor = max(const, 4 * emu_rel) * scale
            res["source"][k] = "const" if const >= 4 * emu_rel else "emu"
            if rule_of(c, k) == "f32":
                res["bounds"][k] = [("pure", floor, None)]
                continue
            emax, emean, _ = _dist(emu[k], res["exact"][k], valid)
            dmax, dmean, _ = _dist(res["exact"][k], pure[k], valid)
            res["figures"][k] = dict(scale=scale, emu_max=emax, emu_mean=emean, storage_max=dmax, storage_mean=dmean,
                                     one_flip=flip[k])
            res["bounds"][k] = [("exact", max(2 * emax, 2 * flip[k], floor), max(10 * emean, floor)),
                                ("pure", max(4 * dmax, floor), max(2 * dmean, floor))]
        out.append(res)
    return out


# ------------------------------------------------------------------------------------------------------------ the GPU side
def _bytes(x):
    return x.contiguous().view(-1).view(torch.uint8)


def _saved(x, N, T, H, nsec):
    """ns_gru_seq's own order [row group][t][workgroup][section][chunk][row][4] -> [N, T, nsec * H]"""
    G = 1 if H == 128 else 4
    U, nrg = H // G, (N + 15) // 16
    v = x.view(nrg, T, G, nsec, U // 4, 16, 4)
    return v.permute(0, 5, 1, 3, 2, 4, 6).reshape(nrg * 16, T, nsec * H)[:N]      # row group, row | t | section, workgroup, chunk, 4


def run_case(c, dev):
    """Runs the case's forward and backward launches; returns per direction the outputs cut to [N, T, .] on the CPU.  All
    layout assertions happen here."""
    from nspeech_amd import ops
    D, fpass, bpass = FORMS[c.form]
    N, T, H, padl, nd = c.N, c.T, c.H, PADL, len(c.dirs)
    P, NG, N16 = padl + T + TAIL, c.N + GUARD_ROWS, (c.N + 15) // 16 * 16
    lengths, dirs = inputs(c)
    wins = windows_of(c) or [(0, T)]
    nan = float("nan")
    ld_h, ld_xg, ld_xc, ld_i, ld_wg, ld_wc = nd * H + 2 * MARGIN, 2 * H + 2 * MARGIN, H + 2 * MARGIN, H + 2 * MARGIN, 2 * H + 8, H + 8
    steps = slice(padl, padl + T)

    def rows(ld, dtype, pad_fill, lo=0, hi=None):
        """[N + guard, P, ld] of SENTINEL; the columns lo .. hi of the pad rows of the N real batch rows hold pad_fill"""
        x = torch.full((NG, P, ld), SENTINEL)
        keep = x[:N, steps, lo:hi].clone()
        x[:N, :, lo:hi] = pad_fill
        x[:N, steps, lo:hi] = keep
        return x.to(dtype).to(dev)

    def block(shape, at, x, dtype=f32):
        full = torch.full(shape, nan)
        full[at] = x
        return full.to(dtype).to(dev)

    h_buf = rows(ld_h, D, 0.0, MARGIN, MARGIN + nd * H)          # the history's pad rows are zero
    dh_buf = torch.full((N, P, ld_h), nan)
    for di, d in enumerate(dirs):
        dh_buf[:, steps, MARGIN + di * H:MARGIN + (di + 1) * H] = d["dh"]
    dh_buf = dh_buf.to(dev)
    dh_before = dh_buf.clone()
    lens_d = None if lengths is None else lengths.to(dev)
    keep = []
    for di, d in enumerate(dirs):
        b = dict(xg=block((N, P, ld_xg), (slice(None), steps, slice(MARGIN, MARGIN + 2 * H)), d["xg"]),
                 xc=block((N, P, ld_xc), (slice(None), steps, slice(MARGIN, MARGIN + H)), d["xc"]),
                 wgT=d["Wg"].t().contiguous().to(D).to(dev), wcT=d["Wc"].t().contiguous().to(D).to(dev),
                 wg=block((H, ld_wg), (slice(None), slice(0, 2 * H)), d["Wg"], D),
                 wc=block((H, ld_wc), (slice(None), slice(0, H)), d["Wc"], D),
                 ru=torch.full((N16 * T * 2 * H + GUARD_F,), SENTINEL, device=dev),
                 c=torch.full((N16 * T * H + GUARD_F,), SENTINEL, device=dev),
                 rh=rows(H, D, SENTINEL), dzg=rows(2 * H, D, 0.0), dzc=rows(H, D, 0.0),
                 hi=[None if t0 == 0 and not c.h0 else torch.full((N, ld_i), nan, device=dev) for t0, _ in wins],
                 dhi=[torch.full((NG, ld_i), SENTINEL, device=dev) for _ in wins])
        if c.h0:
            b["hi"][0][:, MARGIN:MARGIN + H] = d["h0"].to(dev)
        b["before"] = {k: b[k].clone() for k in ("xg", "xc", "wgT", "wcT", "wg", "wc")}
        b["hi0_before"] = None if b["hi"][0] is None else b["hi"][0].clone()
        keep.append(b)

    def params(di, wi, backward):
        b, (t0, t1) = keep[di], wins[wi]
        off = MARGIN + di * H
        kw = {}
        if backward:
            kw = dict(dh=(dh_buf, off), ld_dh=ld_h, dzg=b["dzg"], dzc=b["dzc"], dh_init=(b["dhi"][wi], MARGIN), ld_dhi=ld_i)
        hi = b["hi"][wi]
        # a window = the same arrays with the first row moved to t0 (models/tacotron.py: _gru_pair)
        return ops.gru_seq_params(h_buf, N, t1 - t0, H, P, padl + t0, c.dirs[di], lens_d, (b["xg"], MARGIN), (b["xc"], MARGIN),
                                  b["wgT"], b["wcT"], b["wg"], ld_wg, b["wc"], ld_wc, (h_buf, off), ld_h,
                                  (b["ru"], N16 * t0 * 2 * H), (b["c"], N16 * t0 * H), b["rh"],
                                  h_init=None if hi is None else (hi, MARGIN), ld_hi=ld_i, ld_xg=ld_xg, ld_xc=ld_xc, **kw)

    def launch(direction, wi, work):
        backward = direction == "bwd"
        ops.F32_PASSES = bpass if backward else fpass
        pp = [params(di, wi, backward) for di in range(nd)] + [None]
        assert ops.gru_seq_supported(pp[0], pp[1], backward=backward), "ns_gru_seq_%s declines %s" % (direction, case_id(c))
        if work is None:
            work = torch.zeros(ops.gru_seq_work_floats(pp[0]), device=dev)
        for _ in range(2):                                        # the second launch re-initialises the exchange state
            ops.gru_seq(direction, pp[0], pp[1], work)
            torch.cuda.synchronize()
            assert int(work[:1].view(torch.int32).item()) == 0, (direction, wi, case_id(c))
        return work

    try:
        work = None
        for wi, (t0, _) in enumerate(wins):
            if t0:                                                # the state in front of the window is its initial state
                for di, b in enumerate(keep):
                    b["hi"][wi][:, MARGIN:MARGIN + H] = h_buf[:N, padl + t0 - 1, MARGIN + di * H:MARGIN + (di + 1) * H].float()
            work = launch("fwd", wi, work)
        for wi in range(len(wins) - 1, -1, -1):
            t0 = wins[wi][0]
            work = launch("bwd", wi, work)
            if t0:                                                # ... and its gradient belongs to the row in front of the window
                for di, b in enumerate(keep):
                    dh_buf[:, padl + t0 - 1, MARGIN + di * H:MARGIN + (di + 1) * H] += b["dhi"][wi][:N, MARGIN:MARGIN + H]
        torch.cuda.synchronize()
    finally:
        ops.F32_PASSES = 0

    for t0, _ in wins[1:]:                                        # (the rows this function itself added to)
        dh_buf[:, padl + t0 - 1], dh_before[:, padl + t0 - 1] = 0, 0
    assert torch.equal(_bytes(dh_buf), _bytes(dh_before)), "dh changed"
    if lengths is not None:
        assert torch.equal(lens_d.cpu(), lengths), "lengths changed"
    pad = torch.ones(P, dtype=torch.bool)
    pad[steps] = False
    past = torch.zeros(N, T, dtype=torch.bool) if lengths is None else torch.arange(T)[None, :] >= lengths[:, None].long()

    def untouched(name, x, pad_fill, lo=0, hi=None):
        """the guard rows, the margins and the pad rows of an output [N + guard, P, ld]; returns the step rows' block"""
        v = x.float().cpu()
        assert bool((v[N:] == SENTINEL).all()), "%s: rows n >= N written" % name
        inner = torch.zeros(v.shape[2], dtype=torch.bool)
        inner[lo:hi] = True
        assert bool((v[:N][:, :, ~inner] == SENTINEL).all()), "%s: margins written" % name
        assert bool((v[:N][:, pad][:, :, inner] == pad_fill).all()), "%s: pad rows written" % name
        return v[:N, steps][:, :, inner]

    hv = untouched("h", h_buf, 0.0, MARGIN, MARGIN + nd * H)
    res = []
    for di, b in enumerate(keep):
        for k, before in b["before"].items():
            assert torch.equal(_bytes(b[k]), _bytes(before)), "%s changed" % k
        if b["hi0_before"] is not None:
            assert torch.equal(_bytes(b["hi"][0]), _bytes(b["hi0_before"])), "h_init changed"
        got = dict(h=hv[:, :, di * H:(di + 1) * H], rh=untouched("rh", b["rh"], SENTINEL),
                   dzg=untouched("dzg", b["dzg"], 0.0), dzc=untouched("dzc", b["dzc"], 0.0))
        for k, C in (("ru", 2 * H), ("c", H)):
            v = b[k].cpu()
            assert bool((v[N16 * T * C:] == SENTINEL).all()), "%s: guard tail written" % k
            body = v[:N16 * T * C]
            assert bool(torch.isfinite(body).all()) and bool((body.abs() <= 1).all()), "%s: not finite, or not written, somewhere" % k
            got[k] = torch.cat([_saved(body[N16 * t0 * C:N16 * t1 * C], N, t1 - t0, H, C // H) for t0, t1 in wins], 1)
        assert bool(torch.isfinite(got["rh"]).all()) and bool((got["rh"] != SENTINEL).all()), "rh: not finite, or not written, somewhere"
        for k in ("h", "dzg", "dzc"):
            assert bool(torch.isfinite(got[k]).all()), "%s is not finite" % k
            assert float(got[k][past].abs().max() if past.any() else 0) == 0.0, "%s is not 0 past the length" % k
        for wi in range(len(wins)):
            v = b["dhi"][wi].cpu()
            assert bool((v[N:] == SENTINEL).all()) and bool((v[:, :MARGIN] == SENTINEL).all()) and \
                bool((v[:, MARGIN + H:] == SENTINEL).all()), "dh_init: margins or rows n >= N written"
        got["dh_init"] = b["dhi"][0].cpu()[:N, MARGIN:MARGIN + H]
        res.append(got)
    return res


WORST = {}


def ratio(err, bound):
    """err / bound; an exact buffer (r * h from a zero state: bound 0) must be met exactly."""
    return err / bound if bound > 0 else (0.0 if err == 0 else math.inf)


def check_case(c, dev):
    got = run_case(c, dev)
    refs = references(c)
    bad = []
    for di, (g, r) in enumerate(zip(got, refs)):
        for k in BUFFERS:
            for against, bmax, bmean in r["bounds"][k]:
                emax, emean, _ = _dist(g[k], r[against][k], _valid(r["pure"], k))
                ratios = [ratio(emax, bmax)] + ([ratio(emean, bmean)] if bmean is not None else [])
                print("%s dir %d %-7s vs %-5s (%s): max %.3e / %.3e = %.2f%s" % (
                    case_id(c), di, k, against, r["source"][k], emax, bmax, ratios[0],
                    "" if bmean is None else "   mean %.3e / %.3e = %.2f" % (emean, bmean, ratios[1])))
                key = (c.H, c.form, k, against)
                WORST[key] = [max(a, b) for a, b in zip(WORST.get(key, [0, 0]), ratios + [0])]
                if not max(ratios) <= 1.0:
                    bad.append((di, k, against, ratios, r["figures"].get(k)))
    assert not bad, bad


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_gru_seq_kernels_meet_the_contract(dev, c):
    check_case(c, dev)


def test_worst_ratios_are_reported():
    """Prints, per H, form, buffer and reference, the worst error / bound of the cases above (max, mean)."""
    for key in sorted(WORST):
        print("worst H%-3d %-6s %-7s vs %-5s: max %.2f mean %.2f" % (key + tuple(WORST[key])))
