"""Every LSTM recurrence kernel against the float64 contract of ns_lstm_seq_params (tests/lstm_ref.py, itself proven
by tests/test_lstm_ref_cpu.py), through nspeech_amd.ops: the launch-per-step kernels (csrc/lstm.hip: six arithmetic
forms, both tilings, ns_lstm_seq_* and ns_lstm_seq2_*), the persistent BiLSTM clusters (csrc/lstm_cluster.hip: bf16,
the fp32-state forward, chains of 16, 8 and 4 rows) and the wide decoder kernels (csrc/lstm_wide.hip: bf16, `mixed`, the
pre-split planes, zoneout forward and backward).  Errors are measured against the references, never against another
kernel; every valid (n, t, u) of h, c, gates and dgates is compared.

Layout of every case: h, xg and dh are column blocks of wider buffers (8 columns of margin on either side), rows are
padded (padl, P > padl + T in most cases).  Afterwards the margins and the pad rows of the saved gates still hold their
sentinels, the pad rows of h and c are still zero, inputs are bit-identical, everything past a row's length is exactly
0, and a persistent kernel's status word is 0 after each of two launches on the same work buffer.

Tolerances, relative to scale = max |reference| of the buffer (references() below computes them on the CPU, per shape):
  fp32 rule  - a buffer stored in fp32 and computed from unrounded operands: against the pure reference,
               max <= 2e-5 sqrt(T) scale (dgates: 5e-5 sqrt(T) scale), the bounds test_gru_seq_gpu.py holds the same
               arithmetic to.
  bf16 rule  - a buffer stored in bf16 or computed from bf16-rounded operands:
               against the storage-exact reference of the arrangement: max <= 2 x and mean <= 10 x what a float32
               emulation of the same arrangement, summed in a permuted order, differs from it by at this shape;
               against the pure reference: max <= 4 x and mean <= 2 x the storage-exact reference's own distance.
               None of these four is ever tighter than the fp32 rule's bound for the buffer: the arrangement contains
               all of the fp32 form's arithmetic (at T = 1 nothing is rounded before it is compared and three of the
               four measured figures are 0).
  One flip   - why the maximum against the storage-exact reference is also never below 2 x one_flip().  A value
               rounds to the neighbouring bf16 when its fp32 value lies within the arithmetic's own error (about 1e-7:
               v_exp_f32 / v_rcp_f32 activations, summation order) of a rounding boundary: about one value in 1e4.  The
               emulation draws from the same lottery with other noise.  At the benchmark's sizes it always holds a few
               flips and its maximum is one bf16 step; at the shapes of this module (a few thousand values) it usually
               holds none, or one of a small value, and its maximum is fp32 noise - while the kernel draws its own.  On
               the MI355X, with the bound at 2 x the emulation's maximum alone, 18 of the 42 bf16-rule cases exceeded it
               by factors of exactly 2, 4, 16 ... up to 112: single flips of a value larger than the emulation's.  So the
               bound allows, a priori, what the 2 x is there for - one flip stacked on another - whatever the emulation
               drew: one_flip() is the bf16 step at the buffer's maximum for a buffer stored in bf16, and for a buffer
               computed from a flipped value that step times the largest weight and the cell's largest derivative.
               The mean against the storage-exact reference has the fp32 rule's bound as its floor for the same reason:
               a value flips with probability (fp32 error / bf16 step) and a flip costs one step, so flips add about
               the arithmetic's own fp32 error to the mean - what the fp32 rule bounds - and a flipped h reaches every
               later value of its row.  Measured: the cluster kernels' h at N 5, T 25, H 128 has a mean error of 4e-5
               (0.19 of that floor) where 10 x the emulation's mean, which drew no such flip, is 1.2e-7.
Zoneout masks and the clip are exact on both sides.

Found by this module: ns_lstm_seq_bwd and ns_lstm_wide_bwd with zoneout AND cell_clip rebuilt the plain cell's c' from
the saved gates without the clip (h' was o tanh of the clipped value): dgates off by 15 % (step, T = 25, H = 48) and
37 % (wide, T = 25, H = 256) of the maximum.  Fixed in csrc/lstm.hip and csrc/lstm_wide.hip.

Worst error / bound per family and form on the MI355X, over all cases of the form (every test prints its own per
buffer, `pytest -s`; "exact" = against the storage-exact reference, "pure" = against the pure one; max, or max / mean):
  step     f32x0            pure:  h 0.02  c 0.01  gates 0.01  dgates 0.00
           f32x3, f32x3s    pure:  h 0.10  c 0.11  gates 0.11  dgates 0.02
           f32x1, f32x1b    pure:  h 0.10  c 0.11  gates 0.11;  dgates exact 0.02 / 0.00, pure 0.25 / 0.07
           bf16             exact: h 0.25 / 0.00  c 0.07 / 0.01  gates 0.50 / 0.00  dgates 0.12 / 0.00;  pure: all 0.25 / 0.50
  cluster  bf16 (all rows)  exact: h 0.50 / 0.19  c 0.14 / 0.16  gates 0.50 / 0.16  dgates 0.25 / 0.07;  pure: at most 0.26 / 0.51
           f32state         pure:  h 0.09  c 0.09;  exact: gates 0.50 / 0.01  dgates 0.25 / 0.03;  pure: gates, dgates 0.25 / 0.50
  wide     wide_bf16        exact: h 0.25 / 0.00  c 0.01 / 0.00  gates 0.50 / 0.00  dgates 0.25 / 0.01;  pure: all 0.25 / 0.50
           wide_mixed       pure:  h 0.17  c 0.16  gates 0.13;  dgates exact 0.19 / 0.04, pure 0.25 / 0.09
           wide_planes      pure:  h 0.06  c 0.04  gates 0.09;  dgates exact 0.13 / 0.01, pure 0.25 / 0.08
0.25 / 0.50 against the pure reference is a kernel exactly as far from it as its storage format is (the bounds are 4 x
and 2 x that distance); 0.50 and 0.25 against the storage-exact reference are one flip at and below the top binade."""
import ctypes
import functools
import math
from collections import namedtuple

import pytest
import torch

import lstm_ref as R

pytestmark = pytest.mark.gpu

Case = namedtuple("Case", "family form N T H dirs masked fb clip zone padl tail opt")
Case.__new__.__defaults__ = (None,)
F, B, FB = (False,), (True,), (False, True)       # the directions of a call: forward, reverse, both (seq2 / cluster)
f32, bf = torch.float32, torch.bfloat16
MARGIN = 8                                        # columns on either side of a block in h, xg and dh
SENTINEL = 7.0
CLIP = 0.75

# storage type, f32_passes forward / backward, whT_hi + whT_lo, wh_bf16 + dgates_bf16, preset of the arrangement
Form = namedtuple("Form", "dtype fp bp split whb preset")
FORMS = {
    "f32x0": Form(f32, 0, 0, False, False, "pure"), "f32x3": Form(f32, 3, 3, False, False, "pure"),
    "f32x3s": Form(f32, 3, 3, True, False, "pure"), "f32x1": Form(f32, 3, 1, True, False, "mixed"),
    "f32x1b": Form(f32, 3, 1, True, True, "mixed"), "bf16": Form(bf, 0, 0, False, False, "bf16"),
    "f32state": Form(f32, 3, 0, True, False, "cluster_f32"),                  # cluster: fp32-state forward, bf16 backward
    "wide_bf16": Form(bf, 0, 0, False, False, "wide_bf16"), "wide_mixed": Form(f32, 3, 1, True, True, "wide_mixed"),
    "wide_planes": Form(f32, 3, 1, True, True, "wide_mixed"),
}

#              N   T   H  dirs masked fb  clip zone padl tail
STEP_SHAPES = [(1, 1, 16, F, False, 1.0, 0, False, 0, 0),       # one row, one step, one partial K chunk
               (33, 2, 48, B, True, 0.25, 0, False, 2, 3),      # one live row in the second 32-row block; 32 + 16 K
               (33, 3, 16, F, True, 1.0, 0, True, 1, 0),
               (33, 3, 48, B, True, 1.0, 0, True, 3, 2),        # zoneout against the time index, with lengths
               (17, 13, 256, F, True, 1.0, CLIP, False, 2, 2),  # the 8-unit x 16-row tiling
               (129, 3, 256, FB, True, 0.25, 0, False, 1, 1),   # ns_lstm_seq2_*, the large tiling at H >= 256
               (5, 25, 48, B, True, 1.0, CLIP, True, 0, 4)]     # clip and zoneout together
STEP_CASES = [Case("step", form, *s) for form in ("f32x0", "f32x3", "f32x3s", "f32x1", "f32x1b", "bf16") for s in STEP_SHAPES]
CLUSTER_CASES = [Case("cluster", "bf16", 1, 2, 64, FB, False, 1.0, 0, False, 0, 0),        # one workgroup, no exchange
                 Case("cluster", "bf16", 5, 3, 128, FB, True, 0.25, 0, False, 2, 2),
                 Case("cluster", "bf16", 17, 9, 192, FB, True, 1.0, CLIP, False, 1, 3),
                 Case("cluster", "bf16", 5, 25, 128, FB, True, 1.0, 0, False, 2, 2),
                 Case("cluster", "bf16", 17, 3, 512, FB, True, 1.0, 0, False, 3, 0),
                 Case("cluster", "f32state", 5, 9, 64, FB, True, 0.25, 0, False, 2, 2),
                 Case("cluster", "f32state", 17, 9, 256, FB, True, 1.0, CLIP, False, 1, 1)]
ROWS_CASES = [Case("cluster", "bf16", 17, 9, 128, FB, True, 1.0, 0, False, 2, 2, rows) for rows in (16, 8, 4)]
WIDE_CASES = [Case("wide", "wide_bf16", 1, 2, 256, F, False, 1.0, 0, False, 0, 0),
              Case("wide", "wide_bf16", 17, 9, 1024, F, True, 1.0, 0, True, 1, 0),
              Case("wide", "wide_bf16", 32, 3, 256, F, True, 0.25, CLIP, False, 2, 2),
              Case("wide", "wide_bf16", 5, 25, 256, F, True, 1.0, CLIP, True, 1, 1),
              Case("wide", "wide_mixed", 17, 3, 256, F, True, 1.0, 0, True, 1, 2),
              Case("wide", "wide_mixed", 32, 3, 1024, F, False, 1.0, CLIP, False, 2, 1),
              Case("wide", "wide_mixed", 1, 9, 1024, F, False, 0.25, 0, True, 1, 0),
              Case("wide", "wide_planes", 17, 9, 256, F, True, 1.0, 0, True, 1, 1),
              Case("wide", "wide_planes", 32, 2, 1024, F, True, 1.0, 0, False, 1, 0),
              Case("wide", "wide_bf16", 60, 3, 256, F, True, 1.0, 0, True, 1, 1, "bwd_only"),
              Case("wide", "wide_mixed", 60, 3, 256, F, True, 1.0, 0, False, 1, 1, "bwd_only")]
ALL_CASES = STEP_CASES + CLUSTER_CASES + ROWS_CASES + WIDE_CASES
BUFFERS = ("h", "c", "gates", "dgates")


def case_id(c):
    return "%s-%s-N%d-T%d-H%d-%s%s%s%s%s" % (c.family, c.form, c.N, c.T, c.H, "".join("fr"[d] for d in c.dirs),
                                             "-len" if c.masked else "", "-clip" if c.clip else "",
                                             "-zone" if c.zone else "", "-%s" % c.opt if c.opt else "")


def zone_of(c):
    thr = R.zone_threshold(0.25)
    return (thr, thr, 0x1234567 + c.N, 0x89ABCDE + c.T) if c.zone else None


@functools.lru_cache(maxsize=None)
def inputs(c):
    """The operands of a case, per direction, on the CPU: what both the references and the kernels are given."""
    g = torch.Generator().manual_seed(c.N * 1009 + c.T * 101 + c.H + 7 * len(c.dirs))
    form = FORMS[c.form]
    lengths = None
    if c.masked:
        lengths = torch.randint(1, c.T + 1, (c.N,), generator=g, dtype=torch.int32)
        lengths[0], lengths[-1] = c.T, 1
        if c.family == "wide":               # hand-set as in test_lstm_wide_split_gpu.py: 1, T, T - 1, T / 2 in turn
            lengths = torch.tensor([(1, c.T, max(1, c.T - 1), max(1, c.T // 2))[i % 4] for i in range(c.N)], dtype=torch.int32)
    dirs = []
    for _ in c.dirs:
        xg = torch.randn(c.N, c.T, 4 * c.H, generator=g) * (3.0 if c.clip else 1.0)
        W = torch.randn(c.H, 4 * c.H, generator=g) / c.H ** 0.5
        if form.dtype == bf:                 # the kernel sees bf16 weights: so does the reference
            W = R.bf16(W)
        W_bwd = R.bf16(W) if form.bp == 1 or c.form == "f32state" else W      # one bf16 pass / the bf16 backward call
        dirs.append(dict(xg=xg, W=W, W_bwd=W_bwd, dh=torch.randn(c.N, c.T, c.H, generator=g) * 0.3))
    return lengths, dirs


def rules(c):
    """Per buffer: "f32" or "bf16" (module docstring), from what the arrangement rounds."""
    r = R.PRESETS[FORMS[c.form].preset]
    return dict(h="bf16" if "h" in r else "f32", c="bf16" if "h" in r else "f32",
                gates="bf16" if "h" in r or "gates" in r else "f32", dgates="bf16" if r else "f32")


def _dist(a, b, valid):
    """max and mean |a - b| over the valid entries, and max |b| there."""
    v = valid[:, :, None].expand_as(b)
    d = (a.double() - b.double()).abs()[v]
    return float(d.max()), float(d.mean()), float(b.double().abs()[v].max())


def bf16_step(x):
    """The spacing of bf16 (8 significant bits) at magnitude x."""
    return 2.0 ** (math.floor(math.log2(x)) - 7) if x > 0 else 0.0


def one_flip(preset, scale, w_max, wb_max, partial_max):
    """Per buffer, the most that ONE value rounding to the neighbouring bf16 can move an element (module docstring,
    "One flip"), from the arrangement's rounding points, the buffers' magnitudes and the largest weight alone."""
    dz = bf16_step(scale["h"]) * w_max if "h" in preset else 0.0           # a flipped h[t-1][v] moves a pre-activation by step x |W[v, k]|
    ddh = max(bf16_step(scale["dgates"]) * wb_max if "bwd_operand" in preset else 0.0,     # a flipped operand of the backward product,
              bf16_step(partial_max) if "dh_partial" in preset else 0.0)                   # a flipped partial sum: both move dh[t-1]
    # c' = f c + i j with sig' <= 1/4, tanh' <= 1 and |i|, |j|, |f| <= 1;  dgates = (dc or dh) x factors of at most 1,
    # except d_f = dc c[t-1] f (1 - f) <= dc |c| / 4
    return dict(h=bf16_step(scale["h"]) if "h" in preset else 0.0,
                gates=bf16_step(scale["gates"]) if "h" in preset or "gates" in preset else 0.0,
                c=(1.25 + 0.25 * scale["c"]) * dz,
                dgates=max(bf16_step(scale["dgates"]) if "dgates" in preset else 0.0, ddh * max(1.0, 0.25 * scale["c"])))


@functools.lru_cache(maxsize=None)
def references(c):
    """Per direction: the pure and the storage-exact reference and BOUNDS[buffer] = a list of (against, max bound, mean
    bound or None), all from the CPU: the float32 permuted-order emulation of the arrangement measures the first pair."""
    lengths, dirs = inputs(c)
    preset = R.PRESETS[FORMS[c.form].preset]
    rule = rules(c)
    out = []
    for reverse, d in zip(c.dirs, dirs):
        kw = dict(lengths=lengths, reverse=reverse, forget_bias=c.fb, cell_clip=c.clip, zoneout=zone_of(c), dh=d["dh"])
        pure = R.lstm_seq(d["xg"], d["W"], **kw)
        res = dict(pure=pure, exact=pure, bounds={}, figures={})
        if preset:
            res["exact"] = R.lstm_seq(d["xg"], d["W"], W_bwd=d["W_bwd"], rounding=preset, **kw)
            perm = torch.randperm(c.H, generator=torch.Generator().manual_seed(c.H + c.T))
            emu = R.lstm_seq(d["xg"], d["W"], W_bwd=d["W_bwd"], rounding=preset, dtype=torch.float32, perm=perm, **kw)
        scales = {k: _dist(pure[k], pure[k], pure["valid"])[2] for k in BUFFERS}
        flip = one_flip(preset, scales, float(d["W"].abs().max()), float(d["W_bwd"].abs().max()),
                        res["exact"].get("dh_partial_max", 0.0))
        for k in BUFFERS:
            scale = scales[k]
            floor = (5e-5 if k == "dgates" else 2e-5) * math.sqrt(c.T) * scale
            if rule[k] == "f32":
                res["bounds"][k] = [("pure", floor, None)]
                continue
            emax, emean, _ = _dist(emu[k], res["exact"][k], pure["valid"])
            dmax, dmean, _ = _dist(res["exact"][k], pure[k], pure["valid"])
            res["figures"][k] = dict(scale=scale, emu_max=emax, emu_mean=emean, storage_max=dmax, storage_mean=dmean,
                                     one_flip=flip[k])
            res["bounds"][k] = [("exact", max(2 * emax, 2 * flip[k], floor), max(10 * emean, floor)),
                                ("pure", max(4 * dmax, floor), max(2 * dmean, floor))]
        out.append(res)
    return out


# ------------------------------------------------------------------------------------------------------------ the GPU side
def _block(N, P, padl, T, ld, off, x, fill, dev, dtype=f32):
    """[N * P, ld] filled with `fill`, x [N, T, C] at rows padl .. padl + T, columns off .. off + C."""
    full = torch.full((N, P, ld), fill, dtype=torch.float32)
    full[:, padl:padl + T, off:off + x.shape[2]] = x
    return full.to(dtype).reshape(-1).to(dev)


def _status(work, word=0):
    return int(work[word:word + 1].view(torch.int32).item())


def run_case(c, dev):
    """Runs the case's forward and backward calls; returns per direction the outputs cut to [N, T, .] on the CPU.  All
    layout assertions happen here."""
    from nspeech_amd import _lib as L
    from nspeech_amd import ops
    form = FORMS[c.form]
    N, T, H, padl = c.N, c.T, c.H, c.padl
    P = padl + T + c.tail
    D, nd = form.dtype, len(c.dirs)
    lengths, dirs = inputs(c)
    lens_d = None if lengths is None else lengths.to(dev)
    ld_x, ld_h = 4 * H + 2 * MARGIN, nd * H + 2 * MARGIN
    nan = float("nan")
    h_buf = torch.full((N, P, ld_h), SENTINEL, dtype=D)
    h_buf[:, :, MARGIN:MARGIN + nd * H] = 0                      # the history's pad rows are the zero initial state
    h_buf = h_buf.reshape(-1).to(dev)
    dh_buf = torch.full((N, P, ld_h), nan)
    for di, d in enumerate(dirs):
        dh_buf[:, padl:padl + T, MARGIN + di * H:MARGIN + (di + 1) * H] = d["dh"]
    dh_buf = dh_buf.reshape(-1).to(dev)
    dh_before = dh_buf.clone()
    planes = c.form == "wide_planes"
    hb16 = c.form == "f32state" or planes
    hb_buf = torch.full((N * P * ld_h,), SENTINEL, dtype=bf, device=dev) if hb16 else None
    hlo_buf = torch.full((N * P * ld_h,), SENTINEL, dtype=bf, device=dev) if planes else None
    bwd_dtype = bf if c.form == "f32state" else D               # the fp32-state cluster's backward is the bf16 call
    seq_work = L.lib().ns_lstm_seq_work_bytes
    seq_work.restype = ctypes.c_size_t
    keep, fps, bps = [], [], []
    try:
        ops.CELL_CLIP = c.clip
        for di, (reverse, d) in enumerate(zip(c.dirs, dirs)):
            b = dict(xg=_block(N, P, padl, T, ld_x, MARGIN, d["xg"], nan, dev),
                     c=torch.zeros(N * P * H, device=dev),
                     gates=torch.full((N * P * 4 * H,), SENTINEL, dtype=bf if c.form == "f32state" else D, device=dev),
                     dgates=torch.full((N * P * 4 * H,), SENTINEL, dtype=bwd_dtype, device=dev),
                     whT=d["W"].t().contiguous().to(D).to(dev), wh=d["W_bwd"].to(bwd_dtype).to(dev).contiguous())
            if c.form in ("f32x1", "f32x1b", "wide_mixed", "wide_planes"):
                b["wh"] = d["W"].to(dev).contiguous()             # fp32 weights; the one bf16 pass rounds them itself ...
            b["xg_before"] = b["xg"].clone()
            if form.split:
                b["hi"] = b["whT"].to(bf)
                b["lo"] = (b["whT"] - b["hi"].float()).to(bf)
            if form.whb:                                          # ... or reads the caller's bf16 copy
                b["wh_bf16"] = d["W_bwd"].to(bf).to(dev).contiguous()
                b["dgates_bf16"] = torch.full((N * P * 4 * H,), SENTINEL, dtype=bf, device=dev)
            off = MARGIN + di * H
            ops.F32_PASSES = form.fp
            fp = ops.lstm_seq_params(N, T, H, P, padl, b["xg"], ld_x, b["whT"], None, lens_d, reverse, h_buf, ld_h, b["c"],
                                     b["gates"], xg_off=MARGIN, h_off=off, forget_bias=c.fb, whT_hi=b.get("hi"),
                                     whT_lo=b.get("lo"), zoneout=zone_of(c), h_bf16=hb_buf, h_bf16_off=off, ld_h_bf16=ld_h,
                                     h_lo_bf16=hlo_buf, h_lo_bf16_off=off)
            ops.F32_PASSES = form.bp
            bp = ops.lstm_seq_params(N, T, H, P, padl, b["xg"], ld_x, None, b["wh"], lens_d, reverse,
                                     hb_buf if c.form == "f32state" else h_buf, ld_h, b["c"], b["gates"], dh=dh_buf, ld_dh=ld_h,
                                     dgates=b["dgates"], xg_off=MARGIN, h_off=off, dh_off=off, forget_bias=c.fb,
                                     wh_bf16=b.get("wh_bf16"), dgates_bf16=b.get("dgates_bf16"), zoneout=zone_of(c))
            b["work"] = torch.zeros((seq_work(ctypes.byref(bp)) + 3) // 4, device=dev)
            bp.work = ops.ptr(b["work"])
            keep.append(b), fps.append(fp), bps.append(bp)

        def persistent(direction, call, work, supported):
            assert supported, "%s declines %s of %s" % (c.family, direction, case_id(c))
            for _ in range(2):                                    # the second launch re-initialises the exchange state
                call()
                torch.cuda.synchronize()
                assert _status(work) == 0, (direction, case_id(c))

        if c.family == "step":
            if nd == 2:
                ops.lstm_seq2("fwd", fps[0], fps[1])
                ops.lstm_seq2("bwd", bps[0], bps[1])
            else:
                ops.lstm_seq_call("fwd", fps[0])
                ops.lstm_seq_call("bwd", bps[0])
        elif c.family == "cluster":
            work = torch.zeros(ops.lstm_cluster_work_floats(fps[0]), device=dev)
            persistent("fwd", lambda: ops.lstm_cluster("fwd", fps[0], fps[1], work), work,
                       ops.lstm_cluster_supported(fps[0], fps[1], False))
            if c.opt:
                assert (_status(work, 1) or 16) == c.opt, "NS_CLUSTER_ROWS=%d ran the %d-row form" % (c.opt, _status(work, 1) or 16)
            persistent("bwd", lambda: ops.lstm_cluster("bwd", bps[0], bps[1], work), work,
                       ops.lstm_cluster_supported(bps[0], bps[1], True))
            if c.opt:
                assert (_status(work, 1) or 16) == c.opt
        else:
            work = torch.zeros(ops.lstm_wide_work_floats(fps[0]), device=dev)
            if c.opt == "bwd_only":                               # beyond 32 rows the forward pass keeps the step launches
                ops.lstm_seq_call("fwd", fps[0])
            else:
                persistent("fwd", lambda: ops.lstm_wide("fwd", fps[0], work), work, ops.lstm_wide_supported(fps[0], False))
            persistent("bwd", lambda: ops.lstm_wide("bwd", bps[0], work), work, ops.lstm_wide_supported(bps[0], True))
        torch.cuda.synchronize()
    finally:
        ops.F32_PASSES, ops.CELL_CLIP = 0, 0.0

    hv = h_buf.float().cpu().view(N, P, ld_h)
    pad = torch.ones(P, dtype=torch.bool)
    pad[padl:padl + T] = False
    inside = slice(MARGIN, MARGIN + nd * H)
    assert bool((hv[:, :, :MARGIN] == SENTINEL).all()) and bool((hv[:, :, MARGIN + nd * H:] == SENTINEL).all()), "h: margins written"
    assert float(hv[:, pad, inside].abs().max() if pad.any() else 0) == 0.0, "h: pad rows written"
    assert torch.equal(dh_buf.view(torch.int32), dh_before.view(torch.int32)), "dh changed"
    past = torch.zeros(N, T, dtype=torch.bool) if lengths is None else torch.arange(T)[None, :] >= lengths[:, None].long()
    res = []
    for di, b in enumerate(keep):
        off = MARGIN + di * H
        assert torch.equal(b["xg"].view(torch.int32), b["xg_before"].view(torch.int32)), "xg changed"
        got = dict(h=hv[:, padl:padl + T, off:off + H])
        for k, C in (("c", H), ("gates", 4 * H), ("dgates", 4 * H), ("dgates_bf16", 4 * H)):
            if k not in b:
                continue
            v = b[k].float().cpu().view(N, P, C)
            if k == "c":
                assert float(v[:, pad].abs().max() if pad.any() else 0) == 0.0, "c: pad rows written"
            else:
                assert bool((v[:, pad] == SENTINEL).all()), "%s: pad rows written" % k
            got[k] = v[:, padl:padl + T]
        for k, v in got.items():
            assert float(v[past].abs().max() if past.any() else 0) == 0.0, "%s is not 0 past the length" % k
            assert bool(torch.isfinite(v).all()), "%s is not finite" % k
        if "dgates_bf16" in got:                                  # the bf16 copy is the rounded fp32 gradient
            assert torch.equal(got["dgates_bf16"], got["dgates"].to(bf).float()), "dgates_bf16 != bf16(dgates)"
        if hb16 and c.opt != "bwd_only":
            hb = hb_buf.float().cpu().view(N, P, ld_h)
            assert bool((hb[:, :, :MARGIN] == SENTINEL).all()) and bool((hb[:, :, MARGIN + nd * H:] == SENTINEL).all())
            hi = hb[:, padl:padl + T, off:off + H]
            assert torch.equal(hi, got["h"].to(bf).float()), "h_bf16 != bf16(h)"
            if planes:                                            # hi + lo = the split of the stored h
                lo = hlo_buf.float().cpu().view(N, P, ld_h)[:, padl:padl + T, off:off + H]
                assert torch.equal(lo, (got["h"] - hi).to(bf).float()), "h_lo_bf16 != bf16(h - bf16(h))"
        res.append(got)
    return res


WORST = {}


def check_case(c, dev):
    got = run_case(c, dev)
    refs = references(c)
    bad = []
    for di, (g, r) in enumerate(zip(got, refs)):
        for k in BUFFERS:
            for against, bmax, bmean in r["bounds"][k]:
                emax, emean, _ = _dist(g[k], r[against][k], r["pure"]["valid"])
                ratios = [emax / bmax] + ([emean / bmean] if bmean is not None else [])
                print("%s dir %d %-6s vs %-5s: max %.3e / %.3e = %.2f%s" % (
                    case_id(c), di, k, against, emax, bmax, ratios[0],
                    "" if bmean is None else "   mean %.3e / %.3e = %.2f" % (emean, bmean, ratios[1])))
                key = (c.family, c.form, k, against)
                WORST[key] = [max(a, b) for a, b in zip(WORST.get(key, [0, 0]), ratios + [0])]
                if max(ratios) > 1.0:
                    bad.append((di, k, against, ratios, r["figures"].get(k)))
    assert not bad, bad


@pytest.mark.parametrize("c", STEP_CASES, ids=case_id)
def test_step_kernels_meet_the_contract(dev, c):
    check_case(c, dev)


@pytest.mark.parametrize("c", CLUSTER_CASES, ids=case_id)
def test_cluster_kernels_meet_the_contract(dev, c):
    check_case(c, dev)


@pytest.mark.parametrize("c", ROWS_CASES, ids=case_id)
def test_cluster_row_forms_meet_the_contract(dev, c, monkeypatch):
    monkeypatch.setenv("NS_CLUSTER_ROWS", str(c.opt))
    check_case(c, dev)


@pytest.mark.parametrize("c", WIDE_CASES, ids=case_id)
def test_wide_kernels_meet_the_contract(dev, c):
    check_case(c, dev)


def test_worst_ratios_are_reported():
    """Prints, per family, form, buffer and reference, the worst error / bound of the cases above (max, mean)."""
    for key in sorted(WORST):
        print("worst %-8s %-12s %-6s vs %-5s: max %.2f mean %.2f" % (key + tuple(WORST[key])))
