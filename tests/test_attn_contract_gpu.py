"""Every attention recurrence kernel against the float64 contracts of ns_taco2_attn_params, ns_taco1_attn_params,
ns_attention_step_params and ns_attention_step_bwd_params (tests/attn_ref.py, itself proven by
tests/test_attn_ref_cpu.py), through nspeech_amd.ops:
  step2     ns_taco2_attn_fwd / _bwd (csrc/attn.hip), the plain form (pv == NULL) and the projected-memory form, fp32
            storage, ops.F32_PASSES 0, 3 and 3 forward / 1 backward, at the smallest widths check_attn admits
            (A = 24 - not a multiple of the post-pass' 4 PU = 16 unit tile - and A = 8; E = 8, D1 = 16, D2 = 8)
  cluster2  ns_taco2_attn_cluster_fwd / _bwd (csrc/attn_cluster.hip), A = 64 and A = 256, fp32 and bf16 storage
  cluster1  ns_taco1_attn_cluster_fwd / _bwd (csrc/attn_gru.hip), A = 256, fp32 and bf16 storage
  one       ns_attention_step with and without pv / E2 / pv_out, with ctx_out2, fp32 and bf16 values, and
            ns_attention_step_bwd with has_carry 0 and 1.  ctx_rows is held by tests/test_decode_contract_gpu.py, beside
            ns_rows32's packed rows whose layout tests/decode_ref.py states.
Errors are measured against the references only, never against another kernel; every valid element of every output
buffer is compared.

Around each launch: memory rows are padded (padl_i > 0, Pi > padl_i + Ti) and the pad rows of keys, values and pv hold
1e30; where the ABI has a stride (q_sn, al_sn, ctx_sn, dq_sn, dce_sn, dco_sn) the operand is a column block of a wider
buffer whose margins hold a sentinel afterwards; inputs are bit-identical afterwards; slot 0 of every history is still
zero; align and de are exactly 0 from each row's length up to Tia; the `+=` outputs dkeys, dvalues, dv and dwcl are
prefilled and must come back as reference + prefill with their pad rows unchanged; a persistent kernel is launched twice
on the same work buffer (the `+=` outputs re-primed in between), its status word is 0 after each launch and the second
result is the one compared.

Tolerances, relative to scale = max |reference| of the buffer, all computed on the CPU per case (references()):
  fp32 rule  fp32 storage, unrounded or three-pass operands, against the pure reference: max |err| <= bound x scale,
             bound = max(2e-5 sqrt(S) for histories / 5e-5 sqrt(S) for gradients - the constants of
             test_gru_seq_gpu.py and test_lstm_contract_gpu.py -, 4 x the distance between the reference evaluated in
             float32 with permuted sums and the float64 evaluation).  Which term decided: see the table below.
  bf16 rule  bf16 storage and the one-pass backward of step2, the rule of test_lstm_contract_gpu.py: against the
             storage-exact reference max <= 2 x and mean <= 10 x the float32 emulation's distance, against the pure
             reference max <= 4 x and mean <= 2 x the storage-exact reference's own distance; floors: the fp32 rule's
             bound and, for the maximum against the storage-exact reference, 2 x one_flip().
             The storage-exact arrangements are read off the kernels (tests/attn_ref.py): bf16 storage rounds what is
             stored and nothing the loops carry; the 3 / 1 form runs its ns_gemm and LSTM-step products as three
             split-bf16 passes forward and on bf16-rounded operands backward, the hoisted dvalues product only where
             gemm_classify takes the matrix-core path (T_in a multiple of 4).  A single step (`one`) rounds nothing but
             the outputs it stores as bf16: their storage-exact reference is bf16(reference).
             (With the forward of the 3 / 1 form left unrounded in the arrangement, dp2 and df1 of n2s3t13-tia24-kw1 had
             mean errors of 2.1 and 1.6 bounds: the three passes' 2^-17 moved one gate gradient across a bf16 boundary of
             the one-pass operand, which reaches a sixth of those 48-value buffers.  The arrangement was incomplete, not
             the kernel: with the three passes in it that ratio is 0.01.)
Shapes (SHAPES, ordered from what the models run to what they never do; each line there says what it is for): one step
and one position; a length of 1 beside a full one; taps that cross slice and chunk boundaries, with an even and a short
filter; T_in = 256 with 32 positions per workgroup, with kw 7 and 8; Tia beyond the next multiple of 8; speaker rows and
an active clip over 9 steps; a second group of 32 utterances.  `one` has the same edges.
Every case walks its data seed until no prenet pre-activation lies within 100 bounds of zero (_inputs).

Found by this module: ns_taco2_attn_cluster_bwd lost a term of the location-filter carry with kw = 8 when a workgroup
owns all 32 positions of its slice (T_in >= 249): a slice's carry contributions span ts + kw - 1 = 39 positions and the
exchange published and gathered 38 (`TSMAX + 6`, sized for kw = 7), so tap 7 of a slice's last position never reached
the alignment gradient four positions into the next slice.  Worst error / bound before the fix, n2s3t256-kw8, fp32:
A = 256 de 20.4, dkeys 12.1, dwcl 8.7, dq 8.1, dv 3.8; A = 64 de 1.07, dkeys 1.11.  Fixed in csrc/attn_cluster.hip.
The header stated the taps at t + k - kw/2; kernels and reference use (kw - 1)/2 (conv1d 'same'): header corrected.
No other kernel was found wrong: the never-run plain form and the Tacotron-1 cluster at 32 positions per workgroup
meet the fp32 rule with room to spare.

Worst error / bound per family and form on the MI355X over all cases of the form (every test prints its own per buffer,
`pytest -s`; "exact" = against the storage-exact reference, "pure" = against the pure one; max, or max / mean).  The
fp32 rule's bound came from its constant (2e-5 / 5e-5 sqrt(S)) in every case of every family: four times the float32
emulation's distance was smaller everywhere (its largest value over all buffers and cases, as a fraction of the buffer's
maximum: step2 9.1e-7, cluster2 2.9e-6, cluster1 9.0e-7 - the S-step carry and the softmax do not amplify fp32 noise here).
  step2     plain / pv f32x00   pure:  every buffer <= 0.02
            plain / pv f32x33   pure:  ca 0.65  ga 0.36  hc 0.33  q 0.28  df1 0.22  dp2 0.10  dga 0.09  the rest <= 0.08
            plain / pv f32x31   histories as f32x33;  exact: dp2 0.02 / 0.01  the rest 0.00;  pure: at most 0.28 / 0.56
  cluster2  A64 / A256 f32      pure:  ca 0.06  q 0.02  the rest <= 0.01
            A64 / A256 bf16     exact: ga 0.50  dp2 0.25  df1 0.12  dq 0.12  dga 0.06  hc 0.03  the rest <= 0.02 (means <= 0.01);
                                pure: at most 0.25 / 0.50
  cluster1  f32                 pure:  every buffer <= 0.01
            bf16                exact: df1 0.50 / 0.30  dp2 0.50 / 0.29  dzg 0.25 / 0.53  dzc 0.25 / 0.16  hc 0.12 / 0.01  the
                                rest <= 0.06 / 0.00;  pure: at most 0.29 / 0.77 (dzg), else 0.26 / 0.53
  one       step f32            pure:  align, ctx, pv_out 0.02;   step bf16: align 0.01;  ctx, pv_out exact 0.00, pure 0.25 / 0.50
            bwd f32             pure:  every buffer <= 0.01;      bwd bf16:  da, de, gk <= 0.01;  dq, dctx exact 0.00, pure 0.25 / 0.50
0.25 / 0.50 against the pure reference is a kernel exactly as far from it as its storage format is; 0.50 and 0.25 against
the storage-exact reference are one flip at and below the top binade."""
import ctypes
import functools
import math
from collections import namedtuple

import pytest
import torch

import attn_ref as R

pytestmark = pytest.mark.gpu

f32, bf = torch.float32, torch.bfloat16
SENTINEL = 7.0
BIG = 1e30                      # pad rows of the memory operands: whatever reads them shows
MARGIN = 8
CLIP = 0.4

# N, S, Ti, lengths, kw, Tia (None = round_up(Ti, 8)), Dsp, clip
Shape = namedtuple("Shape", "name N S Ti lengths kw Tia Dsp clip")


def _mixed(N, Ti):
    return tuple((Ti, 1, max(1, Ti - 1), max(1, Ti // 2), max(1, Ti - 7))[i % 5] for i in range(N))


# ordered from what the models already run to what they never do
SHAPES = [Shape("n4s9t20-spk-clip", 4, 9, 20, (20, 13, 1, 17), 7, None, 16, CLIP),      # speaker rows and the clip over enough steps to act
          Shape("n3s4t9", 3, 4, 9, (9, 8, 1), 7, None, 0, 0.0),      # ragged last slice, one position per workgroup, length 1 beside 9
          Shape("n33s2t9", 33, 2, 9, _mixed(33, 9), 7, None, 0, 0.0),      # the second group of 32 utterances
          Shape("n1s1t1", 1, 1, 1, (1,), 7, None, 0, 0.0),      # seven of eight workgroups own nothing; softmax from empty shares
          Shape("n2s5t70-kw8", 2, 5, 70, (70, 65), 8, None, 0, 0.0),      # taps cross slices and the 64-position chunk; even width
          Shape("n2s5t70-kw5", 2, 5, 70, (70, 65), 5, None, 0, 0.0),
          Shape("n2s3t13-tia24-kw1", 2, 3, 13, (13, 7), 1, 24, 0, 0.0),      # Tia beyond the next multiple of 8
          Shape("n2s3t256", 2, 3, 256, (256, 249), 7, 256, 0, 0.0),      # ts = TSMAX exactly, the last slice partial
          # the widest filter at full slices - tap 7 of a slice's last position reaches 4 positions into the next slice, one
          # further than the carry exchange of the cluster backward was sized for
          Shape("n2s3t256-kw8", 2, 3, 256, (256, 249), 8, 256, 0, 0.0)]
SHAPES1 = [s for s in SHAPES if s.N != 33 and s.name != "n2s3t256-kw8"] + [Shape("n32s2t9", 32, 2, 9, _mixed(32, 9), 7, None, 0, 0.0)]

# family, form, widths (A, E, D1, D2), storage dtype, F32_PASSES forward / backward, projected-memory form
Case = namedtuple("Case", "family form A E D1 D2 dtype fp bp pv shape")


def _cases():
    out = []
    for fp, bp in ((0, 0), (3, 3), (3, 1)):
        for pv in (False, True):
            for s in SHAPES:
                A = 8 if s.name == "n1s1t1" else 24
                out.append(Case("step2", "%s-f32x%d%d" % ("pv" if pv else "plain", fp, bp), A, 8, 16, 8, f32, fp, bp, pv, s))
    for A in (64, 256):
        for dtype in (f32, bf):
            for s in SHAPES:
                out.append(Case("cluster2", "A%d-%s" % (A, "f32" if dtype == f32 else "bf16"), A, 16, 256, 128, dtype, 0, 0, True, s))
    for dtype in (f32, bf):
        for s in SHAPES1:
            out.append(Case("cluster1", "f32" if dtype == f32 else "bf16", 256, 16, 256, 128, dtype, 0, 0, True, s))
    return out


ALL_CASES = _cases()


def case_id(c):
    return "%s-%s-%s" % (c.family, c.form, c.shape.name)


def tia_of(s):
    return s.Tia if s.Tia else (s.Ti + 7) // 8 * 8


def rule_of(c):
    """"f32" or "bf16" for the case's gradients / histories (module docstring)."""
    if c.dtype == bf:
        return dict(hist="bf16", grad="bf16")
    return dict(hist="f32", grad="bf16" if c.bp == 1 else "f32")


# ------------------------------------------------------------------------------------------------------- the operands
def _draw(c, seed):
    s = c.shape
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g)
    away = lambda t, lo: torch.sign(t) * (lo + t.abs())           # no value within `lo` of zero: the ReLU kinks stay far
    A, E, D1, D2, Dsp = c.A, c.E, c.D1, c.D2, s.Dsp
    XA = D2 + Dsp + A
    x = dict(keys=r(s.N, s.Ti, A), values=r(s.N, s.Ti, E), f1=away(r(s.N, s.S + 1, D1), 0.5),
             W1c=r(E, D1) * 0.2 / E ** 0.5, W2=r(D1, D2) * 0.1 / D1 ** 0.5, b2=away(r(D2) * 0.4, 0.6),
             Wq=r(A, A) / A ** 0.5, v=r(A) * 2.0 / A ** 0.5, lengths=torch.tensor(s.lengths, dtype=torch.int32),
             spk=r(s.N, Dsp) if Dsp else None, cell_clip=s.clip)
    x["f1"][:, 0] = 0
    if c.family == "cluster1":
        x.update(Wg=r(XA, 2 * A) / XA ** 0.5, bg=r(2 * A) * 0.1, Wc=r(XA, A) / XA ** 0.5, bc=r(A) * 0.1)
    else:
        x.update(Watt=r(XA, 4 * A) * (3.0 if s.clip else 1.0) / XA ** 0.5, batt=r(4 * A) * 0.1, Wcl=r(s.kw, A))
    dhc = r(s.N, s.S + 1, A + E) * 0.3
    if c.dtype == bf:                         # what the kernel is handed as bf16, the references are handed rounded
        for k in ("values", "W1c", "W2", "Wq", "Watt", "Wg", "Wc", "spk"):
            if x.get(k) is not None:
                x[k] = R.bf16(x[k])
    return x, dhc


def fp32_bound(c, k, pure, emu32):
    """The fp32 rule's bound of buffer k (absolute), and which of its two terms decided it."""
    p = _cut(c, k, pure[k])
    scale = float(p.abs().max())
    const = (5e-5 if k in grad_names(c) else 2e-5) * math.sqrt(c.shape.S)
    emu_rel = _dist(_cut(c, k, emu32[k]), p)[0] / scale if scale else 0.0
    return max(const, 4 * emu_rel) * scale, "const" if const >= 4 * emu_rel else "emu"


def kink_margin(c, pure, emu32):
    """Per prenet layer: (the smallest |pre-activation| of the reference, 100 x the fp32-rule bound of the buffer it
    is stored in: p1, and xa for the second layer)."""
    return {z: (float(pure[z][:, 1:].abs().min()), 100 * fp32_bound(c, buf, pure, emu32)[0]) for z, buf in (("z1", "p1"), ("z2", "xa"))}


def _ref_fn(c):
    return R.taco1 if c.family == "cluster1" else R.taco2


def _data_key(c):
    return (c.family == "cluster1", c.A, c.E, c.D1, c.D2, c.dtype == bf, c.shape)


@functools.lru_cache(maxsize=None)
def _inputs(key):
    """Walks the data seed until no prenet pre-activation of the pure reference lies inside the noise of a ReLU kink
    (tests/test_attn_ref_cpu.py asserts the margin)."""
    c = next(c for c in ALL_CASES if _data_key(c) == key)
    base = 1000 * c.A + 17 * c.shape.N + 3 * c.shape.S + c.shape.Ti + c.shape.kw
    for seed in range(base, base + 64):
        x, dhc = _draw(c, seed)
        pure = _ref_fn(c)(x, dhc)
        emu32 = _ref_fn(c)(x, dhc, dtype=torch.float32, perm_seed=c.shape.N + c.shape.Ti)      # the fp32 rule's second term
        if all(got >= need for got, need in kink_margin(c, pure, emu32).values()):
            return x, dhc, pure, seed, emu32
    raise AssertionError("no seed keeps the prenet pre-activations of %s away from zero" % case_id(c))


def inputs(c):
    return _inputs(_data_key(c))


def hist_names(c):
    return R.TACO1_HIST if c.family == "cluster1" else R.TACO2_HIST


def grad_names(c):
    return R.TACO1_GRAD if c.family == "cluster1" else R.TACO2_GRAD


def bf16_step(x):
    return 2.0 ** (math.floor(math.log2(x)) - 7) if x > 0 else 0.0


def _dist(a, b):
    d = (a.double() - b.double()).abs()
    return float(d.max()), float(d.mean())


def _cut(c, k, t):
    """The part of a reference buffer the kernel under test owns."""
    if k in hist_names(c) or k in ("df1", "dp2", "dga", "dzg", "dzc", "dq", "de"):
        t = t[:, 1:]
    if k == "hc" and c.family == "cluster1":
        t = t[..., :c.A]                      # the caller forms the contexts
    return t


@functools.lru_cache(maxsize=None)
def _references(key, grad_rule, pv):
    c = next(c for c in ALL_CASES if _data_key(c) == key and rule_of(c)["grad"] == grad_rule and c.pv == pv)
    x, dhc, pure, _, emu32 = inputs(c)
    s = c.shape
    fn = _ref_fn(c)
    rules = rule_of(c)
    res = dict(pure=pure, exact=pure, bounds={}, source={}, figures={})
    if c.dtype == bf:
        xe = dict(x, pv=R.bf16(R.project_memory(x["values"], x["W1c"])))
        res["exact"] = fn(xe, dhc, bf16_storage=True)
        emu = fn(xe, dhc, dtype=torch.float32, perm_seed=s.N + s.Ti, bf16_storage=True)
    elif grad_rule == "bf16":                 # the one-pass backward: its products run on bf16-rounded operands
        xe = dict(x, pv=R.project_memory(x["values"], x["W1c"]).float()) if c.pv else x
        # (csrc/gemm.hip: gemm_classify sends a transposed-A product whose M = T_in is no multiple of 4 to the exact fp32
        # kernel, whatever f32_passes says - the hoisted dvalues product is then not rounded)
        kw = dict(bwd_operand=R.bf16, dvalues_rounded=s.Ti % 4 == 0, fwd_three_pass=c.fp == 3)
        res["exact"] = fn(xe, dhc, **kw)
        emu = fn(xe, dhc, dtype=torch.float32, perm_seed=s.N + s.Ti, **kw)
    for k in hist_names(c) + grad_names(c):
        p = _cut(c, k, pure[k])
        scale = float(p.abs().max())
        is_grad = k in grad_names(c)
        floor, res["source"][k] = fp32_bound(c, k, pure, emu32)
        if rules["grad" if is_grad else "hist"] == "f32":
            res["bounds"][k] = [("pure", floor, None)]
            continue
        e = _cut(c, k, res["exact"][k])
        emax, emean = _dist(_cut(c, k, emu[k]), e)
        dmax, dmean = _dist(e, p)
        # one value rounding to the neighbouring bf16: a buffer stored in bf16 moves by one step at its own magnitude; a
        # buffer computed from flipped values (the gradients are linear in the saved gates' derivative factors and in
        # the one-pass operands) by the same relative step
        flip = bf16_step(scale)
        res["figures"][k] = dict(scale=scale, emu_max=emax, emu_mean=emean, storage_max=dmax, storage_mean=dmean, one_flip=flip)
        res["bounds"][k] = [("exact", max(2 * emax, 2 * flip, floor), max(10 * emean, floor)),
                            ("pure", max(4 * dmax, floor), max(2 * dmean, floor))]
    return res


def references(c):
    return _references(_data_key(c), rule_of(c)["grad"], c.pv)


# ------------------------------------------------------------------------------------------------------------ the GPU side
def _rows(x, Pi, padl, fill, dtype, dev):
    """x [N, Ti, C] -> flat [N * Pi, C] with `fill` in the pad rows."""
    N, Ti, C = x.shape
    full = torch.full((N, Pi, C), fill, dtype=torch.float32)
    full[:, padl:padl + Ti] = x
    return full.to(dtype).reshape(-1).to(dev)


def _same(a, b):
    return torch.equal(a.view(torch.int16 if a.dtype == bf else torch.int32), b.view(torch.int16 if b.dtype == bf else torch.int32))


def _status(work):
    return int(work[:1].view(torch.int32).item())


def _prefill(ref, like):
    """Known non-zero values at a quarter to a half of the reference's magnitude (fp32-exact constants per element)."""
    scale = float(ref.abs().max()) or 1.0
    pat = torch.tensor([0.25, 0.375, 0.5], dtype=torch.float32)[torch.arange(like.numel()) % 3]
    return (pat * float(torch.tensor(scale, dtype=torch.float32))).reshape(like.shape)


def run_recurrence(c, dev):
    """Runs forward and backward of a step2 / cluster2 / cluster1 case; returns the outputs cut to [N, S(+1), .] on the
    CPU.  All layout assertions happen here."""
    from nspeech_amd import _lib as L
    from nspeech_amd import ops
    s = c.shape
    x, dhc, pure, _, _ = inputs(c)
    N, S, Ti, A, E, D1, D2, Dsp = s.N, s.S, s.Ti, c.A, c.E, c.D1, c.D2, s.Dsp
    S1, Tia, padl = S + 1, tia_of(s), 2
    Pi = padl + Ti + 3
    XA, HC = D2 + Dsp + A, A + E
    D = c.dtype
    taco1 = c.family == "cluster1"
    dv = lambda t, dtype=f32: t.to(dtype).contiguous().to(dev)
    z = lambda n, dtype=f32: torch.zeros(n, dtype=dtype, device=dev)
    keys = _rows(x["keys"], Pi, padl, BIG, f32, dev)
    values = _rows(x["values"], Pi, padl, BIG, D, dev)
    pv_cpu = R.project_memory(x["values"], x["W1c"])
    pv = _rows(pv_cpu.float(), Pi, padl, BIG, D, dev) if c.pv else None
    f1_cpu = x["f1"].clone()
    f1_cpu[:, 0] = BIG                                          # slot 0 of the hoisted frame term is nobody's
    f1 = dv(f1_cpu.reshape(-1))
    lengths = x["lengths"].to(dev)
    dhc_d = dv(dhc.reshape(-1))
    da0_cpu = torch.zeros(N, S1, Tia)
    da0_cpu[:, :, :Ti] = R.hoisted_da0(dhc, x["values"], A).float()
    da0 = dv(da0_cpu.reshape(-1)) if c.pv else None
    xa0 = torch.zeros(N, S1, XA)
    if Dsp:
        xa0[:, :, D2:D2 + Dsp] = x["spk"][:, None, :]
    hist = dict(p1=z(N * S1 * D1, D), xa=dv(xa0.reshape(-1), D), hc=z(N * S1 * HC, D), q=z(N * S1 * A), align=z(N * S1 * Tia))
    align_t = z(N * S1 * Tia, D)
    if taco1:
        hist.update(xc=dv(xa0.reshape(-1), D), ru=z(N * S1 * 2 * A), cc=z(N * S1 * A))
        hc0 = torch.zeros(N, S1, HC)
        hc0[:, :, A:] = SENTINEL                                # the context columns are the caller's
        hist["hc"] = dv(hc0.reshape(-1), D)
        weights = dict(w2=dv(x["W2"], D), wg=dv(x["Wg"], D), wc=dv(x["Wc"], D), wq=dv(x["Wq"], D), b2=dv(x["b2"]), bg=dv(x["bg"]),
                       bc=dv(x["bc"]), v=dv(x["v"]))
        grads = dict(df1=z(N * S1 * D1, D), dp2=z(N * S1 * D2, D), dzg=z(N * S1 * 2 * A, D), dzc=z(N * S1 * A, D), dq=z(N * S1 * A, D),
                     de=z(N * S1 * Tia))
        args = dict(dtype=ops.dt(hist["hc"]), N=N, S=S, Ti=Ti, Pi=Pi, padl_i=padl, Tia=Tia, A=A, E=E, D1=D1, D2=D2, lengths=lengths,
                    keys=keys, pv=pv, f1=f1, align_t=align_t, Dsp=Dsp, **weights)
        args.update(hist)
        bargs = dict(args, dhc=dhc_d, da0=da0, **grads)
        plus = {}
    else:
        hist.update(ca=z(N * S1 * A), ga=z(N * S1 * 4 * A, D))
        weights = dict(w1cT=dv(x["W1c"].t(), D), w2T=dv(x["W2"].t(), D), wattT=dv(x["Watt"].t(), D), wqT=dv(x["Wq"].t(), D),
                       w1c=dv(x["W1c"], D), w2=dv(x["W2"], D), watt=dv(x["Watt"], D), wq=dv(x["Wq"], D), b2=dv(x["b2"]),
                       batt=dv(x["batt"]), wcl=dv(x["Wcl"]), v=dv(x["v"]))
        grads = dict(df1=z((N * S1 + 1) * D1, D), dp2=z(N * S1 * D2, D), dga=z(N * S1 * 4 * A, D), dq=z(N * S1 * A, D), de=z(N * S1 * Tia))
        pre = dict(dkeys=_prefill(pure["dkeys"], torch.empty(N, Pi, A)), dvalues=_prefill(pure["dvalues"], torch.empty(N, Pi, E)),
                   dv=_prefill(pure["dv"], torch.empty(A)), dwcl=_prefill(pure["dwcl"], torch.empty(s.kw, A)))
        plus = {k: dv(t.reshape(-1)) for k, t in pre.items()}
        args = dict(dtype=ops.dt(hist["hc"]), N=N, S=S, Ti=Ti, Pi=Pi, padl_i=padl, Tia=Tia, A=A, E=E, D1=D1, D2=D2, kw=s.kw,
                    lengths=lengths, keys=keys, values=values, f1=f1, pv=pv, Dsp=Dsp, keys_t=z(N * A * Tia), align_t=align_t,
                    **weights)
        args.update(hist)
        wb = L.lib().ns_taco2_attn_work_bytes
        wb.restype = ctypes.c_size_t
        args["work"] = z((wb(ctypes.byref(ops._attn_params(args))) + 3) // 4 + N * D1)
        if c.fp == 3:                                              # the pre-split copies the model hands in with three passes
            hi = weights["wattT"].to(bf)
            args.update(wattT_hi=hi, wattT_lo=(weights["wattT"] - hi.float()).to(bf))
        bargs = dict(args, dhc=dhc_d, da0=da0, dctx_t=z(N * S1 * E, D), post_part=ops.attention_post_part(dev, N, Tia, A), **grads)
        bargs.update(plus)
    frozen = dict(keys=keys, f1=f1, dhc=dhc_d, lengths=lengths, **weights)
    if not taco1:
        frozen["values"] = values
    if c.pv:
        frozen.update(pv=pv, da0=da0)
    before = {k: t.clone() for k, t in frozen.items()}

    def reprime():
        for k, t in plus.items():
            t.copy_(pre[k].reshape(-1))

    try:
        ops.CELL_CLIP = s.clip
        if c.family == "step2":
            ops.F32_PASSES = c.fp
            ops.taco2_attn("fwd", **args)
            ops.F32_PASSES = c.bp
            ops.taco2_attn("bwd", **bargs)
        else:
            sup, wfl, run = ((ops.taco1_attn_cluster_supported, ops.taco1_attn_cluster_work_floats, ops.taco1_attn_cluster) if taco1
                             else (ops.taco2_attn_cluster_supported, ops.taco2_attn_cluster_work_floats, ops.taco2_attn_cluster))
            assert sup(**args), "the cluster kernel declines %s" % case_id(c)
            work = z(wfl(**bargs))
            for direction, a in (("fwd", args), ("bwd", bargs)):
                for _ in range(2):                                # the second launch re-initialises the exchange state
                    reprime()
                    run(direction, work, **a)
                    torch.cuda.synchronize()
                    assert _status(work) == 0, (direction, case_id(c))
        torch.cuda.synchronize()
    finally:
        ops.F32_PASSES, ops.CELL_CLIP = 0, 0.0

    for k, t in frozen.items():
        assert _same(t, before[k]), "%s changed" % k
    past = torch.arange(Tia)[None, :] >= x["lengths"][:, None].long()            # [N, Tia]
    widths = dict(p1=D1, xa=XA, xc=XA, hc=HC, ca=A, ga=4 * A, ru=2 * A, cc=A, q=A, align=Tia, df1=D1, dp2=D2, dga=4 * A, dzg=2 * A,
                  dzc=A, dq=A, de=Tia)
    got = {}
    for k, t in list(hist.items()) + list(grads.items()):
        v = t.float().cpu()[:N * S1 * widths[k]].view(N, S1, widths[k])
        assert bool(torch.isfinite(v).all()), "%s is not finite" % k
        v0 = v[:, 0].clone()
        if k in ("xa", "xc") and Dsp:
            v0[:, D2:D2 + Dsp] = 0
        if k == "hc" and taco1:
            assert bool((v[:, :, A:] == SENTINEL).all()), "hc: the context columns were written"
            v0[:, A:] = 0
        assert float(v0.abs().max()) == 0.0, "%s: slot 0 is not zero" % k
        if k in ("align", "de"):
            assert float(v[:, 1:][past[:, None, :].expand(N, S, Tia)].abs().max() if past.any() else 0) == 0.0, \
                "%s is not 0 from the length on" % k
            v = v[:, :, :Ti]
        got[k] = _cut(c, k, v)
    if not taco1:
        at = align_t.float().cpu().view(N, S1, Tia)[:, 1:, :Ti]
        assert torch.equal(at, got["align"].to(D).float()), "align_t is not align in the storage type"
        assert float(grads["df1"].float()[N * S1 * D1:].abs().max()) == 0.0, "the zero row behind df1 was written"
        pad = torch.ones(Pi, dtype=torch.bool)
        pad[padl:padl + Ti] = False
        for k, C in (("dkeys", A), ("dvalues", E)):
            v = plus[k].cpu().view(N, Pi, C)
            assert torch.equal(v[:, pad], pre[k][:, pad]), "%s: pad rows changed" % k
            got[k] = v[:, padl:padl + Ti].double() - pre[k][:, padl:padl + Ti].double()
        got["dv"] = plus["dv"].cpu().double() - pre["dv"].double()
        got["dwcl"] = plus["dwcl"].cpu().view(s.kw, A).double() - pre["dwcl"].double()
    return got


WORST = {}


def check(c, got, refs, names, tag, cut=True):
    bad = []
    for k in names:
        for against, bmax, bmean in refs["bounds"][k]:
            emax, emean = _dist(got[k], _cut(c, k, refs[against][k]) if cut else refs[against][k])
            ratios = [emax / bmax if bmax else float(emax > 0)] + ([emean / bmean] if bmean else [])
            print("%s %-7s vs %-5s: max %.3e / %.3e = %.2f%s  [%s]" % (
                tag, k, against, emax, bmax, ratios[0], "" if not bmean else "   mean %.3e / %.3e = %.2f" % (emean, bmean, ratios[1]),
                refs["source"].get(k, "")))
            key = (c.family, c.form, k, against)
            WORST[key] = [max(a, b) for a, b in zip(WORST.get(key, [0, 0]), ratios + [0])]
            if max(ratios) > 1.0:
                bad.append((k, against, ratios, refs["figures"].get(k)))
    assert not bad, bad


def check_case(c, dev):
    got = run_recurrence(c, dev)
    check(c, got, references(c), hist_names(c) + grad_names(c), case_id(c))


@pytest.mark.parametrize("c", [c for c in ALL_CASES if c.family == "step2"], ids=case_id)
def test_step_kernels_meet_the_contract(dev, c):
    check_case(c, dev)


@pytest.mark.parametrize("c", [c for c in ALL_CASES if c.family == "cluster2"], ids=case_id)
def test_taco2_cluster_meets_the_contract(dev, c):
    check_case(c, dev)


@pytest.mark.parametrize("c", [c for c in ALL_CASES if c.family == "cluster1"], ids=case_id)
def test_taco1_cluster_meets_the_contract(dev, c):
    check_case(c, dev)


def test_the_cluster_kernels_refuse_what_their_headers_say(dev):
    """Shapes the headers promise a refusal for; none of them is launched."""
    from nspeech_amd import ops
    one = torch.zeros(8, device=dev)
    base = dict(dtype=ops.dt(one), N=2, S=3, Ti=256, Pi=260, padl_i=2, Tia=256, A=64, E=16, D1=256, D2=128, kw=7, pv=one)
    assert ops.taco2_attn_cluster_supported(**base)
    assert not ops.taco2_attn_cluster_supported(**dict(base, Ti=257, Tia=264))
    for A in (8, 24, 128, 512):
        assert not ops.taco2_attn_cluster_supported(**dict(base, A=A))
    assert not ops.taco2_attn_cluster_supported(**dict(base, pv=None))
    ptrs = dict(keys=one, f1=one, w2=one, wg=one, wc=one, wq=one, b2=one, bg=one, bc=one, v=one, p1=one, xa=one, xc=one, hc=one,
                ru=one, cc=one, q=one, align=one)
    base1 = dict(dtype=ops.dt(one), N=2, S=3, Ti=256, Pi=260, padl_i=2, Tia=256, A=256, E=16, D1=256, D2=128, pv=one, **ptrs)
    assert ops.taco1_attn_cluster_supported(**base1)
    assert not ops.taco1_attn_cluster_supported(**dict(base1, Ti=257, Tia=264))
    assert not ops.taco1_attn_cluster_supported(**dict(base1, A=64))
    assert not ops.taco1_attn_cluster_supported(**dict(base1, pv=None))


# ------------------------------------------------------------------------------------------------- one step, one launch
# N, Ti, lengths, kw, Tia, A, E, E2 (0 = no pv), values dtype, ctx_out2
One = namedtuple("One", "N Ti lengths kw Tia A E E2 dtype out2")
ONE_CASES = [One(3, 9, (9, 8, 1), 7, 16, 24, 8, 0, f32, False), One(3, 9, (9, 8, 1), 7, 16, 24, 8, 16, f32, True),
             One(2, 70, (70, 65), 8, 72, 24, 8, 16, bf, True), One(2, 70, (70, 65), 5, 72, 8, 16, 0, bf, False),
             One(33, 13, _mixed(33, 13), 1, 24, 24, 8, 8, f32, False), One(2, 256, (256, 249), 7, 256, 64, 8, 16, f32, True)]


def one_id(o):
    return "N%d-T%d-kw%d-A%d-E%d-E2%d-%s%s" % (o.N, o.Ti, o.kw, o.A, o.E, o.E2, "f32" if o.dtype == f32 else "bf16", "-out2" if o.out2 else "")


@functools.lru_cache(maxsize=None)
def one_inputs(o):
    g = torch.Generator().manual_seed(o.N * 131 + o.Ti * 7 + o.kw + o.A)
    r = lambda *shape: torch.randn(*shape, generator=g)
    L = torch.tensor(o.lengths, dtype=torch.int32)
    valid = torch.arange(o.Ti)[None, :] < L[:, None].long()
    aprev = torch.softmax(torch.where(valid, r(o.N, o.Ti), torch.full((o.N, o.Ti), -float("inf"))), 1)
    cast = (lambda t: R.bf16(t)) if o.dtype == bf else (lambda t: t)
    return dict(keys=r(o.N, o.Ti, o.A), values=cast(r(o.N, o.Ti, o.E)), pv=cast(r(o.N, o.Ti, o.E2)) if o.E2 else None,
                q=r(o.N, o.A), aprev=aprev, Wcl=r(o.kw, o.A), v=r(o.A) * 2.0 / o.A ** 0.5, lengths=L,
                dctx=r(o.N, o.E) * 0.3, carry=r(o.N, o.E) * 0.3, gk=r(o.N, o.Ti, o.kw) * 0.1)


def _wide(x, ld, dev, dtype=f32, fill=SENTINEL):
    """x [N, C] as a column block (MARGIN columns in) of a [N, ld] buffer of sentinels."""
    full = torch.full((x.shape[0], ld), fill, dtype=torch.float32)
    full[:, MARGIN:MARGIN + x.shape[1]] = x
    return full.to(dtype).reshape(-1).to(dev)


def _block_of(buf, N, ld, C, what):
    v = buf.float().cpu().view(N, ld)
    assert bool((v[:, :MARGIN] == SENTINEL).all()) and bool((v[:, MARGIN + C:] == SENTINEL).all()), "%s: margins written" % what
    return v[:, MARGIN:MARGIN + C]


def _one_bounds(ref, emu, names, hist, stored_bf16=()):
    """The two rules of the module docstring for one step (S = 1).  emu = the same reference evaluated in float32.  An
    output the kernel stores as bf16 falls under the bf16 rule: its storage-exact reference is bf16(reference) - nothing
    else of a single step is rounded - and the emulation is bf16(emu)."""
    out = dict(pure=ref, exact=dict(ref), bounds={}, source={}, figures={})
    for k in names:
        scale = float(ref[k].abs().max())
        const = 2e-5 if k in hist else 5e-5
        emu_rel = _dist(emu[k], ref[k])[0] / scale if scale else 0.0
        floor = max(const, 4 * emu_rel) * scale
        out["source"][k] = "const" if const >= 4 * emu_rel else "emu"
        if k not in stored_bf16:
            out["bounds"][k] = [("pure", floor, None)]
            continue
        e = out["exact"][k] = R.bf16(ref[k])
        emax, emean = _dist(R.bf16(emu[k].double()), e)
        dmax, dmean = _dist(e, ref[k])
        flip = bf16_step(scale)
        out["figures"][k] = dict(scale=scale, emu_max=emax, emu_mean=emean, storage_max=dmax, storage_mean=dmean, one_flip=flip)
        out["bounds"][k] = [("exact", max(2 * emax, 2 * flip, floor), max(10 * emean, floor)),
                            ("pure", max(4 * dmax, floor), max(2 * dmean, floor))]
    return out


@pytest.mark.parametrize("o", ONE_CASES, ids=one_id)
def test_attention_step_meets_the_contract(dev, o):
    from nspeech_amd import ops
    x = one_inputs(o)
    N, Ti, Tia, A, E, E2, D = o.N, o.Ti, o.Tia, o.A, o.E, o.E2, o.dtype
    padl, Pi = 2, 2 + Ti + 3
    a = (x["keys"], x["values"], x["q"], x["aprev"], x["Wcl"], x["v"], x["lengths"])
    ref, emu = R.attention_step(*a, pv=x["pv"]), R.attention_step(*a, pv=x["pv"], dtype=torch.float32)
    keys_t = torch.zeros(N, A, Tia)
    keys_t[:, :, :Ti] = x["keys"].transpose(1, 2)
    keys_t = keys_t.reshape(-1).to(dev)
    values = _rows(x["values"], Pi, padl, BIG, D, dev)
    pv = _rows(x["pv"], Pi, padl, BIG, D, dev) if E2 else None
    q_sn, al_sn, ctx_sn, pv_sn = A + 2 * MARGIN, Tia + 2 * MARGIN, E + 2 * MARGIN, E2 + 2 * MARGIN
    ap = torch.zeros(N, Tia)
    ap[:, :Ti] = x["aprev"]
    q, aprev = _wide(x["q"], q_sn, dev), _wide(ap, al_sn, dev)
    aout = torch.full((N * al_sn,), SENTINEL, device=dev)
    ctx, ctx2 = (torch.full((N * ctx_sn,), SENTINEL, dtype=D, device=dev) for _ in range(2))
    pvo = torch.full((N * max(pv_sn, 1),), SENTINEL, dtype=D, device=dev)
    wcl, v, lengths = x["Wcl"].contiguous().to(dev), x["v"].to(dev), x["lengths"].to(dev)
    e_raw = torch.zeros(N * Tia, device=dev)
    frozen = dict(keys_t=keys_t, values=values, q=q, aprev=aprev, wcl=wcl, v=v)
    if E2:
        frozen["pv"] = pv
    before = {k: t.clone() for k, t in frozen.items()}
    ops.attention_step(values, N, Ti, Pi, padl, Tia, A, E, o.kw, lengths, keys_t, values, (q, MARGIN), q_sn, (aprev, MARGIN),
                       (aout, MARGIN), al_sn, (ctx, MARGIN), ctx_sn, (ctx2, MARGIN) if o.out2 else None, ctx_sn, wcl, v, e_raw,
                       pv=pv, E2=E2, pv_out=(pvo, MARGIN) if E2 else None, pv_out_sn=pv_sn)
    torch.cuda.synchronize()
    for k, t in frozen.items():
        assert _same(t, before[k]), "%s changed" % k
    al = _block_of(aout, N, al_sn, Tia, "aout")
    past = torch.arange(Tia)[None, :] >= x["lengths"][:, None].long()
    assert float(al[past].abs().max() if past.any() else 0) == 0.0, "align is not 0 from the length on"
    got = dict(align=al[:, :Ti], ctx=_block_of(ctx, N, ctx_sn, E, "ctx_out"))
    if o.out2:
        assert torch.equal(_block_of(ctx2, N, ctx_sn, E, "ctx_out2"), got["ctx"]), "ctx_out2 != ctx_out"
    else:
        assert bool((ctx2.float() == SENTINEL).all()), "ctx_out2 written without being asked for"
    names = ["align", "ctx"]
    if E2:
        got["pv_out"] = _block_of(pvo, N, pv_sn, E2, "pv_out")
        names.append("pv_out")
    else:
        assert bool((pvo.float() == SENTINEL).all())
    refs = _one_bounds(ref, emu, names, names, stored_bf16=("ctx", "pv_out") if D == bf else ())
    check(Case("one", "step-%s" % ("f32" if D == f32 else "bf16"), A, E, 0, 0, D, 0, 0, bool(E2), None), got, refs, names, one_id(o), cut=False)


@pytest.mark.parametrize("has_carry", [0, 1])
@pytest.mark.parametrize("o", ONE_CASES, ids=one_id)
def test_attention_step_bwd_meets_the_contract(dev, o, has_carry):
    from nspeech_amd import ops
    x = one_inputs(o)
    N, Ti, Tia, A, E, D, kw = o.N, o.Ti, o.Tia, o.A, o.E, o.dtype, o.kw
    padl, Pi = 2, 2 + Ti + 3
    a = (x["keys"], x["values"], x["q"], x["aprev"], x["Wcl"], x["v"], x["lengths"], x["dctx"])
    kw_ = dict(dctx_carry=x["carry"] if has_carry else None, gk_next=x["gk"] if has_carry else None)
    ref, emu = R.attention_step_bwd(*a, **kw_), R.attention_step_bwd(*a, dtype=torch.float32, **kw_)
    keys = _rows(x["keys"], Pi, padl, BIG, f32, dev)
    keys_t = torch.zeros(N, A, Tia)
    keys_t[:, :, :Ti] = x["keys"].transpose(1, 2)
    keys_t = keys_t.reshape(-1).to(dev)
    values = _rows(x["values"], Pi, padl, BIG, D, dev)
    q_sn, al_sn, dce_sn, dq_sn, dco_sn = A + 2 * MARGIN, Tia + 2 * MARGIN, E + 2 * MARGIN, A + 2 * MARGIN, E + 2 * MARGIN
    pad_t = lambda t: torch.cat([t, torch.zeros(N, Tia - Ti)], 1)
    q, aprev, acur = _wide(x["q"], q_sn, dev), _wide(pad_t(x["aprev"]), al_sn, dev), _wide(pad_t(ref["align"].float()), al_sn, dev)
    dctx_ext = _wide(x["dctx"], dce_sn, dev)
    carry = x["carry"].contiguous().to(dev) if has_carry else None
    gk_in = torch.full((N, Tia, 8), float("nan"))                 # without a carry nobody reads it
    if has_carry:
        gk_in.zero_()
        gk_in[:, :Ti, :kw] = x["gk"]
    gk = gk_in.reshape(-1).to(dev)
    da = torch.full((N * Tia,), SENTINEL, device=dev)
    dq = torch.full((N * dq_sn,), SENTINEL, dtype=D, device=dev)
    de = torch.full((N * al_sn,), SENTINEL, device=dev)
    dco = torch.full((N * dco_sn,), SENTINEL, dtype=D, device=dev)
    wcl, v, lengths = x["Wcl"].contiguous().to(dev), x["v"].to(dev), x["lengths"].to(dev)
    frozen = dict(keys=keys, keys_t=keys_t, values=values, q=q, aprev=aprev, acur=acur, dctx_ext=dctx_ext, wcl=wcl, v=v)
    before = {k: t.clone() for k, t in frozen.items()}
    ops.attention_step_bwd(values, N, Ti, Pi, padl, Tia, A, E, kw, lengths, keys, keys_t, values, (q, MARGIN), q_sn,
                           (acur, MARGIN), (aprev, MARGIN), al_sn, (dctx_ext, MARGIN), dce_sn, carry, gk, da, has_carry,
                           (dq, MARGIN), dq_sn, (de, MARGIN), (dco, MARGIN), dco_sn, wcl, v)
    torch.cuda.synchronize()
    for k, t in frozen.items():
        assert _same(t, before[k]), "%s changed" % k
    dev_ = _block_of(de, N, al_sn, Tia, "de_out")
    past = torch.arange(Tia)[None, :] >= x["lengths"][:, None].long()
    gko = gk.cpu().view(N, Tia, 8)
    dav = da.cpu().view(N, Tia)
    for name, t in (("de", dev_), ("da", dav), ("gk", gko)):
        assert float(t[past].abs().max() if past.any() else 0) == 0.0, "%s is not 0 from the length on" % name
    assert float(gko[:, :, kw:].abs().max() if kw < 8 else 0) == 0.0, "gk: taps past the filter width are not 0"
    got = dict(de=dev_[:, :Ti], da=dav[:, :Ti], gk=gko[:, :Ti, :kw], dq=_block_of(dq, N, dq_sn, A, "dq_out"),
               dctx=_block_of(dco, N, dco_sn, E, "dctx_out"))
    names = ["da", "de", "dq", "gk", "dctx"]
    refs = _one_bounds(ref, emu, names, (), stored_bf16=("dq", "dctx") if D == bf else ())
    check(Case("one", "bwd-%s-carry%d" % ("f32" if D == f32 else "bf16", has_carry), A, E, 0, 0, D, 0, 0, False, None), got, refs,
          names, one_id(o), cut=False)


def test_worst_ratios_are_reported():
    """Prints, per family, form, buffer and reference, the worst error / bound of the cases above (max, mean)."""
    for key in sorted(WORST):
        print("worst %-8s %-14s %-7s vs %-5s: max %.2f mean %.2f" % (key + tuple(WORST[key])))
