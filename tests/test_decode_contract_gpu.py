"""The kernels of free-running synthesis against the float64 contracts of tests/decode_ref.py (itself proven by
tests/test_decode_ref_cpu.py), every one through _lib.struct / _lib.call or the library's own entry:
  decode2   ns_taco2_decode (csrc/attn_cluster.hip), forms (A, E, D) = (64, 64, 64) and (256, 512, 1024), N 1 and 2, fp32 / bf16
  decode1   ns_taco1_decode (csrc/attn_gru.hip), A = D1 = D = 256, D2 = 128, N 1, 2, 3, 5 and max_rows + 1, fp32 / bf16
  rows32    ns_rows32 (csrc/rows32.hip), all 32 instantiations CELL x APK x THREE x TWO (x RG 2 / 4 / 8 under APK), with
            ns_rows32_pack (ldw > C) and ns_rows32_pack_rows (col0 > 0)
  step      ns_lstm_step (csrc/lstm.hip): fp32 at f32_passes 0 - 3 with and without pre-split weights, bf16, both tilings
  ctxrows   ns_attention_step with ctx_rows (the ONE_CASES of tests/test_attn_contract_gpu.py with N <= 32)
  keys      ns_taco2_keys_transpose / _add
Errors are measured against the references only; every valid element of every written buffer is compared.

Around each launch: memory rows are padded (padl_i > 0, Pi > padl_i + Ti) and the pad rows of keys, values and pv hold
1e30; f1 holds 1e30 in every slot but the one the header says is read; where the ABI has a stride the operand is a
column block of a wider buffer whose margins hold a sentinel afterwards; inputs are bit-identical afterwards; slot 0 of
every history is still zero; align is exactly 0 from each row's length up to Tia; hc's context columns (not listed as
written) keep their sentinel; a persistent call runs twice on the same `work`, filled with 0xFF bytes (NaN) before the
first call, its status word is 0 after each call and the two results are bit-equal.

Bounds, computed on the CPU per case (loop_references / step bounds of tests/decode_ref.py), nothing fitted:
  loops     the rules of tests/test_attn_contract_gpu.py unchanged: fp32 storage max |err| <= max(2e-5 sqrt(S), 4 x the
            float32-permuted emulation's distance) x max |reference|; bf16 storage the bf16 rule (exact: max <= 2 x, mean
            <= 10 x the emulation's distance, floor 2 x one flip; pure: max <= 4 x, mean <= 2 x the storage's own distance).
  products  per element of the pre-activation, u = 2^-24, mag = |a|.|w| + |bias| + |add| + |xg|: exact-product forms (fp32
            at f32_passes 0; bf16; one pass against the bf16-rounded operands) 2 (K + 4) u mag; three passes min(that +
            3 x 2^-16 mag - the split's truncation, decode_ref.py -, 3e-5 max|a| max|w| sqrt(K)); two passes the
            three-pass bound + 2^-9 mag (tests/test_gemm_epilogue_gpu.py).  Carried to h and c by decode_ref.cell_bounds, to
            y by dense_bound; a value read back from (hi, lo) rows adds 2^-16 |value|; h stored as bf16 adds 2^-8 (|h| + b_h).

Cases added to the issue's tables: step H = 256 at N = 257 is the smallest N whose 16 x ceil(N / 32) big tiles exceed 128
(lstm_step_launch2); rows32 K = 2080 appears with fp32 rows too (the RG = 8 loop's second pass does not depend on APK);
ctxrows leaves out the N = 33 case of ONE_CASES, which ns_attention_step refuses with ctx_rows (asserted, no launch).

Measured on the MI355X: 129 cases (28 decode2, 12 decode1, 45 rows32, 24 step, 10 ctxrows, 6 keys, 4 table / refusal /
report tests) in 2.4 s of wall time; the slowest case takes 0.27 s (the first launch of the module), every other at most
0.25 s.  The (256, 512, 1024) form ran: nothing skipped.  No kernel was found wrong.  Worst error / bound per family
(every test prints its own per buffer, `pytest -s`; test_worst_ratios_are_reported the table):
  decode2   A64 f32 pure: h2 0.06, the rest <= 0.02;  A256 f32 pure: ca 0.04, hc 0.03, the rest <= 0.02
            A64 / A256 bf16 exact: ga 0.12 (A64), h2 0.01, the rest 0.00;  pure: p1, xa, hc, ga 0.50, h2 0.04, the rest <= 0.02
  decode1   f32 pure: every buffer <= 0.01;  bf16 exact: 0.00;  pure: p1, xa, xc, hc 0.50, y2 0.02, the rest 0.01
  rows32    dense three passes: y 0.22 (packed operand), 0.04 (fp32 rows), rows 0.09;  one pass: y 0.04, rows 0.28
            cell three passes: c 0.03, h 0.02;  one pass: c, h 0.00, rows 0.06
  step      f0, f1, f1s <= 0.01;  f2 / f2s: c 0.37, h 0.16;  f3 / f3s: c 0.04, h 0.02;  bf16: c 0.01, h 0.93
  ctxrows   0.13;  keys: bit-exact.
0.50 against the pure reference is a kernel exactly as far from it as its storage format is; the 0.93 of a bf16 h is the
store's own rounding (up to 2^-8 |h|, the term the bound adds for it) beside an error of the fp32 value that is 100 times
smaller (c, 0.01).  The fp32 rule's bound came from its constant in every loop case."""
import ctypes
import functools
import math
from collections import namedtuple

import pytest
import torch

import attn_ref as AR
import decode_ref as R
from test_attn_contract_gpu import (BIG, CLIP, MARGIN, ONE_CASES, SENTINEL, _block_of, _dist, _one_bounds, _rows, _same, _status,
                                    _wide, bf16_step, one_id, one_inputs)

pytestmark = pytest.mark.gpu

f32, bf = torch.float32, torch.bfloat16
D1, D2 = 256, 128
HUGE = 3e38                     # finite garbage where the packed-row contract allows any finite value
WORST = {}


def _note(family, form, k, ratio):
    key = (family, form, k)
    WORST[key] = max(WORST.get(key, 0.0), ratio)


# ============================================================================================ the two decoder loops
Loop = namedtuple("Loop", "family name N S Ti Tia lengths kw Dsp clip A E D dtype")


def _loop_cases():
    out = []
    small = [("s1t9", 1, 9, 16, (9, 1), 7, 0, 0.0), ("s2t9-kw8-spk", 2, 9, 16, (9, 1), 8, 16, 0.0),
             ("s9t9-clip", 9, 9, 16, (9, 1), 7, 0, CLIP), ("s9t9-kw8-spk", 9, 9, 16, (9, 1), 8, 16, 0.0),
             ("s2t256", 2, 256, 256, (256, 255), 7, 0, 0.0), ("s2t256-kw8", 2, 256, 256, (256, 255), 8, 0, 0.0)]
    for dtype in (f32, bf):
        for N in (1, 2):
            for name, S, Ti, Tia, L, kw, Dsp, clip in small:
                out.append(Loop("decode2", "A64-%s" % name, N, S, Ti, Tia, L[:N], kw, Dsp, clip, 64, 64, 64, dtype))
            # 8 N + 64 + 128 workgroups, every one resident: skipped where ns_taco2_decode_supported says 0
            out.append(Loop("decode2", "A256-s3t37" + ("-clip" if N == 2 else ""), N, 3, 37, 40, (37, 20)[:N], 7, 0,
                            CLIP if N == 2 else 0.0, 256, 512, 1024, dtype))
        # single row; pair; pair + single; two pairs + single; two launches (ns_taco1_decode_max_rows() + 1 = 17 on 256 CUs)
        t1 = [("n1s1t9", 1, 1, 9, 16, (9,), 0, 8), ("n2s9t20-spk", 2, 9, 20, 24, (20, 13), 16, 24),
              ("n3s2t9", 3, 2, 9, 16, (9, 8, 1), 0, 8), ("n5s2t13-spk", 5, 2, 13, 16, (13, 7, 1, 13, 10), 16, 24),
              ("n2s2t256", 2, 2, 256, 256, (256, 249), 0, 24), ("n17s2t5", 17, 2, 5, 8, tuple((5, 1, 4, 3, 2)[i % 5] for i in range(17)), 0, 8)]
        for name, N, S, Ti, Tia, L, Dsp, E in t1:
            out.append(Loop("decode1", name, N, S, Ti, Tia, L, 0, Dsp, 0.0, 256, E, 256, dtype))
    return out


LOOP_CASES = _loop_cases()


def loop_id(c):
    return "%s-%s-n%d-%s" % (c.family, c.name, c.N, "f32" if c.dtype == f32 else "bf16")


def loop_names(c):
    return R.TACO2_DECODE if c.family == "decode2" else R.TACO1_DECODE


def _loop_fn(c):
    return R.taco2_decode if c.family == "decode2" else R.taco1_decode


def _draw_loop(c, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g)
    away = lambda t, lo: torch.sign(t) * (lo + t.abs())
    A, E, D, Dsp, N = c.A, c.E, c.D, c.Dsp, c.N
    XA = D2 + Dsp + A
    rnd = (lambda t: AR.bf16(t)) if c.dtype == bf else (lambda t: t)
    x = dict(keys=r(N, c.Ti, A), values=rnd(r(N, c.Ti, E)), W2=rnd(r(D1, D2) * 0.1 / D1 ** 0.5), b2=away(r(D2) * 0.4, 0.6),
             Wq=rnd(r(A, A) / A ** 0.5), v=r(A) * 2.0 / A ** 0.5, lengths=torch.tensor(c.lengths, dtype=torch.int32),
             spk=rnd(r(N, Dsp)) if Dsp else None, cell_clip=c.clip)
    W1c = r(E, D1) * 0.2 / E ** 0.5
    x["pv"] = rnd((x["values"].double() @ W1c.double()).float())
    f1 = torch.full((N, c.S + 1, D1), BIG)
    f1[:, 1] = away(r(N, D1) * 0.4, 0.5)
    x["f1"] = f1
    x["wpf"], x["bpf"] = r(D, D1) * 0.1 / D ** 0.5, away(r(D1) * 0.4, 0.5)
    if c.family == "decode2":
        gain = 2.0 if c.clip else 1.0
        K1 = A + E + D
        x.update(Watt=rnd(r(XA, 4 * A) * (3.0 if c.clip else 1.0) / XA ** 0.5), batt=r(4 * A) * 0.1, Wcl=r(c.kw, A),
                 w_l1=r(K1, 4 * D) * gain / K1 ** 0.5, b_l1=r(4 * D) * 0.1, w_l2=r(2 * D, 4 * D) * gain / (2 * D) ** 0.5,
                 b_l2=r(4 * D) * 0.1)
    else:
        x.update(Wg=rnd(r(XA, 2 * A) / XA ** 0.5), bg=r(2 * A) * 0.1, Wc=rnd(r(XA, A) / XA ** 0.5), bc=r(A) * 0.1,
                 w_proj=r(A + E, D) / (A + E) ** 0.5, b_proj=r(D) * 0.1)
        for i in (1, 2):
            x.update({"wg_%d" % i: r(2 * D, 2 * D) / (2 * D) ** 0.5, "bg_%d" % i: r(2 * D) * 0.1,
                      "wc_%d" % i: r(2 * D, D) / (2 * D) ** 0.5, "bc_%d" % i: r(D) * 0.1})
    return x


def _cut(t):
    return t[:, 1:]


def _fp32_bound(c, k, pure, emu32):
    p = _cut(pure[k])
    scale = float(p.abs().max())
    const = 2e-5 * math.sqrt(c.S)
    emu_rel = _dist(_cut(emu32[k]), p)[0] / scale if scale else 0.0
    return max(const, 4 * emu_rel) * scale, "const" if const >= 4 * emu_rel else "emu"


def loop_kink_margin(c, pure, emu32):
    """Per prenet layer: (smallest |pre-activation| of the reference, 100 x the fp32-rule bound of the buffer it is stored in)."""
    return {z: (float(_cut(pure[z]).abs().min()), 100 * _fp32_bound(c, buf, pure, emu32)[0]) for z, buf in (("z1", "p1"), ("z2", "xa"))}


@functools.lru_cache(maxsize=None)
def loop_inputs(c):
    """Walks the data seed until no prenet pre-activation of the pure reference lies inside the noise of a ReLU kink."""
    base = 7000 + 1000 * (c.family == "decode1") + 131 * c.N + 17 * c.S + c.Ti + c.kw + c.Dsp + c.A + (c.dtype == bf)
    fn = _loop_fn(c)
    for seed in range(base, base + 64):
        x = _draw_loop(c, seed)
        pure = fn(x)
        emu32 = fn(x, dtype=torch.float32, perm_seed=c.N + c.Ti)
        if all(got >= need for got, need in loop_kink_margin(c, pure, emu32).values()):
            return x, pure, emu32, seed
    raise AssertionError("no seed keeps the prenet pre-activations of %s away from zero" % loop_id(c))


@functools.lru_cache(maxsize=None)
def loop_references(c):
    x, pure, emu32, _ = loop_inputs(c)
    fn = _loop_fn(c)
    res = dict(pure=pure, exact=pure, bounds={}, source={}, figures={})
    if c.dtype == bf:
        res["exact"] = fn(x, bf16_storage=True)
        emu = fn(x, dtype=torch.float32, perm_seed=c.N + c.Ti, bf16_storage=True)
    for k in loop_names(c):
        p = _cut(pure[k])
        scale = float(p.abs().max())
        floor, res["source"][k] = _fp32_bound(c, k, pure, emu32)
        if c.dtype == f32:
            res["bounds"][k] = [("pure", floor, None)]
            continue
        e = _cut(res["exact"][k])
        emax, emean = _dist(_cut(emu[k]), e)
        dmax, dmean = _dist(e, p)
        flip = bf16_step(scale)
        res["figures"][k] = dict(scale=scale, emu_max=emax, emu_mean=emean, storage_max=dmax, storage_mean=dmean, one_flip=flip)
        res["bounds"][k] = [("exact", max(2 * emax, 2 * flip, floor), max(10 * emean, floor)),
                            ("pure", max(4 * dmax, floor), max(2 * dmean, floor))]
    return res


def _fill(p, **kw):
    from nspeech_amd import ops
    for k, v in kw.items():
        if v is None:
            continue
        if isinstance(v, tuple):
            v = ops.ptr(v[0], v[1])
        elif hasattr(v, "data_ptr"):
            v = ops.ptr(v)
        setattr(p, k, v)
    return p


def _size_t(name):
    from nspeech_amd import _lib as L
    fn = getattr(L.lib(), name)
    fn.restype = ctypes.c_size_t
    return fn


def run_loop(c, dev):
    """One decode case: returns the written histories cut to [N, S, .] on the CPU.  All layout assertions happen here."""
    from nspeech_amd import _lib as L
    from nspeech_amd import ops
    x, pure, _, _ = loop_inputs(c)
    N, S, Ti, Tia, A, E, D, Dsp, T = c.N, c.S, c.Ti, c.Tia, c.A, c.E, c.D, c.Dsp, c.dtype
    S1, padl = S + 1, 2
    Pi = padl + Ti + 3
    XA, HC = D2 + Dsp + A, A + E
    taco1 = c.family == "decode1"
    dv = lambda t, dtype=f32: t.to(dtype).contiguous().to(dev)
    z = lambda n, dtype=f32: torch.zeros(n, dtype=dtype, device=dev)
    keys = _rows(x["keys"], Pi, padl, BIG, f32, dev)
    values = _rows(x["values"], Pi, padl, BIG, T, dev)
    pv = _rows(x["pv"], Pi, padl, BIG, T, dev)
    f1 = dv(x["f1"].reshape(-1))
    lengths = x["lengths"].to(dev)
    xa0 = torch.zeros(N, S1, XA)
    if Dsp:
        xa0[:, :, D2:D2 + Dsp] = x["spk"][:, None, :]
    hc0 = torch.zeros(N, S1, HC)
    hc0[:, :, A:] = SENTINEL                                     # the context columns are not the entry's to write
    hist = dict(p1=z(N * S1 * D1, T), xa=dv(xa0.reshape(-1), T), hc=dv(hc0.reshape(-1), T), q=z(N * S1 * A), align=z(N * S1 * Tia))
    widths = dict(p1=D1, xa=XA, xc=XA, hc=HC, ca=A, ga=4 * A, ru=2 * A, cc=A, q=A, align=Tia, h2=D, y2=D)
    shared = dict(dtype=ops.dt(hist["hc"]), N=N, S=S, Ti=Ti, Pi=Pi, padl_i=padl, Tia=Tia, A=A, E=E, D1=D1, D2=D2, lengths=lengths,
                  keys=keys, pv=pv, f1=f1, Dsp=Dsp)
    dec = dict(wpf=dv(x["wpf"]), bpf=dv(x["bpf"]))
    if taco1:
        hist.update(xc=dv(xa0.reshape(-1), T), ru=z(N * S1 * 2 * A), cc=z(N * S1 * A), y2=z(N * S1 * D))
        align_t = z(N * S1 * Tia, T)
        weights = dict(w2=dv(x["W2"], T), wg=dv(x["Wg"], T), wc=dv(x["Wc"], T), wq=dv(x["Wq"], T), b2=dv(x["b2"]), bg=dv(x["bg"]),
                       bc=dv(x["bc"]), v=dv(x["v"]))
        dec.update(w_proj=dv(x["w_proj"]), b_proj=dv(x["b_proj"]))
        for i in (1, 2):
            dec.update({"%s_%d" % (k, i): dv(x["%s_%d" % (k, i)]) for k in ("wg", "bg", "wc", "bc")})
        q = L.struct("ns_taco1_decode_params")
        _fill(q.att, align_t=align_t, **shared, **weights, **{k: hist[k] for k in ("p1", "xa", "xc", "hc", "ru", "cc", "q", "align")})
        _fill(q, D=D, values=values, y2=hist["y2"], **dec)
        entry = "ns_taco1_decode"
        mr = L.lib().ns_taco1_decode_max_rows()
        if c.N == 17:
            assert mr + 1 == 17, "the two-launch case is sized for 16 rows per launch, this device takes %d" % mr
    else:
        hist.update(ca=z(N * S1 * A), ga=z(N * S1 * 4 * A, T), h2=z(N * S1 * D))
        align_t = None
        weights = dict(w2=dv(x["W2"], T), watt=dv(x["Watt"], T), wq=dv(x["Wq"], T), b2=dv(x["b2"]), batt=dv(x["batt"]),
                       wcl=dv(x["Wcl"]), v=dv(x["v"]))
        dec.update(w_l1=dv(x["w_l1"]), b_l1=dv(x["b_l1"]), w_l2=dv(x["w_l2"]), b_l2=dv(x["b_l2"]))
        q = L.struct("ns_taco2_decode_params")
        _fill(q.att, kw=c.kw, values=values, cell_clip=float(c.clip), **shared, **weights,
              **{k: hist[k] for k in ("p1", "xa", "hc", "ca", "ga", "q", "align")})
        _fill(q, D=D, h2=hist["h2"], **dec)
        entry = "ns_taco2_decode"
    lib = L.lib()
    if not getattr(lib, entry + "_supported")(ctypes.byref(q)):
        assert c.A == 256 and not taco1, "%s declines %s" % (entry, loop_id(c))
        pytest.skip("%s_supported says 0: the form's %d workgroups cannot be co-resident on this device" % (entry, 8 * N + 192))
    nbytes = (int(_size_t(entry + "_work_bytes")(ctypes.byref(q))) + 19) // 4 * 4
    work = torch.full((nbytes,), 255, dtype=torch.uint8, device=dev).view(f32)      # every word a NaN: the entry clears what it uses
    frozen = dict(keys=keys, values=values, pv=pv, f1=f1, lengths=lengths, **weights, **dec)
    before = {k: t.clone() for k, t in frozen.items()}
    first = None
    for _ in range(2):
        L.check(getattr(lib, entry)(ctypes.byref(q), ctypes.c_void_p(ops.ptr(work)), ctypes.c_void_p(ops.stream())), entry)
        torch.cuda.synchronize()
        assert _status(work) == 0, (entry, loop_id(c), _status(work))
        if first is None:
            first = {k: t.clone() for k, t in hist.items()}
    for k, t in hist.items():
        assert _same(t, first[k]), "%s: the second call on the same work differs from the first" % k
    for k, t in frozen.items():
        assert _same(t, before[k]), "%s changed" % k
    past = torch.arange(Tia)[None, :] >= x["lengths"][:, None].long()
    got = {}
    for k, t in hist.items():
        v = t.float().cpu().view(N, S1, widths[k])
        assert bool(torch.isfinite(v).all()), "%s is not finite" % k
        v0 = v[:, 0].clone()
        if k in ("xa", "xc") and Dsp:
            assert torch.equal(v[:, :, D2:D2 + Dsp], xa0[:, :, D2:D2 + Dsp].to(T).float()), "%s: the speaker columns changed" % k
            v0[:, D2:D2 + Dsp] = 0
        if k == "hc":
            assert bool((v[:, :, A:] == SENTINEL).all()), "hc: the context columns were written"
            v0, v = v0[:, :A], v[:, :, :A]
        assert float(v0.abs().max()) == 0.0, "%s: slot 0 is not zero" % k
        if k == "align":
            assert float(v[:, 1:][past[:, None, :].expand(N, S, Tia)].abs().max() if past.any() else 0) == 0.0, \
                "align is not 0 from the length on"
            v = v[:, :, :Ti]
        got[k] = _cut(v)
    if align_t is not None:
        at = align_t.float().cpu().view(N, S1, Tia)[:, 1:, :Ti]
        assert torch.equal(at, got["align"].to(T).float()), "align_t is not align in the storage type"
    return got


def check_loop(c, got, refs):
    bad = []
    for k in loop_names(c):
        for against, bmax, bmean in refs["bounds"][k]:
            emax, emean = _dist(got[k], _cut(refs[against][k]))
            ratios = [emax / bmax if bmax else float(emax > 0)] + ([emean / bmean] if bmean else [])
            print("%s %-6s vs %-5s: max %.3e / %.3e = %.2f%s  [%s]" % (
                loop_id(c), k, against, emax, bmax, ratios[0], "" if not bmean else "   mean %.3e / %.3e = %.2f" % (emean, bmean, ratios[1]),
                refs["source"].get(k, "")))
            _note(c.family, "%s-%s" % ("A%d" % c.A, "f32" if c.dtype == f32 else "bf16"), "%s/%s" % (k, against), max(ratios))
            if max(ratios) > 1.0:
                bad.append((k, against, ratios, refs["figures"].get(k)))
    assert not bad, bad


@pytest.mark.parametrize("c", [c for c in LOOP_CASES if c.family == "decode2"], ids=loop_id)
def test_taco2_decode_meets_the_contract(dev, c):
    check_loop(c, run_loop(c, dev), loop_references(c))


@pytest.mark.parametrize("c", [c for c in LOOP_CASES if c.family == "decode1"], ids=loop_id)
def test_taco1_decode_meets_the_contract(dev, c):
    check_loop(c, run_loop(c, dev), loop_references(c))


# ================================================================================================== ns_rows32
# cell 0/1, apk 0/1, passes 1/3, N, K, C (dense) or H (cell), opt: what the epilogue is given
Rows = namedtuple("Rows", "cell apk passes N K CH opt")
CELL_OPTS = [dict(dest="fp32"), dict(dest="rows", c_prev=False), dict(dest="all", forget_bias=0.0, clip=CLIP),
             dict(dest="fp32", zoneout=(0.1, 0.3)), dict(dest="rows", zoneout=(0.1, 0.3), clip=CLIP, forget_bias=0.0)]
DENSE_OPTS = [dict(dest="fp32", act=1, bias=True, add=True), dict(dest="rows", act=0, bias=False, add=False),
              dict(dest="all", act=2, bias=True, add=False), dict(dest="fp32", act=0, bias=False, add=True)]


def rows32_key(N, K, cell, apk, passes):
    """The instantiation ns_rows32 launches - a restatement of its dispatch (csrc/rows32.hip, ns_rows32: `three` / `two` and
    cpw at lines 277-278, NS_R32 at 286-291, the a_rows / cell_units branches at 292-301): (CELL, APK, THREE, TWO, RG)."""
    nkc = (K + 31) // 32
    cpw = (nkc + 7) // 8
    rg = 8 if not apk else (2 if cpw <= 2 else 4 if cpw <= 4 else 8)
    return (bool(cell), bool(apk), passes >= 3, N > 16, rg)


ALL_ROWS32_KEYS = sorted({(c, a, t, w, rg) for c in (False, True) for a in (False, True) for t in (False, True) for w in (False, True)
                          for rg in ((2, 4, 8) if a else (8,))})


def _rows_cases():
    out, i = [], 0
    for cell in (0, 1):
        for apk in (0, 1):
            for passes in (1, 3):
                for two in (0, 1):
                    for Ks in (((8, 40, 264), (520,), (1032, 2080)) if apk else ((8, 40, 264, 520, 1032, 2080),)):
                        K = Ks[i % len(Ks)]
                        N = ((17, 32) if two else (1, 16))[i % 2]
                        CH = (4, 20, 64)[i % 3] if cell else (16, 72)[i % 2]
                        opts = CELL_OPTS if cell else DENSE_OPTS
                        out.append(Rows(cell, apk, passes, N, K, CH, i % len(opts)))
                        i += 1
    # every K, N, C / H and option of the table at least once, on top of one case per instantiation
    extra = [Rows(0, 1, 3, 1, 8, 72, 0), Rows(0, 1, 3, 32, 40, 72, 1), Rows(0, 1, 1, 17, 264, 16, 2), Rows(0, 1, 3, 16, 2080, 72, 3),
             Rows(0, 0, 3, 17, 2080, 72, 0), Rows(0, 0, 1, 1, 8, 16, 2), Rows(1, 1, 3, 1, 8, 4, 1), Rows(1, 1, 3, 32, 40, 20, 2),
             Rows(1, 1, 3, 17, 264, 64, 3), Rows(1, 1, 1, 16, 2080, 20, 4), Rows(1, 0, 3, 32, 2080, 64, 4), Rows(1, 0, 3, 16, 520, 4, 0),
             Rows(1, 1, 3, 32, 1032, 64, 0), Rows(1, 0, 1, 17, 40, 20, 1)]
    return out + [e for e in extra if e not in out]


ROWS_CASES = _rows_cases()


def rows_id(c):
    return "%s-%s-x%d-N%d-K%d-%s%d-o%d" % ("cell" if c.cell else "dense", "apk" if c.apk else "f32", c.passes, c.N, c.K,
                                          "H" if c.cell else "C", c.CH, c.opt)


@functools.lru_cache(maxsize=None)
def rows_inputs(c):
    g = torch.Generator().manual_seed(c.N * 7919 + c.K * 31 + c.CH + 5 * c.cell + c.passes)
    r = lambda *shape: torch.randn(*shape, generator=g)
    C = 4 * c.CH if c.cell else c.CH
    o = (CELL_OPTS if c.cell else DENSE_OPTS)[c.opt]
    x = dict(a=r(c.N, c.K), w=r(c.K, C) * (1.5 if o.get("clip") else 0.7) / c.K ** 0.5)
    if c.cell:
        zc, zh = o.get("zoneout", (0.0, 0.0))
        x.update(bias=r(C) * 0.1, c_prev=r(c.N, c.CH) if o.get("c_prev", True) else None, h_prev=r(c.N, c.CH) * 0.5 if zc or zh else None,
                 forget_bias=o.get("forget_bias", 1.0), zoneout_cell=zc, zoneout_output=zh, cell_clip=o.get("clip", 0.0))
    else:
        x.update(bias=r(C) if o["bias"] else None, add=r(c.N, C) if o["add"] else None, act=o["act"])
    return x


def rows_reference(c):
    """(reference, emulation operands x, bounds): one pass is held against the bf16-rounded operands."""
    x = rows_inputs(c)
    product = "three" if c.passes == 3 else "one"
    if c.cell:
        ref = R.rows32_cell(x, product="exact" if c.passes == 3 else "one")
        xb = dict(x, a=AR.bf16(x["a"]), w=AR.bf16(x["w"])) if c.passes == 1 else x
        bz = R.preact_bound(xb, product)
        bh, bc = R.cell_bounds(bz, ref["c_prev"], ref["h_prev"])
        return x, ref, dict(h=bh, c=bc)
    ref = R.rows32_dense(x, product="exact" if c.passes == 3 else "one")
    xb = dict(x, a=AR.bf16(x["a"]), w=AR.bf16(x["w"])) if c.passes == 1 else x
    return x, ref, dict(y=R.dense_bound(R.preact_bound(xb, product), ref["z"], x["act"]))


def _per_element(tag, family, form, k, got, ref, bound):
    err = (got.double() - ref.double()).abs()
    ratio = float((err / bound).max())
    print("%s %-4s: max err %.3e, worst err / bound %.3f (bound there %.3e)" % (tag, k, float(err.max()), ratio,
                                                                               float(bound.flatten()[int((err / bound).argmax())])))
    _note(family, form, k, ratio)
    return ratio


@pytest.mark.parametrize("c", ROWS_CASES, ids=rows_id)
def test_rows32_meets_the_contract(dev, c):
    from nspeech_amd import _lib as L
    from nspeech_amd import ops
    x, ref, bounds = rows_reference(c)
    N, K, H = c.N, c.K, c.CH if c.cell else 0
    C = 4 * H if c.cell else c.CH
    Cout = H if c.cell else C
    o = (CELL_OPTS if c.cell else DENSE_OPTS)[c.opt]
    dv = lambda t: None if t is None else t.float().contiguous().to(dev)
    # ns_rows32_pack out of a wider matrix (ldw > C)
    ldw = C + 12
    wide_w = torch.full((K, ldw), SENTINEL)
    wide_w[:, :C] = x["w"]
    wdev = dv(wide_w)
    packed = torch.full((ops.rows32_packed_floats(K, C) + 8,), SENTINEL, device=dev)
    L.check(L.lib().ns_rows32_pack(ctypes.c_void_p(ops.ptr(wdev)), ctypes.c_int64(ldw), K, C, H, ctypes.c_void_p(ops.ptr(packed)),
                                   ctypes.c_void_p(ops.stream())), "ns_rows32_pack")
    torch.cuda.synchronize()
    assert bool((packed[-8:] == SENTINEL).all()), "ns_rows32_pack wrote past ns_rows32_packed_bytes"
    assert _same(packed[:-8].cpu(), R.pack_weights(x["w"], H)), "ns_rows32_pack: not the layout of the header"
    nkc32 = (K + 31) // 32 * 32
    a_sn = K + 8
    a_dev = _strided(x["a"], a_sn, dev)
    p = L.struct("ns_rows32_params")
    bias = dv(x.get("bias"))
    _fill(p, N=N, K=K, C=C, packed=packed, f32_passes=c.passes, bias=bias, cell_units=H)
    keep = [a_dev, bias]
    col, a_K = 32 * (1 + c.opt % 2), 0
    if c.apk:
        a_K = col + nkc32 + 32
    else:
        _fill(p, a=a_dev, a_sn=a_sn)
    out_sn = Cout + 2 * MARGIN
    outs = {k: torch.full((N * out_sn,), SENTINEL, device=dev) for k in ("out", "out2")}
    dst_K = (40 + Cout + 31) // 32 * 32 + 32
    dst_cols = dict(rows_out=40, rows_out2=8)
    if o["dest"] in ("fp32", "all"):
        _fill(p, out=(outs["out"], MARGIN), out_sn=out_sn, out2=(outs["out2"], MARGIN), out2_sn=out_sn)
    if c.cell:
        c_sn = H + 2 * MARGIN
        c_out = torch.full((N * c_sn,), SENTINEL, device=dev)
        cp = _wide(x["c_prev"], c_sn, dev) if x["c_prev"] is not None else None
        hp = _wide(x["h_prev"], c_sn, dev) if x["h_prev"] is not None else None
        _fill(p, c_prev=(cp, MARGIN) if cp is not None else None, c_sn=c_sn, c_out=(c_out, MARGIN), co_sn=c_sn,
              forget_bias=float(x["forget_bias"]), zoneout_cell=float(x["zoneout_cell"]), zoneout_output=float(x["zoneout_output"]),
              h_prev=(hp, MARGIN) if hp is not None else None, hp_sn=c_sn, cell_clip=float(x["cell_clip"]))
        keep += [cp, hp]
    else:
        add = _wide(x["add"], out_sn, dev) if x["add"] is not None else None
        _fill(p, add=(add, MARGIN) if add is not None else None, add_sn=out_sn, act=int(x["act"]))
        keep.append(add)
    results = []
    for garbage in ((False, True) if c.apk else (False,)):
        if c.apk:
            # the operand at a_rows_col > 0 of a wider buffer, written by ns_rows32_pack_rows; the second run has +-3e38 (finite)
            # in every other column - the operand's own chunk columns past K included - and in the rows from N on
            host = torch.zeros(32, a_K)
            if garbage:
                host = HUGE * (1 - 2 * ((torch.arange(32)[:, None] + torch.arange(a_K)[None, :]) % 2).float())
            arows = R.pack_rows(host, a_K).to(dev)
            expect = host.clone()
            expect[:N, col:col + K] = x["a"]
            L.check(L.lib().ns_rows32_pack_rows(ctypes.c_void_p(ops.ptr(a_dev)), ctypes.c_int64(a_sn), N, K, ctypes.c_void_p(ops.ptr(arows)),
                                                a_K, col, ctypes.c_void_p(ops.stream())), "ns_rows32_pack_rows")
            torch.cuda.synchronize()
            assert _same(arows.cpu(), R.pack_rows(expect, a_K)), "ns_rows32_pack_rows: layout, or columns / rows outside the operand changed"
            _fill(p, a_rows=arows, a_rows_K=a_K, a_rows_col=col)
            keep.append(arows)
        dst = {k: R.pack_rows(torch.full((32, dst_K), SENTINEL), dst_K).to(dev) for k in dst_cols}
        if o["dest"] in ("rows", "all"):
            _fill(p, rows_out=dst["rows_out"], rows_out_K=dst_K, rows_out_col=dst_cols["rows_out"], rows_out2=dst["rows_out2"],
                  rows_out2_K=dst_K, rows_out2_col=dst_cols["rows_out2"])
        for t in list(outs.values()) + ([c_out] if c.cell else []):
            t.fill_(SENTINEL)
        frozen = [t.clone() for t in keep if t is not None] + [packed.clone()]
        L.call("ns_rows32", p, ops.stream())
        torch.cuda.synchronize()
        for t, b in zip([t for t in keep if t is not None] + [packed], frozen):
            assert _same(t, b), "an input changed"
        got = {}
        if o["dest"] in ("fp32", "all"):
            got["fp32"] = _block_of(outs["out"], N, out_sn, Cout, "out").clone()
            assert torch.equal(_block_of(outs["out2"], N, out_sn, Cout, "out2"), got["fp32"]), "out2 != out"
        else:
            assert all(bool((t == SENTINEL).all()) for t in outs.values()), "out / out2 written without being asked for"
        if o["dest"] in ("rows", "all"):
            for k, c0 in dst_cols.items():
                full = torch.from_numpy(R.unpack_rows(dst[k], dst_K, 32))
                other = torch.ones(32, dst_K, dtype=torch.bool)
                other[:N, c0:c0 + Cout] = False
                # SENTINEL = 7 is a bf16: its (hi, lo) pair reads back exactly
                assert bool((full[other] == SENTINEL).all()), "%s: columns or rows outside the destination changed" % k
                got[k] = full[:N, c0:c0 + Cout].clone()
            assert torch.equal(got["rows_out"], got["rows_out2"]), "rows_out2 != rows_out"
            if "fp32" in got:
                hi, lo = R.split_hi_lo(got["fp32"])
                assert torch.equal(got["rows_out"], hi.double() + lo.double()), "rows_out is not the (hi, lo) split of out"
        else:
            assert all(_same(t.cpu(), R.pack_rows(torch.full((32, dst_K), SENTINEL), dst_K)) for t in dst.values())
        if c.cell:
            got["c"] = _block_of(c_out, N, c_sn, H, "c_out").clone()
        results.append(got)
    if len(results) == 2:
        for k in results[0]:
            assert torch.equal(results[0][k], results[1][k]), "%s moved with finite garbage outside the packed operand" % k
    got = results[-1]
    form = "%s-%s-x%d" % ("cell" if c.cell else "dense", "apk" if c.apk else "f32", c.passes)
    main, rk = ("h", "h") if c.cell else ("y", "y")
    worst = []
    for dest in ("fp32", "rows_out"):
        if dest in got:
            b = bounds[main] + (R.SPLIT_EPS * ref[rk].abs() if dest == "rows_out" else 0)
            worst.append(_per_element(rows_id(c), "rows32", form, main + ("/rows" if dest == "rows_out" else ""), got[dest], ref[rk], b))
    if c.cell:
        worst.append(_per_element(rows_id(c), "rows32", form, "c", got["c"], ref["c"], bounds["c"]))
    assert max(worst) <= 1.0, worst


def _strided(x, ld, dev):
    """x [N, K] as the first K columns of [N, ld] rows (16-byte aligned rows; the tail holds a sentinel)."""
    full = torch.full((x.shape[0], ld), SENTINEL)
    full[:, :x.shape[1]] = x
    return full.reshape(-1).to(dev)


def test_rows32_table_reaches_every_instantiation():
    reached = {rows32_key(c.N, c.K, c.cell, c.apk, c.passes) for c in ROWS_CASES}
    assert sorted(reached) == ALL_ROWS32_KEYS, sorted(set(ALL_ROWS32_KEYS) - reached)


# ================================================================================================ ns_lstm_step
# form: f0, f1, f1s, f2, f2s, f3, f3s (s = pre-split wT_hi / wT_lo), bf16
Step = namedtuple("Step", "form N H K opt")
STEP_OPTS = [dict(xg=True, bias=True), dict(xg=False, bias=True, c_prev=False, out2=True), dict(xg=True, bias=False, zoneout=(0.1, 0.3)),
             dict(xg=False, bias=False, clip=CLIP, out2=True), dict(xg=True, bias=True, zoneout=(0.1, 0.3), clip=CLIP, c_prev=True)]
STEP_FORMS = ("f0", "f1", "f1s", "f2", "f2s", "f3", "f3s", "bf16")


def _step_cases():
    out, i = [], 0
    for form in STEP_FORMS:
        # H < 256: the big tiling; H = 256 at 16 tiles: the small one; 16 x ceil(257 / 32) = 144 > 128 tiles: the big one again
        for N, H in ((5, 16), (5, 256), (257, 256)):
            out.append(Step(form, N, H, (40, 392)[i % 2], i % len(STEP_OPTS)))
            i += 1
    return out


STEP_CASES = _step_cases()


def step_tiling(N, H):
    """"half" or "big": the rule of lstm_step_launch2 (csrc/lstm.hip)."""
    big = (H + 15) // 16 * ((N + 31) // 32)
    return "half" if H >= 256 and big <= 128 else "big"


def step_id(c):
    return "%s-N%d-H%d-K%d-o%d" % c


@functools.lru_cache(maxsize=None)
def step_inputs(c):
    g = torch.Generator().manual_seed(c.N * 131 + c.H * 7 + c.K + STEP_FORMS.index(c.form))
    r = lambda *shape: torch.randn(*shape, generator=g)
    o = STEP_OPTS[c.opt]
    rnd = (lambda t: AR.bf16(t)) if c.form == "bf16" else (lambda t: t)
    zc, zh = o.get("zoneout", (0.0, 0.0))
    return dict(a=rnd(r(c.N, c.K)), wT=rnd(r(4 * c.H, c.K) * (1.5 if o.get("clip") else 0.7) / c.K ** 0.5),
                xg=r(c.N, 4 * c.H) * 0.5 if o["xg"] else None, bias=r(4 * c.H) * 0.1 if o["bias"] else None,
                c_prev=r(c.N, c.H) if o.get("c_prev", True) else None, h_prev=rnd(r(c.N, c.H) * 0.5) if zc or zh else None,
                forget_bias=1.0 if c.opt % 2 == 0 else 0.5, zoneout_cell=zc, zoneout_output=zh, cell_clip=o.get("clip", 0.0))


def step_reference(c):
    x = step_inputs(c)
    passes = dict(f0=0, f1=1, f1s=1, f2=2, f2s=2, f3=3, f3s=3, bf16=0)[c.form]
    product = {0: "exact", 1: "one", 2: "two", 3: "three"}[passes]
    # one pass against the bf16-rounded operands; two and three passes against the pure reference
    ref = R.lstm_step(x, product="one" if passes == 1 else "exact")
    xb = dict(x, a=AR.bf16(x["a"]), wT=AR.bf16(x["wT"])) if passes == 1 else x
    bh, bc = R.cell_bounds(R.preact_bound(xb, product, "wT"), ref["c_prev"], ref["h_prev"])
    if c.form == "bf16":
        bh = bh + 2.0 ** -8 * (ref["h"].abs() + bh)
    return x, ref, dict(h=bh, c=bc), passes


@pytest.mark.parametrize("c", STEP_CASES, ids=step_id)
def test_lstm_step_meets_the_contract(dev, c):
    from nspeech_amd import _lib as L
    from nspeech_amd import ops
    x, ref, bounds, passes = step_reference(c)
    N, H, K = c.N, c.H, c.K
    T = bf if c.form == "bf16" else f32
    o = STEP_OPTS[c.opt]
    a_sn = K + 8
    a = _strided(x["a"], a_sn, dev).to(T)
    wT = x["wT"].contiguous().to(dev).to(T)
    sn, g_sn = H + 2 * MARGIN, 4 * H + 2 * MARGIN
    h_out, h_out2 = (torch.full((N * sn,), SENTINEL, dtype=T, device=dev) for _ in range(2))
    c_out = torch.full((N * sn,), SENTINEL, device=dev)
    xg = _wide(x["xg"], g_sn, dev) if x["xg"] is not None else None
    cp = _wide(x["c_prev"], sn, dev) if x["c_prev"] is not None else None
    hp = _wide(x["h_prev"], sn, dev, T) if x["h_prev"] is not None else None
    bias = x["bias"].to(dev) if x["bias"] is not None else None
    p = L.struct("ns_lstm_step_params")
    _fill(p, dtype=ops.dt(a), N=N, H=H, K=K, a=a, a_sn=a_sn, wT=wT, xg=(xg, MARGIN) if xg is not None else None, xg_sn=g_sn, bias=bias,
          c_prev=(cp, MARGIN) if cp is not None else None, c_sn=sn, h_out=(h_out, MARGIN), h_sn=sn,
          h_out2=(h_out2, MARGIN) if o.get("out2") else None, h2_sn=sn, c_out=(c_out, MARGIN), co_sn=sn,
          forget_bias=float(x["forget_bias"]), f32_passes=passes, zoneout_cell=float(x["zoneout_cell"]),
          zoneout_output=float(x["zoneout_output"]), h_prev=(hp, MARGIN) if hp is not None else None, hp_sn=sn,
          cell_clip=float(x["cell_clip"]))
    keep = [t for t in (a, wT, xg, cp, hp, bias) if t is not None]
    if c.form.endswith("s"):
        hi, lo = R.split_hi_lo(x["wT"])
        hi, lo = hi.contiguous().to(dev), lo.contiguous().to(dev)
        _fill(p, wT_hi=hi, wT_lo=lo)
        keep += [hi, lo]
    frozen = [t.clone() for t in keep]
    L.call("ns_lstm_step", p, ops.stream())
    torch.cuda.synchronize()
    for t, b in zip(keep, frozen):
        assert _same(t, b), "an input changed"
    h = _block_of(h_out, N, sn, H, "h_out")
    if o.get("out2"):
        assert torch.equal(_block_of(h_out2, N, sn, H, "h_out2"), h), "h_out2 != h_out"
    else:
        assert bool((h_out2.float() == SENTINEL).all()), "h_out2 written without being asked for"
    form = "%s-%s" % (c.form, step_tiling(N, H))
    worst = [_per_element(step_id(c), "step", form, "h", h, ref["h"], bounds["h"]),
             _per_element(step_id(c), "step", form, "c", _block_of(c_out, N, sn, H, "c_out"), ref["c"], bounds["c"])]
    assert max(worst) <= 1.0, worst


def test_step_table_reaches_both_tilings_of_every_form():
    assert {(c.form, step_tiling(c.N, c.H)) for c in STEP_CASES} == {(f, t) for f in STEP_FORMS for t in ("big", "half")}
    assert step_tiling(256, 256) == "half" and step_tiling(257, 256) == "big"


# ======================================================================================== ns_attention_step, ctx_rows
CTX_CASES = [(o, col) for o in ONE_CASES if o.N <= 32 for col in (0, 32)]


@pytest.mark.parametrize("o,col", CTX_CASES, ids=lambda v: one_id(v) if not isinstance(v, int) else "col%d" % v)
def test_attention_step_writes_the_context_as_packed_rows(dev, o, col):
    from nspeech_amd import ops
    x = one_inputs(o)
    N, Ti, Tia, A, E, T = o.N, o.Ti, o.Tia, o.A, o.E, o.dtype
    padl, Pi = 2, 2 + Ti + 3
    a = (x["keys"], x["values"], x["q"], x["aprev"], x["Wcl"], x["v"], x["lengths"])
    ref, emu = AR.attention_step(*a), AR.attention_step(*a, dtype=torch.float32)
    keys_t = torch.zeros(N, A, Tia)
    keys_t[:, :, :Ti] = x["keys"].transpose(1, 2)
    keys_t = keys_t.reshape(-1).to(dev)
    values = _rows(x["values"], Pi, padl, BIG, T, dev)
    ap = torch.zeros(N, Tia)
    ap[:, :Ti] = x["aprev"]
    q, aprev = x["q"].contiguous().to(dev), ap.to(dev)
    aout, ctx = torch.zeros(N * Tia, device=dev), torch.zeros(N * E, dtype=T, device=dev)
    rows_K = col + E + 40
    g = torch.Generator().manual_seed(o.N + o.Ti + col)
    host = torch.randn(32, (rows_K + 31) // 32 * 32, generator=g)
    rows = R.pack_rows(host, rows_K).to(dev)
    ops.attention_step(values, N, Ti, Pi, padl, Tia, A, E, o.kw, x["lengths"].to(dev), keys_t, values, q, A, aprev, aout, Tia, ctx, E,
                       None, 0, x["Wcl"].contiguous().to(dev), x["v"].to(dev), torch.zeros(N * Tia, device=dev),
                       ctx_rows=(rows, rows_K, col))
    torch.cuda.synchronize()
    hi, lo = R.unpack_rows(rows, rows_K, 32, planes=True)
    hi0, lo0 = R.unpack_rows(R.pack_rows(host, rows_K), rows_K, 32, planes=True)
    other = torch.ones(32, hi.shape[1], dtype=torch.bool)
    other[:N, col:col + E] = False
    assert bool((torch.from_numpy(hi == hi0) & torch.from_numpy(lo == lo0))[other].all()), "columns or rows outside the context changed"
    got = dict(ctx_rows=torch.from_numpy(hi + lo)[:N, col:col + E])
    refs = _one_bounds(ref, emu, ["ctx"], ["ctx"])
    (_, bmax, _), = refs["bounds"]["ctx"]
    # what the kernel holds in fp32 is within the fp32 rule of the reference; the (hi, lo) pair keeps it to 2^-16
    bound = bmax + R.SPLIT_EPS * float(ref["ctx"].abs().max())
    emax = _dist(got["ctx_rows"], ref["ctx"])[0]
    print("%s col %d ctx_rows: max %.3e / %.3e = %.2f" % (one_id(o), col, emax, bound, emax / bound))
    _note("ctxrows", "f32" if T == f32 else "bf16", "ctx_rows", emax / bound)
    if T == f32:
        h2, l2 = R.split_hi_lo(ctx.cpu().view(N, E))
        assert torch.equal(got["ctx_rows"], h2.double() + l2.double()), "ctx_rows is not the (hi, lo) split of ctx_out"
    assert emax <= bound


def test_attention_step_refuses_ctx_rows_above_32_rows(dev):
    from nspeech_amd import _lib as L
    from nspeech_amd import ops
    one = torch.zeros(64, device=dev)
    p = L.struct("ns_attention_step_params")
    _fill(p, dtype=0, N=33, Ti=8, Pi=8, padl_i=0, Tia=8, A=8, E=8, kw=7, lengths=one, keys_t=one, values=one, q=one, q_sn=8, aprev=one,
          aout=one, al_sn=8, ctx_out=one, ctx_sn=8, wcl=one, v=one, e_raw=one, ctx_rows=one, ctx_rows_K=64, ctx_rows_col=0)
    assert L.lib().ns_attention_step(ctypes.byref(p), ctypes.c_void_p(ops.stream())) != 0


# ================================================================================================ the key transposes
@pytest.mark.parametrize("A", [24, 40])
@pytest.mark.parametrize("Ti", [1, 31, 33])
def test_keys_transposes_are_exact(dev, A, Ti):
    from nspeech_amd import ops
    N, padl = 2, 2
    Tia, Pi = (Ti + 7) // 8 * 8, padl + Ti + 3
    g = torch.Generator().manual_seed(A + Ti)
    keys = torch.full((N, Pi, A), BIG)
    keys[:, padl:padl + Ti] = torch.randn(N, Ti, A, generator=g)
    kd = keys.reshape(-1).to(dev)
    kt = torch.full((N * A * Tia + 8,), SENTINEL, device=dev)
    ops.keys_transpose(kd, kt, N, Ti, Tia, Pi, padl, A)
    torch.cuda.synchronize()
    want = R.keys_transpose(dict(keys=keys, Ti=Ti, Tia=Tia, padl=padl)).float()
    assert _same(kd.cpu(), keys.reshape(-1)), "keys changed"
    assert bool((kt[-8:] == SENTINEL).all()), "written past keys_t"
    assert _same(kt[:-8].cpu(), want.reshape(-1)), "the transpose is not bit-exact (columns [T_in, Tia) are 0)"
    # back: keys += keys_t, one fp32 add per element; keys_t's columns from T_in on hold 1e30 and are not read
    pre = torch.full((N, Pi, A), 0.375)
    pre[:, padl:padl + Ti] = torch.randn(N, Ti, A, generator=g)
    src = torch.full((N, A, Tia), BIG)
    src[:, :, :Ti] = torch.randn(N, A, Ti, generator=g)
    pd, sd = pre.reshape(-1).to(dev), src.reshape(-1).to(dev)
    ops.keys_transpose_add(pd, sd, N, Ti, Tia, Pi, padl, A)
    torch.cuda.synchronize()
    want = R.keys_transpose_add(dict(keys=pre, keys_t=src, Ti=Ti, padl=padl), dtype=torch.float32)
    assert _same(sd.cpu(), src.reshape(-1)), "keys_t changed"
    assert _same(pd.cpu(), want.reshape(-1)), "keys += keys_t is not one fp32 add per element with the pad rows unchanged"


def test_worst_ratios_are_reported():
    """Prints, per family, form and buffer, the worst error / bound of the cases above."""
    for key in sorted(WORST):
        print("worst %-8s %-16s %-14s %.2f" % (key + (WORST[key],)))
