"""Every epilogue option of ns_gemm on every kernel form behind its dispatch, against the float64 contract of
tests/gemm_ref.py.

Two tables: FORMS (a kernel form and the smallest shape that selects it - the kernel's name is asserted after every
call, so a later dispatch change cannot drop a form from coverage quietly) and the option sets E0 .. E6.  Every buffer
is larger than the region the call may touch and is reached through a non-zero offset and a leading dimension above N;
what lies outside the region of C must come back bit for bit.

Shapes that differ from the first draft of the table, found by reading gemm_dispatch: the k-slow-A (a_mode 1) forms of
the scalar-epilogue 128-tile kernel run at M = 136 (the 16-byte path needs M % 8 == 0; at M = 130 the generic kernel
runs); the 128-row vector forms of the fp32 kernel with k-contiguous A run at 2176 x 2048 x 64 like their bf16
counterparts (at <= 256 tiles a k-contiguous A with a vector epilogue takes the 64-row form).

Error bound, per element, nothing excluded (u = 2^-24, mag from gemm_ref):
  accumulation   exact products (bf16 operands, fp32 at f32_passes 0): 2 (K + 4) u mag - the fp32 summation bound of
                 any order, doubled for the matrix core's internal rounding;
                 split-bf16 forms: the bounds of test_gemm_fp32_split_bf16 - 3e-5 max|A| max|B| sqrt(K) (three passes,
                 three segments), 2e-2 ... (one pass), three passes + 2^-9 (|A|.|B|) (two segments: B rounded to bf16)
  activation     all four are 1-Lipschitz; tanh and sigmoid add 1e-6 (ten times what common.h documents)
  store          2^-23 |ref| (fp32 C), 2^-8 |ref| (bf16 C), ref being the value BEFORE the store's rounding
Masked and gated-off elements are exact.  Statistics are held against float64 sums of the C read back from the device,
to 2 (M + 4) u sum|terms| per column.
"""
import math
from types import SimpleNamespace as NS

import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu

bf, f32 = torch.bfloat16, torch.float32
U = 2.0 ** -24
MASK = (30, 2, 27, 2)          # does not divide 64
MASK_SHORT = (7, 1, 6, 3)      # for the forms of <= 25 rows, where MASK keeps every row
SENTINEL = -1234.5


# ------------------------------------------------------------------ kernel forms
def _form(fid, kernel, dtype, a_mode, b_mode, M, N, K, vec, kind="exact", passes=0, caps=()):
    return NS(id=fid, kernel=kernel, dtype=dtype, a_mode=a_mode, b_mode=b_mode, M=M, N=N, K=K, vec=vec, kind=kind,
              passes=passes, caps=frozenset(caps))


def _forms():
    F = []
    # caps: stats (takes col_sum), split (takes split_k > 1 on this very kernel), batch
    for dt, nm in ((bf, "bf16"), (f32, "f32")):
        F.append(_form("generic_" + nm, "gemm_generic_kernel", dt, 0, 0, 70, 67, 45, False, caps=("stats", "split", "batch")))
    for M, K in ((1, 104), (17, 104), (32, 104), (17, 1064)):
        F.append(_form("skinny1_M%d_K%d" % (M, K), "gemm_skinny_kernel<1>", bf, 0, 0, M, 72, K, False))
    F.append(_form("skinny2", "gemm_skinny_kernel<2>", bf, 0, 0, 5, 4104, 64, False))
    for b in (0, 1):
        F.append(_form("mfma_half_0%d" % b, "gemm_mfma_kernel<0, %d, true, 64, 64>" % b, bf, 0, b, 130, 136, 72, True,
                       caps=("stats",)))
    F.append(_form("mfma_vec_10", "gemm_mfma_kernel<1, 0, true, 64, 128>", bf, 1, 0, 136, 140, 104, True, caps=("stats",)))
    F.append(_form("mfma_vec_11", "gemm_mfma_kernel<1, 1, true, 64, 128>", bf, 1, 1, 136, 136, 100, True, caps=("stats",)))
    for b in (0, 1):
        F.append(_form("mfma_vec_0%d" % b, "gemm_mfma_kernel<0, %d, true, 64, 128>" % b, bf, 0, b, 2176, 2048, 64, True,
                       caps=("stats",)))
    for a in (0, 1):
        for b in (0, 1):
            F.append(_form("mfma_scalar_%d%d" % (a, b), "gemm_mfma_kernel<%d, %d, false, 64, 128>" % (a, b), bf, a, b,
                           130 if a == 0 else 136, 136, 72, False, caps=("stats", "split", "batch")))
    F.append(_form("mfma_scalar_00_N67", "gemm_mfma_kernel<0, 0, false, 64, 128>", bf, 0, 0, 130, 67, 72, False,
                   caps=("stats", "split", "batch")))
    F.append(_form("mfma_bk32", "gemm_mfma_kernel<1, 1, false, 32, 128>", bf, 1, 1, 640, 640, 808, False, caps=("bk32",)))
    F.append(_form("x256_1", "gemm_x256_kernel<1>", bf, 0, 0, 1030, 6272, 192, True, caps=("stats",)))
    F.append(_form("x256_3", "gemm_x256_kernel<3>", bf, 0, 0, 1024, 6144, 128, True, kind="x3", passes=3, caps=("stats", "presplit")))
    F.append(_form("x256_2", "gemm_x256_kernel<2>", bf, 0, 0, 1024, 6144, 128, True, kind="x2", passes=2, caps=("stats", "presplit")))
    for P in (1, 3):
        kind = "p%d" % P
        F.append(_form("skinny_f32_%d_8" % P, "gemm_skinny_f32_kernel<%d, 1, 8>" % P, f32, 0, 0, 20, 72, 104, False, kind, P))
        F.append(_form("skinny_f32_%d_16" % P, "gemm_skinny_f32_kernel<%d, 2, 16>" % P, f32, 0, 0, 20, 1040, 104, False, kind, P))
        for a in (0, 1):
            for b in (0, 1):
                F.append(_form("f32_p%d_scalar_%d%d" % (P, a, b), "gemm_mfma_f32_kernel<%d, %d, %d, false, 128>" % (a, b, P),
                               f32, a, b, 136, 136, 100, False, kind, P, caps=("stats", "split", "batch")))
        for b in (0, 1):
            F.append(_form("f32_p%d_vec_1%d" % (P, b), "gemm_mfma_f32_kernel<1, %d, %d, true, 128>" % (b, P), f32, 1, b,
                           136, 136, 100, True, kind, P, caps=("stats",)))
            F.append(_form("f32_p%d_half_0%d" % (P, b), "gemm_mfma_f32_kernel<0, %d, %d, true, 64>" % (b, P), f32, 0, b,
                           130, 136, 100, True, kind, P, caps=("stats",)))
            F.append(_form("f32_p%d_vec_0%d" % (P, b), "gemm_mfma_f32_kernel<0, %d, %d, true, 128>" % (b, P), f32, 0, b,
                           2176, 2048, 64, True, kind, P, caps=("stats",)))
    return F


FORMS = _forms()
K_TILE = {"gemm_generic_kernel": 16, "gemm_mfma_kernel": 64, "gemm_mfma_f32_kernel": 32}     # K per tile of the split-K forms


# ------------------------------------------------------------------ option sets
def _opt(oid, **kw):
    d = dict(id=oid, act=0, alpha=1.0, bias=False, addend=None, c_dtype=f32, mask=None, stats=False, gate=False,
             accumulate=0, stat_z=None, split_k=1, det=False, batch=1)
    d.update(kw)
    return NS(**d)


E_PLAIN = [_opt("E0")]
E_PLAIN += [_opt("E1_" + n, act=a, alpha=-0.5, bias=True, addend=f32) for n, a in
            (("tanh", R.ACT_TANH), ("sigmoid", R.ACT_SIGMOID), ("softsign", R.ACT_SOFTSIGN), ("relu", R.ACT_RELU))]
E_PLAIN += [_opt("E2", addend=bf, c_dtype=bf, mask=MASK, stats=True)]
E2_SHORT = _opt("E2_short_mask", addend=bf, c_dtype=bf, mask=MASK_SHORT, stats=True)
E_PLAIN += [_opt("E3", gate=True, accumulate=1, alpha=1.5)]
E_STATZ = [_opt("E4_z%s_acc%d" % ("bf16" if z == bf else "f32", acc), stat_z=z, stats=True, mask=MASK, accumulate=acc)
           for z in (f32, bf) for acc in (0, 1)]


def _split_opt(split_k, det):
    return _opt("E5_k%d_%s" % (split_k, "fixed" if det else "atomic"), split_k=split_k, det=det, accumulate=2, alpha=1.5,
                bias=True, addend=f32, gate=True, mask=MASK)


E_BATCH = _opt("E6", batch=3, split_k=2, accumulate=2)


def _cases():
    out = []
    for f in FORMS:
        if "bk32" in f.caps:        # the form IS a split-K launch of >= 600 workgroups: 25 tiles x 24 slices
            opts = [_split_opt(24, False), _split_opt(24, True)]
        else:
            opts = list(E_PLAIN)
            if bool(R.valid_rows(f.M, MASK).all()):
                opts.append(E2_SHORT)
            if "stats" in f.caps:
                opts += E_STATZ
            if "split" in f.caps:
                nk = -(-f.K // K_TILE[f.kernel.split("<")[0]])
                for s in sorted({2, 3, nk + 1}):            # nk + 1: the last slices are empty
                    opts += [_split_opt(s, False), _split_opt(s, True)]
            if "batch" in f.caps:
                opts.append(E_BATCH)
        out += [pytest.param(f, o, id="%s-%s" % (f.id, o.id)) for o in opts]
    return out


# ------------------------------------------------------------------ data
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _uniform(n, seed):
    return torch.rand(n, generator=_gen(seed)) * 2.0 - 1.0


def _o13(n, seed):
    """magnitudes 1 .. 3 with random signs: an operand read at a wrong index moves the result by O(1)"""
    g = _gen(seed)
    return (1.0 + 2.0 * torch.rand(n, generator=g)) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)


def _gate(n, seed, dtype):
    """about half the entries <= 0, exact +0.0 and -0.0 among them"""
    g = _gen(seed)
    x = torch.randn(n, generator=g)
    r = torch.rand(n, generator=g)
    x = torch.where(r < 0.05, torch.zeros(()), x)
    x = torch.where((r >= 0.05) & (r < 0.10), -torch.zeros(()), x)
    return x.to(dtype)


_OPERANDS = {}


def _operands(dev, f, batch):
    """A and B of a form (and their low parts), made once, with the float64 products of the reference beside them"""
    key = (f.id, batch)
    if key in _OPERANDS:
        return _OPERANDS[key]
    seed = 1000 * (FORMS.index(f) + 1) + batch
    aligned = f.kernel != "gemm_generic_kernel"
    pad, off = (8, 8) if aligned else (3, 3)
    o = NS(cache={})
    o.lda = (f.K if f.a_mode == 0 else f.M) + pad
    o.ldb = (f.K if f.b_mode == 0 else f.N) + pad
    o.a_off, o.b_off = off, 2 * off
    a_item = (f.M if f.a_mode == 0 else f.K) * o.lda
    b_item = (f.N if f.b_mode == 0 else f.K) * o.ldb
    o.sa, o.sb = (a_item + 16, b_item + 24) if batch > 1 else (0, 0)
    a32 = _uniform(o.a_off + a_item + (batch - 1) * o.sa + 8, seed + 1)
    b32 = _uniform(o.b_off + b_item + (batch - 1) * o.sb + 8, seed + 2)
    o.A, o.B = a32.to(f.dtype), b32.to(f.dtype)
    o.A_lo = o.B_lo = None
    if "presplit" in f.caps:          # fp32 values as bf16 hi + lo pairs, as test_gemm_256_tile_kernel splits them
        o.A_lo, o.B_lo = (a32 - o.A.float()).to(bf), (b32 - o.B.float()).to(bf)
    o.dA, o.dB = o.A.to(dev), o.B.to(dev)
    o.dA_lo = None if o.A_lo is None else o.A_lo.to(dev)
    o.dB_lo = None if o.B_lo is None else o.B_lo.to(dev)
    o.maxA = o.maxB = 0.0
    for z in range(batch):
        a = R.operand_a(o.A, f.M, f.K, o.lda, f.a_mode, o.a_off + z * o.sa)
        b = R.operand_b(o.B, f.K, f.N, o.ldb, f.b_mode, o.b_off + z * o.sb)
        if o.A_lo is not None:
            a = a + R.operand_a(o.A_lo, f.M, f.K, o.lda, f.a_mode, o.a_off)
            b = b + R.operand_b(o.B_lo, f.K, f.N, o.ldb, f.b_mode, o.b_off)
        o.maxA, o.maxB = max(o.maxA, a.abs().max().item()), max(o.maxB, b.abs().max().item())
    _OPERANDS[key] = o
    return o


def _bound(f, o, ref, opt):
    if f.kind == "exact":
        acc = 2.0 * (f.K + 4) * U * ref.mag
    else:
        split3 = 3e-5 * o.maxA * o.maxB * math.sqrt(f.K)
        if f.kind in ("p3", "x3"):
            acc = torch.full_like(ref.mag, split3)
        elif f.kind == "p1":
            acc = torch.full_like(ref.mag, 2e-2 * o.maxA * o.maxB * math.sqrt(f.K))
        else:
            acc = split3 + 2.0 ** -9 * ref.absprod
    act = 1e-6 if opt.act in (R.ACT_TANH, R.ACT_SIGMOID) else 0.0
    store = (2.0 ** -8 if opt.c_dtype == bf else 2.0 ** -23) * ref.exact.abs()
    return acc + act + store


def _bits(t):
    return t.view(torch.int16 if t.dtype == bf else torch.int32)


def _run_case(dev, f, opt, repeats=1):
    """Runs the call (`repeats` times from the same prior C), checks every element of the last result and returns
    (worst err / bound, worst statistics err / tolerance, the C buffers of all runs)."""
    from nspeech_amd import ops, profiling
    M, N, K = f.M, f.N, f.K
    o = _operands(dev, f, opt.batch)
    seed = 1000 * (FORMS.index(f) + 1) + 17 * len(opt.id) + sum(map(ord, opt.id))
    v = 4 if f.vec else 1                       # offsets of the vector forms keep 16-byte alignment; the others are odd
    pad = 8 if f.vec else 3
    ldc, c_off = N + pad, (2 * (N + pad) + 4 if f.vec else 1)
    sc = M * ldc + 24 if opt.batch > 1 else 0
    kw = dict(a_mode=f.a_mode, b_mode=f.b_mode, a_off=o.a_off, b_off=o.b_off, c_off=c_off, act=opt.act, alpha=opt.alpha,
              accumulate=opt.accumulate, split_k=opt.split_k, f32_passes=f.passes)
    dkw = {}                                    # the device tensors of the same arguments
    if opt.batch > 1:
        kw.update(batch=opt.batch, batch_strides=(o.sa, o.sb, sc))
    prior = torch.full((c_off + M * ldc + (opt.batch - 1) * sc + 16,), SENTINEL).to(opt.c_dtype)
    region = torch.cat([R._mn(M, N, ldc, c_off + z * sc).reshape(-1) for z in range(opt.batch)])
    prior[region] = (_o13(region.numel(), seed + 1) if opt.accumulate else torch.full((region.numel(),), float("nan"))).to(opt.c_dtype)

    def operand(name, values, off_name=None, off=0, ld_name=None, ld=0):
        kw[name], dkw[name] = values, values.to(dev)
        if off_name:
            kw[off_name] = off
        if ld_name:
            kw[ld_name] = ld
    if opt.bias:
        operand("bias", _o13(N + 3 * v, seed + 2), "bias_off", v)
    if opt.addend is not None:
        ld = N + 4 * v
        operand("addend", _o13(2 * v + M * ld + 8, seed + 3).to(opt.addend), "addend_off", 2 * v, "ld_add", ld)
    if opt.gate:
        ld = N + (4 if f.vec else 5)
        operand("gate", _gate(3 * v + M * ld + 8, seed + 4, f.dtype), "gate_off", 3 * v, "ld_gate", ld)
    if opt.mask:
        kw["row_mask"] = opt.mask
    if opt.stat_z is not None:
        ld = N + (12 if f.vec else 7)
        operand("stat_z", torch.tanh(torch.randn(v + M * ld + 8, generator=_gen(seed + 5))).to(opt.stat_z), "stat_z_off", v,
                "ld_stat_z", ld)
        operand("stat_mean", 0.1 * torch.randn(N, generator=_gen(seed + 6)))
        operand("stat_istd", 1.0 + 0.2 * torch.rand(N, generator=_gen(seed + 7)))
    stats = opt.stats and "stats" in f.caps     # the skinny forms never see statistics: the dispatch routes those calls away
    sums = torch.full((2 * N,), float("nan"), device=dev) if stats else None
    if o.A_lo is not None:
        dkw.update(a_lo=o.dA_lo, b_lo=o.dB_lo)
    runs = []
    for _ in range(repeats):
        Cd = prior.to(dev, copy=True)
        call = dict(kw, **dkw)
        if stats:
            call.update(col_sum=sums, col_sumsq=sums[N:])
        ops.gemm(o.dA, o.dB, Cd, M, N, K, o.lda, o.ldb, ldc, **call)
        assert profiling._last_kernel() == f.kernel, (profiling._last_kernel(), f.kernel)
        torch.cuda.synchronize()
        runs.append(Cd.cpu())
    full = runs[-1]
    outside = torch.ones(prior.numel(), dtype=torch.bool)
    outside[region] = False
    assert torch.equal(_bits(full)[outside], _bits(prior)[outside]), "the call wrote outside its region of C"
    got = full.double()[region].reshape(opt.batch, M, N)
    ref = R.gemm_ref(o.A, o.B, prior, M, N, K, o.lda, o.ldb, ldc, a_lo=o.A_lo, b_lo=o.B_lo, cache=o.cache, **kw)
    want_off = prior.double()[region].reshape(opt.batch, M, N) if opt.accumulate else torch.zeros_like(got)
    assert torch.equal(got[ref.off], want_off[ref.off]), "masked / gated-off elements are exact"
    if opt.gate or (opt.mask == MASK_SHORT and M >= 4) or (opt.mask == MASK and M >= 26):       # the case does switch elements off
        assert ref.off.any() and not ref.off.all()
    err, bound = (got - ref.exact).abs(), _bound(f, o, ref, opt)       # from the unrounded value: the store term is the rounding
    ratio = (err / bound).max().item()
    worst = int((err / bound).argmax())
    assert bool((err <= bound).all()), "err / bound %.3g at flat element %d: got %r, want %r" % (
        ratio, worst, got.reshape(-1)[worst].item(), ref.exact.reshape(-1)[worst].item())
    sratio = 0.0
    if stats:
        zz = mean = istd = None
        if opt.stat_z is not None:
            zz = R._take(kw["stat_z"], R._mn(M, N, kw["ld_stat_z"], kw["stat_z_off"]))
            mean, istd = kw["stat_mean"].double(), kw["stat_istd"].double()
        s1, s2, a1, a2 = R.column_stats(got[0], ref.valid, zz, mean, istd)
        sd = sums.double().cpu()
        tol = 2.0 * (M + 4) * U
        e1, e2 = (sd[:N] - s1).abs(), (sd[N:] - s2).abs()
        sratio = max((e1 / (tol * a1)).max().item(), (e2 / (tol * a2)).max().item())
        assert bool((e1 <= tol * a1).all()), "col_sum: err / tolerance %.3g" % sratio
        assert bool((e2 <= tol * a2).all()), "col_sumsq: err / tolerance %.3g" % sratio
    print("RATIO %s %s err/bound %.4f stats %.4f" % (f.id, opt.id, ratio, sratio))
    return ratio, sratio, runs


@pytest.mark.parametrize("form,opt", _cases())
def test_gemm_epilogue(dev, monkeypatch, form, opt):
    from nspeech_amd import ops
    monkeypatch.setattr(ops, "DETERMINISTIC_SPLITK", bool(opt.det))
    _, _, runs = _run_case(dev, form, opt, repeats=3 if opt.det else 1)
    if opt.det:         # a fixed summation order: the same bits every time, and the tile counters left at zero
        assert torch.equal(_bits(runs[0]), _bits(runs[1])) and torch.equal(_bits(runs[0]), _bits(runs[2]))
        counters = ops._splitk_scratch(torch.zeros(1, device=dev).device, form.M, form.N, opt.split_k)[1]
        assert int(counters.abs().max().item()) == 0


# ------------------------------------------------------------------ the BatchNorm finaliser folded into the statistics' second stage
# ns_gemm_params.bn: gemm_stats_finalize_kernel goes on from a column's sums to mean / 1/std and the moving statistics.
# 64-row slots: 2200 rows are 35 (more than the 32 slot lanes: the strided slot loop), 130 rows 3; N = 36 leaves a ragged
# second block of 32 columns.  The four outputs are held to pointwise_ref.bn_finalize applied to the col_sum / col_sumsq
# that the SAME call returned (which test_gemm_epilogue holds to float64 sums), at the bound of the bn_fwd contract.
@pytest.mark.parametrize("rows,N,dtype", [(2200, 128, f32), (130, 512, bf), (2200, 36, f32)],
                         ids=["35-slots", "3-slots", "N36"])
def test_bn_fold_against_the_bn_fwd_contract(dev, rows, N, dtype):
    import numpy as np
    import pointwise_ref as P
    from nspeech_amd import ops
    K, mask = 64, (110, 3, 104, 0)
    g = _gen(rows + N)
    A = (torch.randn(rows, K, generator=g) * 0.3).to(dtype).to(dev)
    B = (torch.randn(N, K, generator=g) * 0.3).to(dtype).to(dev)
    bias = (torch.randn(N, generator=g) * 0.1).to(dev)
    mm0, mv0 = 0.1 * torch.randn(N, generator=g), 1.0 + 0.2 * torch.rand(N, generator=g)
    count = float(R.valid_rows(rows, mask).sum())
    z = torch.full((rows, N), float("nan"), dtype=dtype, device=dev)
    st = torch.full((4 * N + 8,), float("nan"), device=dev)
    st[4 * N:] = SENTINEL
    mm, mv = mm0.to(dev), mv0.to(dev)
    ops.gemm(A, B, z, rows, N, K, K, K, N, bias=bias, act=R.ACT_RELU, row_mask=mask, col_sum=st, col_sumsq=st[N:], f32_passes=0,
             bn=dict(count=count, training=True, moving_mean=mm, moving_var=mv, mean_out=st[2 * N:], istd_out=st[3 * N:]))
    torch.cuda.synchronize()
    got = st.cpu().numpy()
    assert (got[4 * N:] == SENTINEL).all()
    fr = lambda x: (P.framed(np.asarray(x, np.float32)), "f32")
    c = dict(p=dict(C=N, training=1, count=count, momentum=0.99, eps=1e-3),
             bufs=dict(col_sum=fr(got[:N]), col_sumsq=fr(got[N:2 * N]), moving_mean=fr(mm0.numpy()), moving_var=fr(mv0.numpy())))
    want = P.bn_finalize(P.RunErr(), c)
    have = (got[2 * N:3 * N], got[3 * N:4 * N], mm.cpu().numpy(), mv.cpu().numpy())
    for name, w, h in zip(("mean_out", "istd_out", "moving_mean", "moving_var"), want, have):
        val, err = P.RunErr().out(w)
        v = P.accepts(h, val, err, "f32", 2.0)
        print("BN FOLD %s %-12s error / bound %.3f" % ((rows, N), name, v.worst))
        assert v.ok, (name, v.why)
    assert not np.array_equal(mm.cpu().numpy(), mm0.numpy())


# ------------------------------------------------------------------ refusals: an argument error, and nothing launched
def _refused(dev, M=64, N=128, K=64, dtype=bf, c_dtype=f32, presplit=False, **kw):
    from nspeech_amd import ops
    from nspeech_amd import _lib as L
    A = _uniform(M * K, 1).to(dtype).to(dev)
    B = _uniform(N * K, 2).to(dtype).to(dev)
    if presplit:
        kw.update(a_lo=torch.zeros_like(A), b_lo=torch.zeros_like(B))
    before = torch.full((M * N,), SENTINEL).to(c_dtype)
    Cm = before.to(dev)
    with pytest.raises(L.NSError):
        ops.gemm(A, B, Cm, M, N, K, K, K, N, **kw)
    torch.cuda.synchronize()
    assert torch.equal(_bits(Cm.cpu()), _bits(before)), "a refused call must not launch a kernel"


@pytest.mark.parametrize("M", [32, 8])
def test_pre_split_operands_are_refused_on_skinny_shapes(dev, M):
    """M <= 32, bf16, both operands k-contiguous: the skinny kernel reads A and B only and would drop the low parts"""
    _refused(dev, M=M, presplit=True)


def test_col_sumsq_without_col_sum_is_refused(dev):
    _refused(dev, col_sumsq=torch.zeros(128, device=dev))


def test_accumulate_into_bf16_is_refused(dev):
    _refused(dev, c_dtype=bf, accumulate=1)


def test_split_k_with_an_activation_is_refused(dev):
    _refused(dev, split_k=2, accumulate=2, act=R.ACT_RELU)


def test_stat_z_with_atomic_accumulate_is_refused(dev):
    s = torch.zeros(2 * 128, device=dev)
    _refused(dev, accumulate=2, col_sum=s, col_sumsq=s[128:], stat_z=torch.zeros(64 * 128, device=dev), ld_stat_z=128,
             stat_mean=torch.zeros(128, device=dev), stat_istd=torch.ones(128, device=dev))


def test_two_passes_on_fp32_operands_without_low_parts_are_refused(dev):
    """f32_passes = 2 means the two-segment product of PRE-SPLIT bf16 operands; on fp32 operands it used to run the
    one-pass product without saying so"""
    _refused(dev, dtype=f32, f32_passes=2)
    _refused(dev, M=16, dtype=f32, f32_passes=2)
