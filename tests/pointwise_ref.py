"""Float64 contract of the element-wise, reduction and optimiser kernels (csrc/elementwise.hip, ns_zero / ns_zero_many of
core.hip), stated from include/nspeech_hip.h and the models that call them - not from the kernels.  Proven on the CPU by
tests/test_pointwise_ref_cpu.py; tests/test_pointwise_contract_gpu.py holds every kernel form to it.

A CASE is a dict: op, name, p (the call's scalar arguments), bufs {name: (flat float32 / int array, "f32" | "bf16" | "i32"
| "i64")} - every buffer the call sees, outputs with their prefill and sentinel margins - and outs (the buffers the call may
write).  expect(case) -> {out: (value float64, err)} over the WHOLE buffer: margins, padding and skipped columns are
expected as they were, so comparing every element is also the margin check.  Three kinds of expected value:

  exact     err is None: the contract is a copy or a rounding (or a one-hot probe / an exact-by-construction sum, below);
            the kernel's bits must be those of float32(value) - or RNE_bf16 of it for a bf16 buffer.
  exact by construction (reductions): inputs are integer multiples of one unit (1/4; squares 1/16) with
            sum |terms| / unit < 2^24, prefill included (assert_exact_sum), so every partial sum in every order is an
            exact fp32 number and the result is order-free.
  bounded   err is the first-order running-error bound of the documented expression, computed beside the value by
            RunErr: each fp32 operation with result r adds 2^-24 |r| and earlier errors travel through the absolute
            partial derivatives; constants formed in fp32 (1 - beta1) are operations like any other; division and sqrtf
            are one rounding each; the inverse square root of BatchNorm's finalise (rsqrtf) is charged RSQRT_ULP = 2 ulp
            (no table of ROCm's device-library ulp figures is installed beside the compiler, so the issue's fallback
            figure is used); a sum of n terms in an unknown order is charged (n - 1) 2^-24 sum |x_i|.  Contraction to FMA
            only removes roundings.  The GPU test's bound is 2 x err (the second-order terms); float32 emulations of a
            correct kernel stay within 1 x err (worst ratios, measured by the CPU module over its association orders
            with and without FMA):
              bn_fwd 0.920  bn_bwd 0.915  adam 0.998  highway 0.997  act_bwd 0.853  gru_pointwise 0.995  random sums 0.014
            BatchNorm backward (ns_bn_bwd / ns_bn_bwd_finalize): dpre carries the bound of its whole expression, the
            error of the two column sums included where the call forms them (Exact, an arithmetic that asserts that no
            operation rounds, replaces RunErr in its exact-by-construction cases); dgamma / dbeta are ONE fp32 add of
            given sums - exact - or bounded sums; dbias is held to the column sums of the dpre that the same call stored
            (check()), and bit for bit in the exact cases.
  A value stored as bf16 follows the "bf16 store" rule of tests/test_wavenet_contract_gpu.py (restated in accepts()).

`mut` arguments select the WRONG kernels that the CPU module shows the comparison to reject; None is the contract.
"""
import numpy as np

U = 2.0 ** -24            # unit roundoff of fp32
RSQRT_ULP = 2.0           # see the module docstring
SENT = 7.0                # sentinel: margins, padding, columns a leading dimension leaves out
MARGIN = 8                # elements of SENT on either side of every buffer (keeps 16-byte alignment)
UNIT = 0.25               # exact-by-construction inputs are multiples of it
ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID, ACT_SOFTSIGN = range(5)


# ------------------------------------------------------------------------------------------------------ roundings
def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def rne_bf16(x):
    """float32 -> the nearest bf16 value (ties to even), as float32.  Finite inputs."""
    u = _u32(x).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32).reshape(np.shape(x))


def trunc_bf16(x):
    return (_u32(x) & np.uint32(0xFFFF0000)).view(np.float32).reshape(np.shape(x))


def store(x32, dtype):
    return rne_bf16(x32) if dtype == "bf16" else np.asarray(x32, np.float32)


def split_hi_lo(x32, mut=None):
    x32 = np.asarray(x32, np.float32)
    hi = trunc_bf16(x32) if mut == "truncate" else rne_bf16(x32)
    lo = rne_bf16(x32 - (trunc_bf16(x32) if mut == "lo_unrounded" else hi))       # the subtraction is exact in fp32
    return hi, (trunc_bf16(x32 - hi) if mut == "truncate" else lo)


# ------------------------------------------------------------------------------------------------------ arithmetics
class RunErr(object):
    """Values are (value, first-order error bound) pairs of float64 arrays."""

    def lift(self, x):
        x = np.asarray(x, np.float64)
        return (x, np.zeros_like(x))

    def _r(self, v, e):
        return (v, e + U * np.abs(v))

    def add(self, a, b):
        return self._r(a[0] + b[0], a[1] + b[1])

    def sub(self, a, b):
        return self._r(a[0] - b[0], a[1] + b[1])

    def mul(self, a, b):
        return self._r(a[0] * b[0], np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1])

    def div(self, a, b):
        q = a[0] / b[0]
        return self._r(q, (a[1] + np.abs(q) * b[1]) / np.abs(b[0]))

    def sqrt(self, a):
        r = np.sqrt(a[0])
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.where(r > 0, a[1] / (2 * r), np.sqrt(a[1]))
        return self._r(r, d)

    def rsqrt(self, a):
        r = a[0] ** -0.5
        return (r, 0.5 * r / a[0] * a[1] + RSQRT_ULP * 2 * U * r)

    def neg(self, a):
        return (-a[0], a[1])

    def abs(self, a):
        return (np.abs(a[0]), a[1])

    def maximum(self, a, b):
        return (np.maximum(a[0], b[0]), np.maximum(a[1], b[1]))

    def where(self, c, a, b):
        return (np.where(c, a[0], b[0]), np.where(c, a[1], b[1]))

    def prod(self, fs):
        r = fs[0]
        for f in fs[1:]:
            r = self.mul(r, f)
        return r

    def muladd(self, fs, c):
        return self.add(self.prod(fs), c)

    def dot2(self, a, b, c, d):
        return self.add(self.mul(a, b), self.mul(c, d))

    def colsum(self, a, n):
        """Sum over axis 0 of n terms (the others are +0) in an unknown order: the terms' own errors and the module's
        charge (n - 1) 2^-24 sum |x_i|."""
        return (a[0].sum(0), a[1].sum(0) + max(n - 1, 0) * U * np.abs(a[0]).sum(0))

    def value(self, a):
        return a[0]

    def out(self, a, shape=None):
        v, e = np.broadcast_arrays(a[0], a[1])
        return v.astype(np.float64), e.astype(np.float64)


def quantum(x):
    """The largest power of two that divides every element of x (float64 values that are exact binary fractions)."""
    x = np.abs(np.asarray(x, np.float64).reshape(-1))
    x = x[x != 0]
    q = 1.0
    while x.size and (np.floor(x / q) != x / q).any():
        q /= 2
        assert q > 2.0 ** -60
    return q


class Exact(RunErr):
    """Exact by construction, asserted and not assumed: every operation's result must be an fp32 number as it stands
    (so no operation rounds, fused or not), every sum must meet assert_exact_sum on its terms' own quantum."""

    def _r(self, v, e):
        v = np.asarray(v, np.float64)
        assert (v.astype(np.float32).astype(np.float64) == v).all(), "an intermediate is not an fp32 number"
        return (v, np.zeros_like(v))

    def colsum(self, a, n):
        assert_exact_sum(np.abs(a[0]).sum(0), quantum(a[0]))
        return self._r(a[0].sum(0), 0)


class F32(object):
    """The same expressions in NumPy float32: `order` picks the association of every product chain (rotations of the
    factor list, and pairs first), `fma` fuses the last multiply of a multiply-add (product in float64, rounded once)."""

    def __init__(self, order=0, fma=False):
        self.order, self.fma = order, fma

    def lift(self, x):
        return np.asarray(x, np.float32)

    def add(self, a, b):
        return np.float32(a) + np.float32(b)

    def sub(self, a, b):
        return np.float32(a) - np.float32(b)

    def mul(self, a, b):
        return np.float32(a) * np.float32(b)

    def div(self, a, b):
        return np.float32(a) / np.float32(b)

    def sqrt(self, a):
        return np.sqrt(np.float32(a))

    def rsqrt(self, a):
        return (np.asarray(a, np.float64) ** -0.5).astype(np.float32)

    def neg(self, a):
        return -np.float32(a)

    def abs(self, a):
        return np.abs(np.float32(a))

    def maximum(self, a, b):
        return np.maximum(np.float32(a), np.float32(b))

    def where(self, c, a, b):
        return np.where(c, np.float32(a), np.float32(b)).astype(np.float32)

    def _arranged(self, fs):
        k = self.order % len(fs)
        return list(fs[k:]) + list(fs[:k])

    def prod(self, fs):
        fs = self._arranged(fs)
        if len(fs) >= 4 and self.order >= len(fs):           # pairs first
            return self.mul(self.mul(fs[0], fs[1]), self.prod_plain(fs[2:]))
        return self.prod_plain(fs)

    def prod_plain(self, fs):
        r = fs[0]
        for f in fs[1:]:
            r = self.mul(r, f)
        return r

    def _fma(self, a, b, c):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)

    def muladd(self, fs, c):
        fs = self._arranged(fs)
        head = self.prod_plain(fs[:-1])
        return self._fma(head, fs[-1], c) if self.fma else self.add(self.mul(head, fs[-1]), c)

    def dot2(self, a, b, c, d):
        if not self.fma:
            return self.add(self.mul(a, b), self.mul(c, d))
        return self._fma(a, b, self.mul(c, d)) if self.order % 2 == 0 else self._fma(c, d, self.mul(a, b))

    def colsum(self, a, n):
        """float32 sums over axis 0 in four orders: forward, backward, NumPy's pairwise, 64 interleaved lanes."""
        a = np.asarray(a, np.float32)
        seq = lambda v: np.cumsum(v, 0, dtype=np.float32)[-1]
        k = self.order % 4
        if k == 0:
            return seq(a)
        if k == 1:
            return seq(a[::-1])
        if k == 2:
            return np.add.reduce(a, 0, dtype=np.float32)
        pad = np.concatenate([a, np.zeros((-len(a) % 64,) + a.shape[1:], np.float32)]).reshape((-1, 64) + a.shape[1:])
        return seq(seq(pad))

    def value(self, a):
        return np.asarray(a, np.float64)

    def out(self, a, shape=None):
        return np.asarray(a, np.float32)


# ------------------------------------------------------------------------------------------------------ comparison
def bits_equal(got, want):
    return _u32(got) == _u32(want)


class Verdict(object):
    def __init__(self, ok, worst=0.0, why="", neighbours=0, counted=0):
        self.ok, self.worst, self.why, self.neighbours, self.counted = ok, worst, why, neighbours, counted

    def __bool__(self):
        return bool(self.ok)
    __nonzero__ = __bool__


def bf16_coarse(val, band):
    """Where bf16 is coarser than the band: its spacing at val is at least 4 x band."""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(val), 1e-300))) - 7) >= 4 * band


def accepts(got, val, err, dtype="f32", factor=2.0):
    """Does `got` (float32 array of what the buffer holds; bf16 buffers widened exactly) meet the expectation?  Every
    element is compared.  err None: bit equality with float32(val), or RNE_bf16 of it.  Otherwise fp32 buffers:
    |got - val| <= factor * err (so an element with err 0 - a margin, a masked row - must EQUAL val); bf16 buffers, the
    bf16 store rule with band = factor * err: bf16(val - band) <= got <= bf16(val + band), and at most 1 % of the computed
    values (err > 0) may differ from bf16(val), counted where bf16 is coarser than the band (spacing >= 4 x band)."""
    got = np.asarray(got, np.float32).reshape(-1)
    val = np.asarray(val).reshape(-1)
    assert got.shape == val.shape, (got.shape, val.shape)
    if err is not None and (~np.isfinite(got) & (got != val)).any():          # (an empty segment's min / max are +-inf)
        return Verdict(False, np.inf, "non-finite output")
    if err is None:
        want = store(np.asarray(val, np.float32), dtype)
        bad = ~bits_equal(got, want)
        return Verdict(not bad.any(), 0.0, "%d of %d elements differ in bits, first at %s" %
                       (bad.sum(), bad.size, np.flatnonzero(bad)[:4]))
    err = np.broadcast_to(np.asarray(err, np.float64), val.shape).reshape(-1)
    band = factor * err
    with np.errstate(invalid="ignore"):
        d = np.where(got == val, 0.0, np.abs(got.astype(np.float64) - val))
    if dtype == "f32":
        bad = ~(d <= band)
        live = band > 0
        worst = float((d[live] / band[live]).max()) if live.any() else 0.0
        return Verdict(not bad.any(), worst, "%d of %d elements beyond the bound, first at %s, worst %.3g x" %
                       (bad.sum(), bad.size, np.flatnonzero(bad)[:4], worst))
    lo, hi = rne_bf16((val - band).astype(np.float32)), rne_bf16((val + band).astype(np.float32))
    bad = ~((lo <= got) & (got <= hi))
    counted = (err > 0) & bf16_coarse(val, band)
    neigh = counted & (got != rne_bf16(val.astype(np.float32)))
    n, m = int(neigh.sum()), int((err > 0).sum())
    worst = n / (0.01 * m) if m else 0.0
    ok = not bad.any() and n <= 0.01 * m
    return Verdict(ok, worst, "%d of %d outside the band (first at %s); %d neighbours of %d computed values" %
                   (bad.sum(), bad.size, np.flatnonzero(bad)[:4], n, m), n, m)


def pair_accepts(hi, lo, val, err, factor=2.0):
    """A pre-split pair written WITHOUT the fp32 value beside it: hi follows the bf16 store rule; lo = bf16(y - hi) of the
    kernel's own y leaves |hi + lo - y| <= 2^-16 |y| (bf16 rounds to 8 significant bits: lo's rounding is at most 2^-8 of a
    remainder of at most 2^-8 |y|), so |hi + lo - val| <= factor * err + 2^-16 (|val| + factor * err)."""
    v = accepts(hi, val, err, "bf16", factor)
    if not v:
        return v
    err = np.broadcast_to(np.asarray(err, np.float64), np.shape(val)).reshape(-1)
    s = np.asarray(hi, np.float64).reshape(-1) + np.asarray(lo, np.float64).reshape(-1)
    lim = factor * err + 2.0 ** -16 * (np.abs(val).reshape(-1) + factor * err)
    bad = ~(np.abs(s - np.asarray(val).reshape(-1)) <= lim)
    return Verdict(not bad.any(), v.worst, "hi + lo: %d elements beyond the bound" % bad.sum(), v.neighbours, v.counted)


# ------------------------------------------------------------------------------------------------------ inputs
def framed(x, fill=SENT, margin=MARGIN):
    x = np.asarray(x, np.float32).reshape(-1)
    return np.concatenate([np.full(margin, fill, np.float32), x, np.full(margin, fill, np.float32)])


def rounding_values(n, seed, bf16=False):
    """n float32 values for the contracts that are a rounding: bf16 ties in both directions (1 + 2^-8 rounds down to even,
    1 + 3 2^-8 up), one fp32 ulp either side of a tie, both signs, -0.0 and 0.0, magnitudes 2^-30 .. 2^30."""
    rng = np.random.RandomState(seed)
    head = []
    for s in (1.0, -1.0):
        for e in (0, -30, 30, 7):
            for m in (1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8):
                t = np.float32(s * m * 2.0 ** e)
                head += [t, np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(-np.inf))]
    head += [np.float32(-0.0), np.float32(0.0), np.float32(2.0 ** -30), np.float32(-2.0 ** 30)]
    man = rng.randint(0, 1 << 23, n).astype(np.uint32)
    tie = rng.rand(n) < 0.5                            # half of them: a tie pattern, or one ulp beside it
    man = np.where(tie, (man & np.uint32(0x7F0000)) | np.uint32(0x8000), man)
    man = (man.astype(np.int64) + np.where(tie, rng.randint(-1, 2, n), 0)).astype(np.uint32) & np.uint32(0x7FFFFF)
    exp = rng.randint(127 - 30, 127 + 30, n).astype(np.uint32)
    sign = rng.randint(0, 2, n).astype(np.uint32)
    x = ((sign << 31) | (exp << 23) | man).view(np.float32)
    x[:min(n, len(head))] = np.asarray(head, np.float32)[:n]
    return rne_bf16(x) if bf16 else x


def unit_values(shape, seed, most=2):
    """Non-zero integer multiples of UNIT, |multiple| <= most."""
    rng = np.random.RandomState(seed)
    m = rng.randint(1, most + 1, shape) * (2 * rng.randint(0, 2, shape) - 1)
    return (m * UNIT).astype(np.float32)


def assert_exact_sum(abs_terms_total, unit):
    """The exactness condition: sum |terms| / unit < 2^24 (the prefilled accumulator is a term)."""
    assert float(np.max(abs_terms_total)) / unit < 2 ** 24, (float(np.max(abs_terms_total)), unit)


def sum_expect(val, abs_total, n_terms, exact, unit=UNIT):
    """Expectation of a sum: exact by construction, or (n - 1) 2^-24 sum |x_i| for an unknown order."""
    if exact:
        assert_exact_sum(abs_total, unit)
        return None
    return np.maximum(np.asarray(n_terms, np.float64) - 1, 0) * U * abs_total


def row_valid(rows, mask):
    if not mask:
        return np.ones(rows, bool)
    period, lo, hi = mask
    t = np.arange(rows) % period
    return (t >= lo) & (t < hi)


# ------------------------------------------------------------------------------------------------------ expectations
def _f64(c, name):
    return c["bufs"][name][0].astype(np.float64)


def _whole(c, outs):
    """{out: (value, None)} of the untouched buffers, to be filled in."""
    return {o: [c["bufs"][o][0].astype(np.float64), None] for o in outs}


def expect_copy3d(c, mut=None):
    p, (src, sdt), (dst, ddt) = c["p"], c["bufs"]["src"], c["bufs"]["dst"]
    i, j, k = np.indices((p["I"], p["J"], p["Cc"]))
    s = src[p["src_off"] + i * p["src_strides"][0] + j * p["src_strides"][1] + k]
    d = p["dst_off"] + i * p["dst_strides"][0] + j * p["dst_strides"][1] + k
    out = dst.copy()
    v = (dst[d] + s).astype(np.float32) if p["accumulate"] and mut != "overwrite" else s        # ONE fp32 add
    out[d] = trunc_bf16(v) if (mut == "truncate" and ddt == "bf16") else store(v, ddt)
    return {"dst": (out, None)}


def _ids(c, mut=None):
    ids, V = c["bufs"]["ids"][0].astype(np.int64), c["p"]["V"]
    return ids % V if mut == "no_clamp" else np.clip(ids, 0, V - 1)


def expect_embedding_fwd(c, mut=None):
    p = c["p"]
    table, out = c["bufs"]["table"][0], c["bufs"]["out"][0].copy()
    N, T, P, padl, D = p["N"], p["T"], p["P"], p["padl"], p["D"]
    ids = _ids(c, mut).reshape(N, T)
    rows = (np.arange(N)[:, None] * P + padl + np.arange(T)[None, :]).reshape(-1)
    src = table[p["table_off"] + ids.reshape(-1)[:, None] * D + np.arange(D)[None, :]]
    out[MARGIN + rows[:, None] * D + np.arange(D)[None, :]] = store(src, c["bufs"]["out"][1])
    return {"out": (out, None)}


def expect_embedding_bwd(c, mut=None):
    p = c["p"]
    N, T, P, padl, D, V = p["N"], p["T"], p["P"], p["padl"], p["D"], p["V"]
    ids = _ids(c, mut).reshape(-1)
    dout = _f64(c, "dout")
    rows = (np.arange(N)[:, None] * P + padl + np.arange(T)[None, :]).reshape(-1)
    terms = dout[MARGIN + rows[:, None] * D + np.arange(D)[None, :]]
    acc, ab, cnt = np.zeros((V, D)), np.zeros((V, D)), np.zeros((V, 1))
    np.add.at(acc, ids, terms)
    np.add.at(ab, ids, np.abs(terms))
    np.add.at(cnt, ids, 1.0)
    out = _f64(c, "dtable")
    sl = slice(p["dtable_off"], p["dtable_off"] + V * D)
    old = np.zeros(V * D) if mut == "overwrite" else out[sl]
    err = np.zeros_like(out)
    e = sum_expect(acc, ab + np.abs(old.reshape(V, D)), cnt + 1, c["exact"])
    out[sl] = (old.reshape(V, D) + acc).reshape(-1)
    if e is not None:
        err[sl] = e.reshape(-1)
    return {"dtable": (out, None if c["exact"] else err)}


def bn_finalize(A, c, mut=None):
    """mean, istd and the new moving statistics of tf.layers.batch_normalization (axis -1): biased batch variance
    sumsq / count - mean^2, clamped at 0; moving = moving * momentum + batch * (1 - momentum)."""
    p, b = c["p"], c["bufs"]
    C = p["C"]
    get = lambda name: A.lift(b[name][0][MARGIN:MARGIN + C])
    mm = get("moving_mean") if "moving_mean" in b else None
    if p["training"]:
        count = A.lift(np.float32(p["count"]))
        mean = A.div(get("col_sum"), count)
        var = A.muladd([A.neg(mean), mean], A.div(get("col_sumsq"), count))
        if mut != "no_clamp":
            var = A.maximum(var, A.lift(np.float32(0)))
        if mm is not None:
            mom = A.lift(np.float32(p["momentum"]))
            one_m = A.sub(A.lift(np.float32(1)), mom)
            if mut == "momentum_swapped":
                mom, one_m = one_m, mom
            new_mm, new_mv = A.dot2(mm, mom, mean, one_m), A.dot2(get("moving_var"), mom, var, one_m)
        else:
            new_mm = new_mv = None
    else:
        mean, var, new_mm, new_mv = mm, get("moving_var"), None, None
    istd = A.rsqrt(A.add(var, A.lift(np.float32(p["eps"]))))
    return mean, istd, new_mm, new_mv


def compute_bn_fwd(c, A, mut=None):
    """y = (z - mean) * istd * gamma + beta, 0 in rows that fail the (period, lo, hi) test.  -> {buffer: A value over the
    buffer's written elements}, plus "y_value": the unrounded y of the logical [rows, C] array."""
    p, b = c["p"], c["bufs"]
    rows, C = p["rows"], p["C"]
    res = {}
    if p["stats_final"]:
        mean, istd = A.lift(b["mean_out"][0][MARGIN:MARGIN + C]), A.lift(b["istd_out"][0][MARGIN:MARGIN + C])
    else:
        mean, istd, mm, mv = bn_finalize(A, c, mut)
        res["mean_out"], res["istd_out"] = mean, istd
        if mm is not None:
            res["moving_mean"], res["moving_var"] = mm, mv
    z = A.lift(b["z"][0][MARGIN:MARGIN + rows * C].reshape(rows, C))
    g, be = A.lift(b["gamma"][0][MARGIN:MARGIN + C]), A.lift(b["beta"][0][MARGIN:MARGIN + C])
    y = A.muladd([A.sub(z, mean), istd, g], be)
    valid = row_valid(rows, None if mut == "mask_ignored" else p["row_mask"])[:, None]
    res["y_value"] = A.where(valid, y, A.lift(np.zeros((rows, C), np.float32)))
    return res


def expect_bn_fwd(c):
    p = c["p"]
    rows, C = p["rows"], p["C"]
    r = compute_bn_fwd(c, RunErr())
    res = _whole(c, c["outs"])
    for name in ("mean_out", "istd_out", "moving_mean", "moving_var"):
        if name in r:
            v, e = RunErr().out(r[name])
            res[name][1] = np.zeros_like(res[name][0])
            res[name][0][MARGIN:MARGIN + C], res[name][1][MARGIN:MARGIN + C] = v, e
    yv, ye = RunErr().out(r["y_value"])
    if "y" in c["outs"]:
        ld = p["ld_y"] or C
        idx = (p["y_off"] + np.arange(rows)[:, None] * ld + np.arange(C)[None, :]).reshape(-1)
        res["y"][1] = np.zeros_like(res["y"][0])
        res["y"][0][idx], res["y"][1][idx] = yv.reshape(-1), ye.reshape(-1)
    out = {o: (v, e if e is not None else np.zeros_like(v)) for o, (v, e) in res.items() if o not in ("y_hi", "y_lo")}
    out["y_value"] = (yv, ye)              # the pre-split pair is held to it (pair_accepts) or to the kernel's own y
    return out


# BatchNorm backward.  Host restatement of ns_bn_bwd's choice of kernels (bn_bwd_vector_form, bn_bwd_row_blocks and the
# scalar form's grid in csrc/elementwise.hip): "vector" = bn_bwd_apply4_kernel + bn_bwd_finalize_kernel on the given sums,
# "fallback" = the same behind bn_bwd_reduce4_kernel + ns_stats_finalize, "scalar" = bn_bwd_reduce_kernel +
# bn_bwd_apply_kernel (+ the ordered bias pass), which recomputes given sums.  p["off"][buffer] is the element offset of
# the operand in its buffer; every buffer itself is 16-byte aligned.
BN_BWD_BUFFERS = ("dy", "z", "dpre", "mean", "istd", "gamma", "work", "sum_dy", "sum_dyxh")


def bn_bwd_form(c, byte_offset=None):
    """byte_offset(buffer) -> the operand's address modulo 16; None: from p["off"] and the element sizes."""
    p, b = c["p"], c["bufs"]
    size = lambda k: 2 if b[k][1] == "bf16" else 4
    at = byte_offset or (lambda k: p["off"][k] * size(k) % 16)
    al = lambda k, n: at(k) % n == 0
    ok = p["C"] % 4 == 0 and p["ld_dy"] % 4 == 0 and al("dy", 16) and al("z", 4 * size("z")) and al("dpre", 4 * size("dpre"))
    ok = ok and all(al(k, 16) for k in ("mean", "istd", "gamma", "work"))
    if p["sums"]:
        ok = ok and al("sum_dy", 16) and al("sum_dyxh", 16)
    return ("vector" if p["sums"] else "fallback") if ok else "scalar"


def bn_bwd_row_blocks(c):
    """(row blocks, rows per block) of the case's form."""
    rows = c["p"]["rows"]
    nb = max(1, min(32, -(-rows // 64))) if bn_bwd_form(c) == "scalar" else max(1, min(64, -(-rows // 128)))
    return nb, -(-rows // nb)


def compute_bn_bwd(c, A, mut=None):
    """include/nspeech_hip.h, ns_bn_bwd: modules.py:194-198 (y = BN(act(pre))) differentiated.  With V the rows that pass
    the (period, lo, hi) test and xhat = (z - mean) * istd:
        s1 = sum_V dy, s2 = sum_V dy * xhat (or the given sums as they stand - the vector form), 1 / count formed once and
        multiplied with (two roundings), dz = gamma * istd * (dy - s1 / count - xhat * s2 / count), dpre = dz * act'(z) in
        V and +0 elsewhere; act' through z as in compute_act_bwd.  Masked rows of dy and z are not looked at.
    -> dict(dpre [rows, C], s1, s2 [C]: A values; given: the sums were taken as handed in)."""
    p, b = c["p"], c["bufs"]
    rows, C, act, off = p["rows"], p["C"], p["act"], p["off"]
    vec = lambda name: A.lift(b[name][0][off[name]:off[name] + C])
    ld = C if mut == "ld_ignored" else (p["ld_dy"] or C)
    valid = row_valid(rows, p["row_mask"])[:, None]
    look = np.ones_like(valid) if mut in ("sums_unmasked", "dpre_mask_ignored") else valid
    dy = A.lift(np.where(look, b["dy"][0][off["dy"] + np.arange(rows)[:, None] * ld + np.arange(C)[None, :]], np.float32(0)))
    z = A.lift(np.where(look, b["z"][0][off["z"]:off["z"] + rows * C].reshape(rows, C), np.float32(0)))
    mean, istd, gamma = vec("mean"), vec("istd"), vec("gamma")
    one, zero = A.lift(np.float32(1)), A.lift(np.zeros((rows, C), np.float32))
    centred = A.sub(z, mean)
    xhat = A.mul(centred, istd)
    given = bool(p["sums"]) and bn_bwd_form(c) == "vector" and mut != "recompute_sums"
    if given:
        s1, s2 = vec("sum_dy"), vec("sum_dyxh")
    else:
        summed = np.ones_like(valid) if mut == "sums_unmasked" else valid
        if mut == "drop_last_block":
            nb, rpb = bn_bwd_row_blocks(c)
            summed = summed & (np.arange(rows) < (nb - 1) * rpb)[:, None]
        n = int(summed.sum())
        s1 = A.colsum(A.where(summed, dy, zero), n)
        s2 = A.colsum(A.where(summed, A.mul(dy, centred if mut == "s2_no_istd" else xhat), zero), n)
    inv = A.div(one, A.lift(np.float32(rows if mut == "count_rows" else p["count"])))
    inner = A.muladd([A.neg(xhat), A.mul(s2, inv)], A.sub(dy, A.mul(s1, inv)))
    d = A.prod([gamma, inner] if mut == "no_istd_scale" else [gamma, istd, inner])
    zv = A.value(z)
    if act == ACT_RELU:
        d = A.where((zv >= 0) if mut == "relu_at_zero" else (zv > 0), d, zero)
    elif act == ACT_TANH:
        d = A.mul(d, A.sub(one, z) if mut == "tanh_linear" else A.muladd([A.neg(z), z], one))
    elif act == ACT_SIGMOID:
        d = A.prod([d, z, A.add(one, z) if mut == "sigmoid_plus" else A.sub(one, z)])
    elif act == ACT_SOFTSIGN:
        f = A.sub(one, A.abs(z))
        d = A.mul(d, f) if mut == "softsign_unsquared" else A.prod([d, f, f])
    return dict(dpre=d if mut == "dpre_mask_ignored" else A.where(valid, d, zero), s1=s1, s2=s2, given=given)


def _bn_bwd_slots(c):
    p = c["p"]
    return {k: slice(p["off"][k], p["off"][k] + p["C"]) for k in ("dgamma", "dbeta", "dbias") if k in c["bufs"]}


def emulate_bn_bwd(c, A, mut=None):
    """What a float32 kernel that evaluates the contract with arithmetic A leaves in every output buffer."""
    p, b = c["p"], c["bufs"]
    rows, C, off = p["rows"], p["C"], p["off"]
    with np.errstate(all="ignore"):
        r = compute_bn_bwd(c, A, mut)
        got = {o: b[o][0].copy() for o in c["outs"]}
        d32 = np.broadcast_to(A.out(r["dpre"]), (rows, C)).astype(np.float32)
        stored = store(d32, b["dpre"][1])
        got["dpre"][off["dpre"]:off["dpre"] + rows * C] = stored.reshape(-1)
        s1, s2 = np.asarray(A.out(r["s1"]), np.float32), np.asarray(A.out(r["s2"]), np.float32)
        if mut == "swapped":
            s1, s2 = s2, s1
        sb = F32(getattr(A, "order", 0)).colsum(d32 if mut == "dbias_unrounded" else stored, rows)
        for k, sl in _bn_bwd_slots(c).items():
            old = np.float32(0) if mut == "overwrite" else b[k][0][sl]
            got[k][sl] = old + dict(dgamma=s2, dbeta=s1, dbias=sb)[k]              # one fp32 add
    return got


def expect_bn_bwd(c):
    """dpre: bounded (exact in the exact cases).  dgamma / dbeta: exactly one fp32 add of the given sums (vector form), else
    bounded.  dbias: in the exact cases the exact sum of the stored dpre; otherwise check() holds it to the kernel's own
    stored dpre (the header's "summed on the rounded values") and expect() has no entry for it.  work: see check()."""
    p, b = c["p"], c["bufs"]
    rows, C, off = p["rows"], p["C"], p["off"]
    A = Exact() if c["exact"] else RunErr()
    r = compute_bn_bwd(c, A)
    res = {"work": (b["work"][0].astype(np.float64), None)}
    v, e = A.out(r["dpre"])
    val, err = b["dpre"][0].astype(np.float64), np.zeros(b["dpre"][0].shape)
    sl = slice(off["dpre"], off["dpre"] + rows * C)
    val[sl], err[sl] = np.broadcast_to(v, (rows, C)).reshape(-1), np.broadcast_to(e, (rows, C)).reshape(-1)
    res["dpre"] = (val, None if c["exact"] else err)
    stored = store(val[sl].astype(np.float32), b["dpre"][1]).astype(np.float64).reshape(rows, C)
    for k, sl in _bn_bwd_slots(c).items():
        val, err = b[k][0].astype(np.float64), np.zeros(b[k][0].shape)
        if k == "dbias":
            if not c["exact"]:
                continue
            assert_exact_sum(np.abs(stored).sum(0) + np.abs(val[sl]), quantum(np.concatenate([stored.reshape(-1), val[sl]])))
            val[sl] += stored.sum(0)
            res[k] = (val, None)
            continue
        s = r["s2"] if k == "dgamma" else r["s1"]
        if r["given"]:
            val[sl] += s[0]                       # two fp32 numbers: their float64 sum is exact, float32() of it the one add
            res[k] = (val, None)
        else:
            v, e = A.out(A.add(A.lift(val[sl]), s))
            val[sl], err[sl] = v, e
            res[k] = (val, None if c["exact"] else err)
    return res


def expect_colsum(c, mut=None):
    p = c["p"]
    rows, C, ld = p["rows"], p["C"], p["ld"]
    x = _f64(c, "x")
    Cr = C + 1 if mut == "pad_column" else C
    m = x[p["x_off"] + np.arange(rows)[:, None] * ld + np.arange(Cr)[None, :]]
    if mut == "pad_column":
        m = np.concatenate([m[:, :C - 1], m[:, C - 1:C] + m[:, C:]], 1)
    if mut == "drop_row":
        m = np.delete(m, min(rows - 1, 128), 0)
    out = _f64(c, "out")
    sl = slice(p["out_off"], p["out_off"] + C)
    old = np.zeros(C) if mut == "overwrite" else out[sl].copy()
    s = m.sum(0)
    if mut == "drop_tail":
        s[C - 1] = 0
    e = sum_expect(s, np.abs(m).sum(0) + np.abs(old), m.shape[0] + 1, c["exact"])
    out[sl] = old + s
    if e is None:
        return {"out": (out, None)}
    err = np.zeros_like(out)
    err[sl] = e
    return {"out": (out, err)}


def expect_l1_loss(c, mut=None):
    """loss_acc[0] += sum |pred - target| over all bins, loss_acc[1] += the same over bins < n_prio;
    dpred = sign(pred - target) * (fp32(w_all) + (bin < n_prio ? fp32(w_prio) : 0)): one fp32 add; sign(0) = 0."""
    p = c["p"]
    N, T, P, padl, F, ldp, n_prio = p["N"], p["T"], p["P"], p["padl"], p["F"], p["ldp"], p["n_prio"]
    if mut == "prio_plus":
        n_prio += 1
    if mut == "prio_minus":
        n_prio -= 1
    prow = (np.arange(N)[:, None] * P + padl + np.arange(T)[None, :]).reshape(-1)
    pred = c["bufs"]["pred"][0][MARGIN + prow[:, None] * ldp + np.arange(F)[None, :]]
    tgt = c["bufs"]["target"][0][MARGIN:MARGIN + N * T * F].reshape(N * T, F)
    d32 = pred - tgt                                          # fp32: one rounding per term
    d = pred.astype(np.float64) - tgt
    prio = np.arange(F) < n_prio
    res = {}
    acc = _f64(c, "loss_acc")
    o = p["acc_off"]
    ab = np.abs(d)
    s = np.array([ab.sum(), ab[:, prio].sum()])
    n = np.array([ab.size, N * T * int(prio.sum())], np.float64)
    old = acc[o:o + 2].copy()
    if c["exact"]:
        assert_exact_sum(s + np.abs(old), UNIT)
        err = None
    else:                                                     # n roundings of the terms + n adds (the prefill is a term)
        err = np.zeros_like(acc)
        err[o:o + 2] = U * s + n * U * (s + np.abs(old))
    acc[o:o + 2] = old + s
    res["loss_acc"] = (acc, err)
    if "dpred" in c["bufs"]:
        w = np.where(prio | (mut == "prio_all"), np.float32(p["w_all"]) + np.float32(p["w_prio"]), np.float32(p["w_all"]) + np.float32(0))
        sg = np.sign(d32).astype(np.float32)
        if mut == "sign0":
            sg = np.where(d32 >= 0, 1, -1).astype(np.float32)
        g = sg * w.astype(np.float32)[None, :]
        dp, ddt = c["bufs"]["dpred"]
        out = dp.copy()
        out[MARGIN + prow[:, None] * p["ldd"] + np.arange(F)[None, :]] = store(g, ddt)
        res["dpred"] = (out, None)
    return res


def expect_sumsq(c, mut=None):
    p = c["p"]
    x = _f64(c, "x")[MARGIN:MARGIN + p["n"]]
    out = _f64(c, "out")
    o = p["out_off"]
    old = out[o]
    s = float((x * x).sum())
    if c["exact"]:
        assert_exact_sum(s + abs(old), UNIT * UNIT)
        err = None
    else:
        err = np.zeros_like(out)
        err[o] = U * s + p["n"] * U * (s + abs(old))
    out[o] = (0.0 if mut == "overwrite" else old) + s
    return {"out": (out, err)}


def expect_segment_stats(c):
    """out[4 s + (0, 1, 2, 3)] = sum, sum of squares, min, max of x[offsets[s] : offsets[s + 1]]; an EMPTY segment gives
    0, 0, +inf, -inf (the identities of the four reductions).  min / max are exact always."""
    x = _f64(c, "x")[MARGIN:]
    offs = c["bufs"]["offsets"][0]
    out = _f64(c, "out")
    err = np.zeros_like(out)
    exact_words = np.zeros(out.shape, bool)
    for s in range(len(offs) - 1):
        seg = x[offs[s]:offs[s + 1]]
        n = len(seg)
        o = MARGIN + 4 * s
        sq = seg * seg
        out[o:o + 4] = [seg.sum(), sq.sum(), seg.min() if n else np.inf, seg.max() if n else -np.inf]
        if c["exact"]:
            assert_exact_sum(np.abs(seg).sum(), UNIT)
            assert_exact_sum(sq.sum(), UNIT * UNIT)
        else:
            err[o] = max(n - 1, 0) * U * np.abs(seg).sum()
            err[o + 1] = U * sq.sum() + max(n - 1, 0) * U * sq.sum()
    return {"out": (out, None if c["exact"] else err)}


def compute_adam(c, A, mut=None):
    """tf.clip_by_global_norm + tf.train.AdamOptimizer: g' = g * grad_scale * clip / max(sqrt(gnorm_sq) * grad_scale, clip)
    (the norm is that of the scaled gradient), m' = beta1 m + (1 - beta1) g', v' = beta2 v + (1 - beta2) g'^2,
    p' = p - lr_t m' / (sqrt(v') + eps)."""
    p, b = c["p"], c["bufs"]
    n = p["n"]
    get = lambda name: A.lift(b[name][0][MARGIN:MARGIN + n])
    f = lambda x: A.lift(np.float32(x))
    scale = f(p["grad_scale"])
    if "gnorm_sq" in b:
        gn = A.sqrt(A.lift(b["gnorm_sq"][0][MARGIN:MARGIN + 1]))
        if mut != "norm_unscaled":
            gn = A.mul(gn, f(p["grad_scale"]))
        den = gn if mut == "always_clip" else A.maximum(gn, f(p["clip"]))
        scale = A.mul(scale, A.div(f(p["clip"]), den))
    g = A.mul(get("g"), scale)
    b1, b2 = f(p["beta1"]), f(p["beta2"])
    one = f(1)
    m = A.dot2(b2 if mut == "beta2_for_m" else b1, get("m"), A.sub(one, b2 if mut == "beta2_for_m" else b1), g)
    v = A.add(A.mul(b2, get("v")), A.prod([A.sub(one, b2), g, g]))
    den = A.sqrt(A.add(v, f(p["eps"]))) if mut == "eps_inside" else A.add(A.sqrt(v), f(p["eps"]))
    w = A.muladd([A.neg(f(p["lr_t"])), A.div(m, den)], get("p"))
    return {"p": w, "m": m, "v": v}


def expect_adam(c):
    """A raised status word (p["raised"] is its slot): nothing is updated and skipped[0] = 1; otherwise skipped is left."""
    res = _whole(c, c["outs"])
    n = c["p"]["n"]
    if c["p"]["raised"] is not None:
        if "skipped" in res:
            res["skipped"][0][MARGIN] = 1.0
        return {o: (v, None) for o, (v, e) in res.items() if o != "shadow"}
    r = compute_adam(c, RunErr())
    for name in ("p", "m", "v"):
        v, e = RunErr().out(r[name])
        res[name][1] = np.zeros_like(res[name][0])
        res[name][0][MARGIN:MARGIN + n], res[name][1][MARGIN:MARGIN + n] = v, e
    return {o: (v, e if e is not None else np.zeros_like(v)) for o, (v, e) in res.items() if o != "shadow"}


def expect_cast2d(c, mut=None):
    """dst[r, c] (or dst[c, r] when transposed) = (T) src[r, c]; dst_hi / dst_lo = the pre-split pair of the same value."""
    p = c["p"]
    rows, cols = p["rows"], p["cols"]
    src = c["bufs"]["src"][0][p["src_off"] + np.arange(rows)[:, None] * p["ld_src"] + np.arange(cols)[None, :]]
    r, k = np.indices((rows, cols))
    idx = p["dst_off"] + (k * p["ld_dst"] + r if p["transpose"] else r * p["ld_dst"] + k)
    res = {}
    hi, lo = split_hi_lo(src, mut)
    for name, v in (("dst", src), ("dst_hi", hi), ("dst_lo", lo)):
        if name in c["bufs"]:
            buf, dt = c["bufs"][name]
            out = buf.copy()
            out[idx] = trunc_bf16(v) if (mut == "truncate" and dt == "bf16") else store(v, dt)
            res[name] = (out, None)
    return res


def expect_split(c, mut=None):
    n = c["p"]["n"]
    hi, lo = split_hi_lo(c["bufs"]["src"][0][MARGIN:MARGIN + n], mut)
    res = {}
    for name, v in (("hi", hi), ("lo", lo)):
        out = c["bufs"][name][0].copy()
        out[MARGIN:MARGIN + n] = v
        res[name] = (out, None)
    return res


def compute_gru_pointwise(c, A, mut=None):
    """The four element-wise pieces of tf.contrib.rnn.GRUCell around the gate products (see ns_gru_pointwise_params).
    -> {buffer: (A value [N, H], column offset in the buffer's rows, row stride, rows written)}."""
    p, b = c["p"], c["bufs"]
    N, H, t, mode = p["N"], p["H"], p["t"], p["mode"]

    def get(name, sn, col=0):
        idx = MARGIN + np.arange(N)[:, None] * sn + col + np.arange(H)[None, :]
        return A.lift(b[name][0][idx])
    lengths = b["lengths"][0] if "lengths" in b else None
    ln = lengths if lengths is not None else np.full(N, p["T"])
    masked = (t >= ln)[:, None] if lengths is not None else np.zeros((N, 1), bool)
    zero = A.lift(np.zeros((N, H), np.float32))
    one = A.lift(np.float32(1))
    hp = get("h_prev", p["hp_sn"]) if "h_prev" in b else zero
    if "h_init" in b:
        first = (t == ln - 1) if (p["reverse"] and mut != "init_at_zero") else np.full(N, t == 0)
        hp = A.where(first[:, None], get("h_init", p["hi_sn"]), hp)
    r = get("ru", p["ru_sn"]) if "ru" in b else zero
    u = get("ru", p["ru_sn"], H) if "ru" in b else zero
    everyrow = np.ones((N, 1), bool)
    if mode == 0:
        return {"out": (A.mul(r, hp), 0, p["out_sn"], everyrow)}
    if mode == 1:
        h = A.where(masked, zero, A.dot2(u, hp, A.sub(one, u), get("c", p["c_sn"])))
        res = {"out": (h, 0, p["out_sn"], everyrow)}
        if "out2" in b:
            res["out2"] = (h, 0, p["out2_sn"], everyrow)
        return res
    if mode == 2:
        cc = get("c", p["c_sn"])
        dh = get("dh", p["dh_sn"])
        if "dh_add" in b:
            dh = A.add(dh, get("dh_add", p["dha_sn"]))
        dh = A.where(masked, zero, dh)
        dzc = A.prod([dh, A.sub(one, u), A.muladd([A.neg(cc), cc], one)])
        dzu = A.prod([dh, A.sub(hp, cc), u, A.sub(one, u)])
        return {"out": (dzc, 0, p["out_sn"], everyrow), "dzg": (dzu, H, p["dzg_sn"], everyrow),
                "carry": (A.mul(dh, u), 0, p["carry_sn"], ~masked)}
    drh = A.where(masked, zero, get("dh", p["dh_sn"]))
    dzr = A.prod([drh, hp, r, A.sub(one, r)])
    carry = A.muladd([drh, r], get("carry", p["carry_sn"]))
    return {"dzg": (dzr, 0, p["dzg_sn"], everyrow), "carry": (carry, 0, p["carry_sn"], ~masked)}


def scatter_rows(c, r, A):
    """compute_gru_pointwise's result laid into copies of the case's buffers -> {buffer: (value, err or None)}."""
    N, H = c["p"]["N"], c["p"]["H"]
    res = {}
    for name, (a, col, sn, rows) in r.items():
        buf = c["bufs"][name][0]
        idx = MARGIN + np.arange(N)[:, None] * sn + col + np.arange(H)[None, :]
        sel = np.broadcast_to(rows, (N, H))
        if isinstance(A, RunErr):
            v, e = A.out(a)
            val, err = buf.astype(np.float64), np.zeros(buf.shape)
            val[idx[sel]], err[idx[sel]] = np.broadcast_to(v, (N, H))[sel], np.broadcast_to(e, (N, H))[sel]
            res[name] = (val, err)
        else:
            val = buf.copy()
            val[idx[sel]] = store(np.broadcast_to(A.out(a), (N, H))[sel], c["bufs"][name][1])
            res[name] = val
    return res


def expect_gru_pointwise(c):
    return scatter_rows(c, compute_gru_pointwise(c, RunErr()), RunErr())


def compute_highway(c, A, mut=None):
    """y = h t + x (1 - t); backward dhpre = dy t (h > 0), dtpre = dy (h - x) t (1 - t), dx = dy (1 - t)."""
    p, b = c["p"], c["bufs"]
    n = p["n"]
    get = lambda name: A.lift(b[name][0][MARGIN:MARGIN + n])
    h, t, x = get("h"), get("t"), get("x")
    one = A.lift(np.float32(1))
    if not p["backward"]:
        return {"y": A.dot2(h, t, x, A.sub(one, t))}
    dy = get("dy")
    pos = (A.value(h) >= 0) if mut == "relu_at_zero" else (A.value(h) > 0)
    return {"dhpre": A.where(pos, A.mul(dy, t), A.lift(np.zeros(n, np.float32))),
            "dtpre": A.prod([dy, A.sub(h, x), t, A.sub(one, t)]), "dx": A.mul(dy, A.sub(one, t))}


def compute_act_bwd(c, A, mut=None):
    """dpre = dy * act'(y) from the stored OUTPUT y: ReLU (y > 0), tanh 1 - y^2, sigmoid y (1 - y), softsign (1 - |y|)^2;
    0 in rows that fail the (period, lo, hi) test."""
    p, b = c["p"], c["bufs"]
    rows, C, act = p["rows"], p["C"], p["act"]
    get = lambda name: A.lift(b[name][0][MARGIN:MARGIN + rows * C].reshape(rows, C))
    dy, y = get("dy"), get("y")
    one = A.lift(np.float32(1))
    zero = A.lift(np.zeros((rows, C), np.float32))
    if act == ACT_RELU:
        d = A.where(A.value(y) > 0, dy, zero)
    elif act == ACT_TANH:
        d = A.mul(dy, A.muladd([A.neg(y), y], one))
    elif act == ACT_SIGMOID:
        d = A.prod([dy, y, A.sub(one, y)])
    elif act == ACT_SOFTSIGN:
        s = A.sub(one, A.abs(y))
        d = A.prod([dy, s, s])
    else:
        d = dy
    valid = row_valid(rows, None if mut == "mask_ignored" else p["row_mask"])[:, None]
    return {"dpre": A.where(valid, d, zero)}


def _flat_expect(c, r, n):
    res = {}
    for name, a in r.items():
        v, e = RunErr().out(a)
        val, err = c["bufs"][name][0].astype(np.float64), np.zeros(c["bufs"][name][0].shape)
        val[MARGIN:MARGIN + n], err[MARGIN:MARGIN + n] = v.reshape(-1), e.reshape(-1)
        res[name] = (val, err)
    return res


def flat_emulate(c, r, n, A):
    res = {}
    for name, a in r.items():
        val = c["bufs"][name][0].copy()
        val[MARGIN:MARGIN + n] = store(A.out(a).reshape(-1), c["bufs"][name][1])
        res[name] = val
    return res


def expect_highway(c):
    return _flat_expect(c, compute_highway(c, RunErr()), c["p"]["n"])


def expect_act_bwd(c):
    return _flat_expect(c, compute_act_bwd(c, RunErr()), c["p"]["rows"] * c["p"]["C"])


def expect_zero(c):
    """Every listed range [start, start + n) of the buffer reads +0.0; nothing else changes."""
    out = c["bufs"]["buf"][0].copy()
    for start, n in c["p"]["ranges"]:
        out[start:start + n] = 0.0
    return {"buf": (out, None)}


EXPECT = dict(copy3d=expect_copy3d, embedding_fwd=expect_embedding_fwd, embedding_bwd=expect_embedding_bwd,
              bn_fwd=expect_bn_fwd, colsum=expect_colsum, l1_loss=expect_l1_loss, sumsq=expect_sumsq,
              segment_stats=expect_segment_stats, adam=expect_adam, cast2d=expect_cast2d, split_hi_lo=expect_split,
              gru_pointwise=expect_gru_pointwise, highway=expect_highway, act_bwd=expect_act_bwd, zero=expect_zero,
              bn_bwd=expect_bn_bwd)


def expect(c):
    return EXPECT[c["op"]](c)


# ------------------------------------------------------------------------------------------------------ cases
# The inputs of tests/test_pointwise_contract_gpu.py, built here so that the CPU module can show the references, the
# exactness conditions and the mutants on exactly them.  Which kernel body a case takes is said in the GPU module.
def case(op, name, p, bufs, outs, exact=False):
    return dict(op=op, name=name, p=p, bufs=bufs, outs=list(outs), exact=exact)


def _vals(n, seed, dt, kind="round"):
    if kind == "round":
        return rounding_values(n, seed, dt == "bf16")
    x = np.random.RandomState(seed).randn(n).astype(np.float32)
    return rne_bf16(x) if dt == "bf16" else x


def copy3d_cases():
    out = []

    def one(name, I, J, Cc, ss, ds, sdt, ddt, acc, so=0, do=0, seed=1):
        ns = so + max(1, (I - 1) * ss[0] + (J - 1) * ss[1] + Cc)
        nd = do + (I - 1) * ds[0] + (J - 1) * ds[1] + Cc + 2
        dst = _vals(nd, seed + 1, ddt) if acc else np.full(nd, SENT, np.float32)
        out.append(case("copy3d", name, dict(I=I, J=J, Cc=Cc, src_strides=ss, dst_strides=ds, src_off=MARGIN + so,
                                             dst_off=MARGIN + do, accumulate=acc),
                        dict(src=(framed(_vals(ns, seed, sdt)), sdt), dst=(framed(dst), ddt)), ["dst"]))
    one("1x1x1", 1, 1, 1, (1, 1), (1, 1), "f32", "f32", 0)
    for sdt in ("f32", "bf16"):
        for ddt in ("f32", "bf16"):
            for acc in (0, 1):
                one("3x5x7-%s-%s-acc%d" % (sdt, ddt, acc), 3, 5, 7, (42, 8), (50, 9), sdt, ddt, acc, 1, 2, seed=3 + acc)
    one("1x300x129-broadcast-f32-bf16", 1, 300, 129, (0, 0), (300 * 129, 129), "f32", "bf16", 0, seed=5)
    one("1x300x129-broadcast-bf16-f32-acc", 1, 300, 129, (0, 0), (300 * 129, 129), "bf16", "f32", 1, seed=6)
    n = 4096 * 256 + 3
    one("second-trip-acc", 1, 1, n, (n, n), (n, n), "f32", "f32", 1, seed=7)
    one("second-trip-bf16", 1, 1, n, (n, n), (n, n), "f32", "bf16", 0, seed=8)
    return out


EMB_SHAPES = {"speaker": (1, 1, 1, 0, 4, 5), "ragged": (3, 300, 305, 2, 260, 5), "one-id": (1, 300, 300, 0, 1024, 5)}


def _emb_ids(key):
    N, T, P, padl, D, V = EMB_SHAPES[key]
    if key == "one-id":
        return np.full(N * T, 2, np.int32)
    ids = np.random.RandomState(11).randint(0, V, N * T).astype(np.int32)
    ids[0] = -1 if key == "ragged" else 3
    if key == "ragged":
        ids[[1, 255, 256, 299, 300, N * T - 1]] = [V + 3, 4, 0, -1, V + 3, 1]
    return ids


def embedding_fwd_cases():
    out = []
    for key, dts in (("speaker", ("f32",)), ("ragged", ("f32", "bf16")), ("one-id", ("f32", "bf16"))):
        N, T, P, padl, D, V = EMB_SHAPES[key]
        for dt in dts:
            toff = 4 if key == "ragged" else 0
            table = np.concatenate([np.full(toff, SENT, np.float32), rounding_values(V * D, 12)])
            out.append(case("embedding_fwd", "%s-%s" % (key, dt),
                            dict(N=N, T=T, P=P, padl=padl, D=D, V=V, table_off=MARGIN + toff),
                            dict(ids=(_emb_ids(key), "i32"), table=(framed(table), "f32"),
                                 out=(framed(np.full(N * P * D, SENT)), dt)), ["out"]))
    return out


def embedding_bwd_cases():
    out = []
    for key in EMB_SHAPES:
        N, T, P, padl, D, V = EMB_SHAPES[key]
        for exact in (True, False):
            if not exact and key != "ragged":
                continue
            toff = 4 if key == "ragged" else 0
            dout = unit_values(N * P * D, 13) if exact else np.random.RandomState(14).randn(N * P * D).astype(np.float32)
            tab = unit_values(toff + V * D, 15)            # the += output is prefilled; pad rows of dout carry values too
            out.append(case("embedding_bwd", "%s-%s" % (key, "exact" if exact else "random"),
                            dict(N=N, T=T, P=P, padl=padl, D=D, V=V, dtable_off=MARGIN + toff),
                            dict(ids=(_emb_ids(key), "i32"), dout=(framed(dout), "f32"), dtable=(framed(tab), "f32")),
                            ["dtable"], exact))
    return out


def probes(base, buf, positions, value=1.0, zero=True):
    """One-hot probes: the case `base` with buffer `buf` all zero (between its margins) but `value` at one flat index of
    the buffer - one case per position.  The expectation is exact."""
    out = []
    for name, pos in positions:
        c = dict(base, name="%s-probe-%s" % (base["name"], name), exact=True, bufs=dict(base["bufs"]))
        x = base["bufs"][buf][0].copy()
        if zero:
            x[MARGIN:-MARGIN] = 0.0
        x[pos] = value if zero else x[pos] + value
        c["bufs"][buf] = (x, base["bufs"][buf][1])
        out.append(c)
    return out


def embedding_bwd_probes():
    base = [c for c in embedding_bwd_cases() if c["name"] == "ragged-exact"][0]
    N, T, P, padl, D, V = EMB_SHAPES["ragged"]
    at = lambda n, t, d: MARGIN + (n * P + padl + t) * D + d
    pos = [("first", at(0, 0, 0)), ("last", at(2, 299, 259)), ("chunk-255", at(0, 255, 7)), ("chunk-256", at(0, 256, 7)),
           ("col-255", at(1, 5, 255)), ("col-256", at(1, 5, 256)), ("pad-before", at(1, -1, 0)), ("pad-behind", at(0, T, 0))]
    return probes(base, "dout", pos)


def bn_fwd_cases():
    out = []

    def one(name, rows, C, dt, training=1, mask=None, ld_y=0, y_shift=0, with_y=True, pair=False, moving=True,
            stats_final=False, seed=20):
        rng = np.random.RandomState(seed)
        z = (rng.randn(rows, C) * 2 + 0.5).astype(np.float32)
        z = rne_bf16(z) if dt == "bf16" else z
        valid = row_valid(rows, mask)
        count = float(max(1, valid.sum()))
        z64 = z.astype(np.float64) * valid[:, None]
        cs, cq = z64.sum(0).astype(np.float32), (z64 * z64).sum(0).astype(np.float32)
        if training and C > 2 and dt == "f32":    # a column whose sumsq / count - mean^2 is negative in fp32 and in float64
            cs[2], cq[2] = np.float32(count), np.float32(count * (1 - 2.0 ** -12))
        f = lambda x: (framed(x), "f32")
        bufs = dict(z=(framed(z), dt), gamma=f(1 + 0.3 * rng.randn(C)), beta=f(0.2 * rng.randn(C)))
        outs = []
        if stats_final:
            bufs["mean_out"], bufs["istd_out"] = f(rng.randn(C) * 0.3), f(0.5 + rng.rand(C))
        else:
            bufs["mean_out"], bufs["istd_out"] = f(np.full(C, SENT)), f(np.full(C, SENT))
            outs += ["mean_out", "istd_out"]
            if training:
                bufs["col_sum"], bufs["col_sumsq"] = f(cs), f(cq)
            if moving or not training:
                bufs["moving_mean"], bufs["moving_var"] = f(rng.randn(C) * 0.5), f(0.5 + rng.rand(C))
                if training:
                    outs += ["moving_mean", "moving_var"]
        if with_y:
            bufs["y"] = (framed(np.full(y_shift + rows * (ld_y or C), SENT)), dt)
            outs.append("y")
        if pair:
            bufs["y_hi"], bufs["y_lo"] = (framed(np.full(rows * C, SENT)), "bf16"), (framed(np.full(rows * C, SENT)), "bf16")
            outs += ["y_hi", "y_lo"]
        out.append(case("bn_fwd", name, dict(rows=rows, C=C, count=count, eps=1e-3, momentum=0.99, training=training,
                                             row_mask=mask, y_off=MARGIN + y_shift, ld_y=ld_y, stats_final=stats_final,
                                             dtype=dt), bufs, outs))
    one("scalar-C6-train-mask", 70, 6, "f32", mask=(10, 2, 9))
    one("scalar-C6-bf16", 70, 6, "bf16", seed=21)
    one("scalar-C8-misaligned-y", 70, 8, "f32", y_shift=1, seed=22)
    one("scalar-C6-ld", 70, 6, "f32", ld_y=9, seed=23)
    one("vector-C8-rows1-infer", 1, 8, "f32", training=0, seed=24)
    one("vector-C8-rows1-train", 1, 8, "f32", moving=False, seed=25)
    one("vector-C132-ld-pair", 70, 132, "f32", ld_y=136, pair=True, mask=(7, 1, 6), seed=26)
    one("vector-C132-bf16", 70, 132, "bf16", ld_y=136, seed=27)
    one("vector-C8-pair-only", 70, 8, "f32", with_y=False, pair=True, seed=28)
    one("vector-C132-stats-final", 70, 132, "f32", stats_final=True, seed=29)
    one("scalar-C6-stats-final-infer", 70, 6, "bf16", training=0, stats_final=True, seed=30)
    one("vector-second-trip", (4096 * 256 * 4 + 8) // 8, 8, "f32", seed=31)
    return out


def colsum_cases(random=False):
    out = []
    shapes = [("vector", 1, 4, 4, 0), ("vector", 129, 64, 64, 0), ("vector-ragged", 300, 66, 68, 0),
              ("vector-64-blocks", 8193, 130, 132, 0), ("column", 300, 37, 37, 0), ("column", 70, 257, 259, 0),
              ("column-empty-blocks", 5, 37, 37, 0), ("column-shifted", 129, 64, 64, 1)]
    for form, rows, C, ld, shift in shapes:
        for dt in ("f32", "bf16"):
            for work in (True, False):
                if random and (dt == "bf16" or not work) and rows != 300:
                    continue
                x = np.full((rows, ld), SENT, np.float32)            # the padding behind a row holds the sentinel
                x[:, :C] = (np.random.RandomState(40).randn(rows, C) if random else unit_values((rows, C), 40))
                x = np.concatenate([np.full(shift, SENT, np.float32), rne_bf16(x.reshape(-1)) if dt == "bf16" else x.reshape(-1)])
                name = "%s-%dx%d-ld%d-%s-%s%s" % (form, rows, C, ld, dt, "work" if work else "atomic", "-random" if random else "")
                out.append(case("colsum", name, dict(rows=rows, C=C, ld=ld, x_off=MARGIN + shift, out_off=MARGIN, work=work, dtype=dt),
                                dict(x=(framed(x), dt), out=(framed(unit_values(C, 41)), "f32")), ["out"], not random))
    return out


def colsum_probes():
    """(8193, 130, 132), vector form: 64 row blocks of 129 rows, 3 blocks of 64 columns, the last quad ragged (columns
    128, 129 valid; 130, 131 padding).  (300, 37, 37), per-column form: 64 row blocks of 5 rows."""
    out = []
    for base in colsum_cases():
        if base["name"] in ("vector-64-blocks-8193x130-ld132-f32-work", "vector-64-blocks-8193x130-ld132-bf16-atomic"):
            at = lambda r, k: MARGIN + r * 132 + k
            pos = [("first", at(0, 0)), ("last", at(8192, 129)), ("quad-3", at(17, 3)), ("quad-4", at(17, 4)),
                   ("colblock-63", at(128, 63)), ("colblock-64", at(129, 64)), ("rowblock-128", at(128, 5)),
                   ("rowblock-129", at(129, 5)), ("tail-128", at(8191, 128)), ("padding-130", at(200, 130)),
                   ("padding-131", at(8192, 131))]
            out += probes(base, "x", pos)
        if base["name"] == "column-300x37-ld37-f32-work":
            at = lambda r, k: MARGIN + r * 37 + k
            out += probes(base, "x", [("first", at(0, 0)), ("last", at(299, 36)), ("rowblock-4", at(4, 36)), ("rowblock-5", at(5, 0))])
    return out


L1_SHAPES = [  # name, N, T, P, padl, F, ldp, ldd, n_prio, dpred dtype (None: absent), acc shift
    ("wide-quad-257", 1, 7, 12, 3, 257, 260, 260, 5, "f32", 0),
    ("wide-quad-259", 1, 1, 1, 0, 259, 260, 264, 259, "bf16", 2),
    ("wide-quad-1029-rows2050", 2, 1025, 1025, 0, 1029, 1032, 1032, 5, "f32", 0),
    ("wide-quad-1029-nograd", 1, 7, 7, 0, 1029, 1032, 0, 0, None, 0),
    ("wide-scalar-1025", 1, 7, 12, 3, 1025, 1025, 1025, 5, "f32", 2),
    ("wide-scalar-1025-bf16", 7, 1, 4, 3, 1025, 1025, 1028, 1025, "bf16", 0),
    ("narrow-quad-80-rows3400", 4, 850, 853, 3, 80, 80, 80, 5, "f32", 0),
    ("narrow-quad-80-nograd", 1, 7, 7, 0, 80, 84, 0, 80, None, 2),
    ("narrow-flat-78", 1, 7, 12, 3, 78, 80, 80, 5, "f32", 0),
    ("narrow-flat-78-rows1", 1, 1, 1, 0, 78, 78, 78, 0, "bf16", 0),
    ("narrow-flat-80-bf16", 4, 850, 853, 3, 80, 80, 80, 5, "bf16", 2)]


def l1_loss_cases(random=False):
    out = []
    for name, N, T, P, padl, F, ldp, ldd, n_prio, ddt, shift in L1_SHAPES:
        if random and "rows" in name:
            continue
        rng = np.random.RandomState(50)
        if random:
            pred, tgt = rng.randn(N * P * ldp).astype(np.float32), rng.randn(N * T, F).astype(np.float32)
        else:
            pred, tgt = unit_values(N * P * ldp, 51), unit_values((N * T, F), 52)      # pad rows carry values as well
        prow = (np.arange(N)[:, None] * P + padl + np.arange(T)[None, :]).reshape(-1)
        same = rng.rand(N * T, F) < 0.1                                               # pred == target: sign(0) = 0
        same[0, [0, F - 1]] = True
        tgt = np.where(same, pred[prow[:, None] * ldp + np.arange(F)[None, :]], tgt).astype(np.float32)
        bufs = dict(pred=(framed(pred), "f32"), target=(framed(tgt), "f32"),
                    loss_acc=(framed([3.25, -1.5, 2.0, 0.75]), "f32"))
        outs = ["loss_acc"]
        if ddt:
            bufs["dpred"] = (framed(np.full(N * P * ldd, SENT)), ddt)
            outs.append("dpred")
        out.append(case("l1_loss", name + ("-random" if random else ""),
                        dict(N=N, T=T, P=P, padl=padl, F=F, ldp=ldp, ldd=ldd, n_prio=n_prio, w_all=0.5 / (N * T * F),
                             w_prio=0.5 / (N * T * max(1, n_prio)), acc_off=MARGIN + shift), bufs, outs, not random))
    return out


def l1_loss_probes():
    """One differing element (pred - target = 1 there, equal everywhere else) at the boundaries of each body."""
    out = []
    want = {"wide-quad-1029-rows2050": [(0, 0), (0, 4), (0, 5), (0, 1023), (0, 1024), (0, 1027), (0, 1028), (2047, 3),
                                        (2048, 3), (2049, 1028)],
            "wide-scalar-1025": [(0, 0), (0, 511), (0, 512), (0, 1024), (6, 1024), (3, 5), (4, 4)],
            "narrow-quad-80-rows3400": [(0, 0), (0, 3), (0, 4), (0, 5), (0, 79), (3276, 63), (3276, 64), (3399, 79)],
            "narrow-flat-78": [(0, 0), (0, 4), (0, 5), (0, 77), (6, 77)]}
    for base in l1_loss_cases():
        if base["name"] not in want:
            continue
        p = base["p"]
        b = dict(base, bufs=dict(base["bufs"]))
        prow = (np.arange(p["N"])[:, None] * p["P"] + p["padl"] + np.arange(p["T"])[None, :]).reshape(-1)
        tgt = base["bufs"]["pred"][0][MARGIN + prow[:, None] * p["ldp"] + np.arange(p["F"])[None, :]]
        b["bufs"]["target"] = (framed(tgt), "f32")
        pos = [("r%d-f%d" % (r, f), MARGIN + r * p["F"] + f) for r, f in want[base["name"]]]
        out += probes(b, "target", pos, value=-1.0, zero=False)
    return out


SUMSQ_N = (1, 3, 4, 5, 1027, 9001, 600001, 4200003)


def sumsq_cases(random=False):
    out = []
    for n in SUMSQ_N:
        for work in (True, False):
            if random and n not in (1027, 600001):
                continue
            x = np.random.RandomState(60).randn(n).astype(np.float32) if random else unit_values(n, 60, 1 if n > 10 ** 6 else 2)
            out.append(case("sumsq", "n%d-%s%s" % (n, "work" if work else "atomic", "-random" if random else ""),
                            dict(n=n, out_off=MARGIN + 1, work=work),
                            dict(x=(framed(x), "f32"), out=(framed([0.5, 2.75]), "f32")), ["out"], not random))
    return out


def sumsq_probes():
    """n = 4 200 003: 512 blocks x 256 threads x 8 quads = 1 048 576 quads per trip (second trip from quad 1 048 576), the
    three tail elements behind the last whole quad."""
    base = [c for c in sumsq_cases() if c["name"] == "n4200003-work"][0]
    n = 4200003
    pos = [("first", 0), ("quad-3", 3), ("quad-4", 4), ("block-1023", 1023), ("block-1024", 1024),
           ("stride-end", 4 * 131072 - 1), ("stride-next", 4 * 131072), ("trip-end", 4 * 1048576 - 1),
           ("trip-next", 4 * 1048576), ("tail-first", n - 3), ("last", n - 1)]
    return probes(base, "x", [(k, MARGIN + i) for k, i in pos], value=0.5)


SEG_OFFSETS = np.array([3, 3, 4, 1027, 2051, 3076, 8076], np.int64)      # lengths 0, 1, 1023, 1024, 1025, 5000


def segment_stats_cases():
    out = []
    nseg = len(SEG_OFFSETS) - 1
    for random in (False, True):
        x = np.random.RandomState(70).randn(8080).astype(np.float32) if random else unit_values(8080, 70)
        out.append(case("segment_stats", "random" if random else "exact", dict(nseg=nseg),
                        dict(x=(np.concatenate([np.full(MARGIN, SENT, np.float32), x]), "f32"), offsets=(SEG_OFFSETS, "i64"),
                             out=(framed(np.full(4 * nseg, SENT)), "f32")), ["out"], not random))
    base = dict(out[0], bufs=dict(out[0]["bufs"]))
    base["bufs"]["x"] = (np.concatenate([out[0]["bufs"]["x"][0], np.full(MARGIN, SENT, np.float32)]), "f32")
    pos = [("outside-before", 2), ("seg1", 3), ("seg2-first", 4), ("seg2-last", 1026), ("seg3-first", 1027), ("seg4-last", 3075),
           ("seg5-1024", 3076 + 1024), ("last", 8075), ("outside-behind", 8076)]
    out += probes(base, "x", [(k, MARGIN + i) for k, i in pos])
    for c in out[2:]:
        c["bufs"]["x"] = (c["bufs"]["x"][0][:-MARGIN], "f32")
    return out


def adam_cases():
    out = []

    def one(name, n, norm=None, grad_scale=1.0, shadow=True, status_n=0, raised=None, seed=80):
        rng = np.random.RandomState(seed)
        g = (rng.randn(n) * 10.0 ** rng.uniform(-4, 1, n)).astype(np.float32)           # five decades of gradient
        v = ((rng.randn(n) * 1e-2) ** 2 * rng.rand(n)).astype(np.float32)
        if n > 3:
            g[[1, n - 2]], v[[1, n - 2]] = 0.0, 0.0                                      # g = 0 with v = 0
        f = lambda x: (framed(x), "f32")
        bufs = dict(p=f(rng.randn(n)), g=f(g), m=f(rng.randn(n) * 1e-2), v=f(v), skipped=f([0.5]))
        outs = ["p", "m", "v", "skipped"]
        if norm is not None:
            bufs["gnorm_sq"] = f([norm])
        if shadow:
            bufs["shadow"] = (framed(np.full(n, SENT)), "bf16")
            outs.append("shadow")
        out.append(case("adam", name, dict(n=n, clip=1.0, grad_scale=grad_scale, lr_t=1e-3 * 0.7, beta1=0.9, beta2=0.999,
                                           eps=1e-8, status_n=status_n, raised=raised), bufs, outs))
    one("n1-no-norm", 1)
    one("n255-below-clip", 255, norm=0.25, status_n=12)
    one("n255-scaled-below-clip", 255, norm=2.25, grad_scale=0.5, shadow=False, seed=81)      # 1.5 * 0.5 < clip
    one("n257-above-clip", 257, norm=37.7, grad_scale=1.0 / 3, seed=82)
    one("second-trip", 4096 * 256 + 3, norm=37.7, grad_scale=0.5, status_n=12, seed=83)
    for slot in (0, 5, 11):
        one("n257-raised-%d" % slot, 257, norm=37.7, status_n=12, raised=slot, seed=84)
    for slot in (12, 31):          # the first slot past the twelve of version 107 and the last of NS_ADAM_STATUS_MAX = 32
        one("n257-raised-%d" % slot, 257, norm=37.7, status_n=32, raised=slot, seed=84)
    return out


CAST_SHAPES = [("scalar", 5, 7, 9, 11), ("scalar", 33, 65, 65, 67), ("vector", 64, 64, 64, 64), ("vector-edge", 68, 132, 136, 140)]


def cast2d_case(form, rows, cols, ld_src, ld_w, transpose, ddt, pair, with_dst=True, seed=90):
    ld_dst = (ld_w - cols + rows) if transpose else ld_w
    if form.startswith("vector"):
        ld_dst = (ld_dst + 3) // 4 * 4
    nd = (cols if transpose else rows) * ld_dst
    bufs = dict(src=(framed(rounding_values(rows * ld_src, seed)), "f32"))
    outs = []
    if with_dst:
        bufs["dst"] = (framed(np.full(nd, SENT)), ddt)
        outs.append("dst")
    if pair:
        bufs["dst_hi"], bufs["dst_lo"] = (framed(np.full(nd, SENT)), "bf16"), (framed(np.full(nd, SENT)), "bf16")
        outs += ["dst_hi", "dst_lo"]
    name = "%s-%dx%d-%s-%s%s%s" % (form, rows, cols, "T" if transpose else "N", ddt, "-pair" if pair else "", "" if with_dst else "-only")
    return case("cast2d", name, dict(rows=rows, cols=cols, ld_src=ld_src, ld_dst=ld_dst, transpose=transpose,
                                     src_off=MARGIN, dst_off=MARGIN), bufs, outs)


def cast2d_cases():
    out = []
    for form, rows, cols, ld_src, ld_w in CAST_SHAPES:
        for transpose in (0, 1):
            for ddt in ("f32", "bf16"):
                out.append(cast2d_case(form, rows, cols, ld_src, ld_w, transpose, ddt, ddt == "f32" and rows > 5))
            out.append(cast2d_case(form, rows, cols, ld_src, ld_w, transpose, "f32", True, with_dst=False, seed=91))
    return out


def cast_batch_cases():
    """Five descriptors of one CastBatch launch: mixed orientation, dtype and size, a 4 x 4 one among them."""
    spec = [(4, 4, 4, 4, 1, "bf16", False), (64, 64, 64, 64, 0, "f32", True), (68, 132, 136, 140, 1, "bf16", False),
            (128, 8, 8, 8, 1, "f32", False), (12, 200, 200, 204, 0, "bf16", True)]
    return [cast2d_case("vector", r, k, ls, lw, t, dt, pair, seed=92 + i) for i, (r, k, ls, lw, t, dt, pair) in enumerate(spec)]


def split_cases():
    return [case("split_hi_lo", "n%d" % n, dict(n=n),
                 dict(src=(framed(rounding_values(n, 95)), "f32"), hi=(framed(np.full(n, SENT)), "bf16"),
                      lo=(framed(np.full(n, SENT)), "bf16")), ["hi", "lo"]) for n in (1, 255, 4096 * 256 + 1)]


def gru_pointwise_cases():
    out = []
    for N, H in ((3, 128), (33, 256)):
        for dt in ("f32", "bf16"):
            for mode in range(4):
                for variant in ("plain", "lengths", "init-fwd", "init-rev", "wide"):
                    if N == 33 and variant not in ("lengths", "init-rev"):
                        continue
                    rng = np.random.RandomState(100 + mode)
                    w = 8 if variant == "wide" else 0
                    t, T = (0 if variant == "init-fwd" else 4), 9
                    sig = lambda x: (1 / (1 + np.exp(-x))).astype(np.float32)
                    cast = lambda x: rne_bf16(np.asarray(x, np.float32)) if dt == "bf16" else np.asarray(x, np.float32)
                    f = lambda x, d="f32": (framed(x), d)
                    p = dict(mode=mode, N=N, H=H, t=t, T=T, reverse=variant == "init-rev", dtype=dt, ru_sn=2 * H + w, c_sn=H + w,
                             hp_sn=H + w, out_sn=H + w, out2_sn=H + 2 * w, dzg_sn=2 * H + w, dh_sn=H + w, carry_sn=H + w,
                             dha_sn=H + w, hi_sn=H + w)
                    bufs = dict(ru=f(sig(rng.randn(N * p["ru_sn"]))), h_prev=f(cast(rng.randn(N * p["hp_sn"]) * 0.5), dt))
                    outs = []
                    if variant != "plain":       # rows at (the reverse direction's first step), before and past their length
                        bufs["lengths"] = (np.resize(np.array([t + 1, t, t + 3], np.int32), N), "i32")
                    if variant in ("init-fwd", "init-rev", "wide"):
                        bufs["h_init"] = f(rng.randn(N * p["hi_sn"]) * 0.5)
                    if mode in (1, 2):
                        bufs["c"] = f(np.tanh(rng.randn(N * p["c_sn"])))
                    if mode in (0, 1, 2):
                        bufs["out"] = f(np.full(N * p["out_sn"], SENT), dt)
                        outs.append("out")
                    if mode == 1 and variant in ("wide", "lengths"):
                        bufs["out2"] = f(np.full(N * p["out2_sn"], SENT), dt)
                        outs.append("out2")
                    if mode in (2, 3):
                        bufs["dzg"], bufs["dh"] = f(np.full(N * p["dzg_sn"], SENT), dt), f(rng.randn(N * p["dh_sn"]))
                        bufs["carry"] = f(rng.randn(N * p["carry_sn"]))
                        outs += ["dzg", "carry"]
                    if mode == 2 and variant in ("wide", "lengths"):
                        bufs["dh_add"] = f(rng.randn(N * p["dha_sn"]))
                    out.append(case("gru_pointwise", "N%d-H%d-%s-mode%d-%s" % (N, H, dt, mode, variant), p, bufs, outs))
    return out


POINT_N = (1, 257, 4096 * 256 + 5)


def highway_cases():
    out = []
    for n in POINT_N:
        for dt in ("f32", "bf16"):
            for backward in (0, 1):
                rng = np.random.RandomState(110 + backward)
                cast = lambda x: rne_bf16(np.asarray(x, np.float32)) if dt == "bf16" else np.asarray(x, np.float32)
                h = np.maximum(rng.randn(n), 0) * (rng.rand(n) < 0.8)
                h[0] = 0.0 if n > 1 else 0.75                                           # h = 0 exactly: the ReLU edge
                bufs = dict(h=(framed(cast(h)), dt), t=(framed(cast(1 / (1 + np.exp(-rng.randn(n))))), dt),
                            x=(framed(cast(rng.randn(n))), dt))
                if backward:
                    bufs.update(dy=(framed(rng.randn(n)), "f32"), dhpre=(framed(np.full(n, SENT)), dt),
                                dtpre=(framed(np.full(n, SENT)), dt), dx=(framed(np.full(n, SENT)), "f32"))
                    outs = ["dhpre", "dtpre", "dx"]
                else:
                    bufs["y"] = (framed(np.full(n, SENT)), dt)
                    outs = ["y"]
                out.append(case("highway", "n%d-%s-%s" % (n, dt, "bwd" if backward else "fwd"), dict(n=n, backward=backward, dtype=dt),
                                bufs, outs))
    return out


def act_bwd_cases():
    out = []
    for rows, C in ((1, 1), (1, 257), (257, 1), (349527, 3)):               # 1, 257, 257 and 4096 * 256 + 5 elements
        for dt in ("f32", "bf16"):
            for act in range(5):
                if rows > 1000 and act not in (ACT_RELU, ACT_TANH):
                    continue
                rng = np.random.RandomState(120 + act)
                n = rows * C
                y = rng.randn(n)
                y = {ACT_RELU: np.maximum(y, 0), ACT_TANH: np.tanh(y), ACT_SIGMOID: 1 / (1 + np.exp(-y)),
                     ACT_SOFTSIGN: y / (1 + np.abs(y))}.get(act, y).astype(np.float32)
                if n > 1:
                    y[n // 2] = 0.0
                y = rne_bf16(y) if dt == "bf16" else y
                mask = (5, 1, 4) if rows > 1 else None
                out.append(case("act_bwd", "%dx%d-%s-act%d" % (rows, C, dt, act), dict(rows=rows, C=C, act=act, row_mask=mask, dtype=dt),
                                dict(dy=(framed(rng.randn(n)), "f32"), y=(framed(y), dt), dpre=(framed(np.full(n, SENT)), dt)),
                                ["dpre"]))
    return out


def _bn_bwd_case(name, rows, C, act, dt="f32", ddt=None, mask=None, sums=None, ld=0, col0=0, shift=None, null=(),
                 no_finalize=False, exact=False, count=None, wrong_sums=False, seed=140):
    """The name's prefix says which kernels the case must reach (asserted against bn_bwd_form).  shift: the one operand
    that starts one element off alignment.  Masked rows of dy and z hold 1e30, the columns of a wide dy outside the block
    NaN, `work` is 200 * C NaNs between sentinels (the guard tail behind it must survive), the gradients are prefilled."""
    form, ddt = name.split("-")[0], ddt or dt
    sums = (form == "vector") if sums is None else sums
    rng = np.random.RandomState(seed)
    valid = row_valid(rows, mask)
    nv = int(valid.sum())
    if exact:
        assert count or (nv & (nv - 1)) == 0, "the mask makes the count a power of two"
        half = lambda *shape: (rng.randint(-2, 3, shape) * 0.5).astype(np.float32)
        z, dy, mean = half(rows, C), half(rows, C), half(C)
        istd = (2.0 ** rng.randint(-1, 2, C)).astype(np.float32)
        gamma = (2.0 ** rng.randint(-1, 2, C) * (2 * rng.randint(0, 2, C) - 1)).astype(np.float32)
        grad = lambda: unit_values(C, rng.randint(1 << 20))
    else:
        x = rng.randn(rows, C)
        z = {ACT_RELU: np.maximum(x, 0), ACT_TANH: np.tanh(x), ACT_SIGMOID: 1 / (1 + np.exp(-x)),
             ACT_SOFTSIGN: x / (1 + np.abs(x))}.get(act, x).astype(np.float32)
        tiny = np.float32(2.0 ** -126)                  # the smallest positive normal of fp32 and of bf16 alike
        special = {ACT_RELU: [0, tiny, 0, tiny], ACT_TANH: [1, -1, 0], ACT_SIGMOID: [0, 1, 1], ACT_SOFTSIGN: [1, -1]}.get(act, [])
        vr = np.flatnonzero(valid)
        for i, v in enumerate(special):
            z[vr[i % len(vr)], (3 * i + 1) % C] = v
        z = rne_bf16(z) if dt == "bf16" else z
        dy = rng.randn(rows, C).astype(np.float32)
        mean = (z[valid].mean(0) + 0.1 * rng.randn(C)).astype(np.float32)
        istd, gamma = (0.5 + rng.rand(C)).astype(np.float32), (1 + 0.3 * rng.randn(C)).astype(np.float32)
        grad = lambda: rng.randn(C).astype(np.float32)
    xhat = (z.astype(np.float64) - mean) * istd
    s1, s2 = (dy * valid[:, None]).sum(0, dtype=np.float64), (dy * xhat * valid[:, None]).sum(0)
    if wrong_sums:
        s1, s2 = rng.randn(C), rng.randn(C)
    z[~valid] = rne_bf16(np.float32(1e30))
    dy[~valid] = 1e30
    if ld:
        wide = np.full((rows, ld), np.nan, np.float32)
        wide[:, col0:col0 + C] = dy
        dy = wide
    off, bufs = {}, {}

    def put(k, x, d="f32"):
        sh = 1 if shift == k else 0
        bufs[k] = (framed(np.concatenate([np.full(sh, SENT, np.float32), np.asarray(x, np.float32).reshape(-1)])), d)
        off[k] = MARGIN + sh + (col0 if k == "dy" else 0)
    put("dy", dy), put("z", z, dt), put("dpre", np.full(rows * C, SENT), ddt)
    put("mean", mean), put("istd", istd), put("gamma", gamma), put("work", np.full(200 * C, np.nan))
    if sums:
        put("sum_dy", s1), put("sum_dyxh", s2)
    for k in ("dgamma", "dbeta", "dbias"):
        if k not in null:
            put(k, grad())
    c = case("bn_bwd", name, dict(rows=rows, C=C, count=float(count or max(1, nv)), act=act, row_mask=mask, dtype=dt, ld_dy=ld,
                                  sums=bool(sums), no_finalize=no_finalize, off=off), bufs,
             ["dpre", "work"] + [k for k in ("dgamma", "dbeta", "dbias") if k in bufs], exact)
    assert bn_bwd_form(c) == form, (name, bn_bwd_form(c))
    return c


def bn_bwd_cases():
    """Chosen from ns_bn_bwd's conditions.  Scalar form: min(32, ceil(rows / 64)) row blocks of ceil(rows / blocks) rows -
    65: 33 + 32; 2049: 32 blocks of 65, the last of 34 - and a channel loop of 256 threads (C = 258: a second trip of two).
    Vector forms: min(64, ceil(rows / 128)) row blocks x ceil(C / 64) column blocks of 16 quads x 16 row lanes, 64 rows per
    trip - 128: one block; 129: two of 65 and 64, so one lane takes a second trip; 300: three; 8193: 64 of 129 (the finaliser's
    eight lanes add eight blocks each; ns_stats_finalize's 32 lanes two slots each); C = 4 one quad, 68 a second column block
    with one quad and a ragged 32-column finaliser block, 132 a third.  Masks: (10, 2, 9) and (7, 3, 7) do not divide the
    rows, (10, 0, 7) lo = 0, (7, 3, 7) hi = period, (700, 0, 500) and (3000, 0, 2600) leave whole row blocks invalid."""
    N, R, T, S, Q = ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID, ACT_SOFTSIGN
    one = _bn_bwd_case
    out = [one("scalar-C6-rows70-tanh-mask", 70, 6, T, mask=(10, 2, 9)),
           one("scalar-C258-rows3-sigmoid", 3, 258, S, seed=141),
           one("scalar-C8-ld10-none", 5, 8, N, ld=10, seed=142),
           one("scalar-C6-ld9-col2-tanh-mask", 70, 6, T, ld=9, col0=2, mask=(7, 3, 7), seed=143),
           one("scalar-C6-rows1-softsign", 1, 6, Q, seed=144),
           one("scalar-C6-rows65-relu", 65, 6, R, seed=145),
           one("scalar-C6-rows2049-none-mask", 2049, 6, N, mask=(700, 0, 500), seed=146),
           one("scalar-C6-rows70-sums-given-tanh-mask", 70, 6, T, mask=(10, 0, 7), sums=True, seed=147),
           one("scalar-C6-rows130-bf16-relu-mask", 130, 6, R, dt="bf16", mask=(10, 2, 9), seed=148),
           one("scalar-C6-rows130-bf16dpre-sigmoid", 130, 6, S, ddt="bf16", seed=149),
           one("scalar-exact-C6-rows160-relu", 160, 6, R, mask=(10, 2, 6), exact=True, seed=150),
           one("scalar-exact-C6-rows160-count128-none", 160, 6, N, mask=(50, 0, 49), count=128, exact=True, seed=151)]
    for i, k in enumerate(("z", "dy", "dpre", "mean", "istd", "gamma", "work")):
        out.append(one("scalar-C8-shifted-%s" % k, 67, 8, (T, R, S, Q, N)[i % 5], shift=k, mask=(10, 2, 9), seed=152 + i))
    out.append(one("scalar-C8-shifted-sum_dy", 67, 8, T, shift="sum_dy", sums=True, seed=159))
    for k in ("dgamma", "dbeta", "dbias"):
        out.append(one("scalar-C6-rows70-no-%s" % k, 70, 6, T, mask=(10, 2, 9), null=(k,), seed=160))
    for form in ("vector", "fallback"):
        sd = 170 if form == "vector" else 200
        out += [one(form + "-C4-rows1-none", 1, 4, N, seed=sd),
                one(form + "-C68-rows128-tanh-mask", 128, 68, T, mask=(10, 0, 7), seed=sd + 1),
                one(form + "-C132-rows129-sigmoid-mask", 129, 132, S, mask=(7, 3, 7), seed=sd + 2),
                one(form + "-C8-rows8193-relu-mask", 8193, 8, R, mask=(3000, 0, 2600), seed=sd + 3),
                one(form + "-C68-rows300-bf16-softsign-mask", 300, 68, Q, dt="bf16", mask=(10, 2, 9), seed=sd + 4),
                one(form + "-C68-rows300-bf16dpre-relu-ld80-col8", 300, 68, R, ddt="bf16", ld=80, col0=8, seed=sd + 5),
                one(form + "-exact-C68-rows160-relu", 160, 68, R, mask=(10, 2, 6), exact=True, seed=sd + 6),
                one(form + "-exact-C68-rows160-count128-none", 160, 68, N, mask=(50, 0, 49), count=128, exact=True, seed=sd + 7),
                one(form + "-exact-C8-rows160-bf16dpre-none", 160, 8, N, ddt="bf16", mask=(10, 2, 6), exact=True, seed=sd + 8)]
        for k in ("dgamma", "dbeta", "dbias"):
            out.append(one(form + "-C8-rows70-no-%s" % k, 70, 8, T, mask=(10, 2, 9), null=(k,), seed=sd + 9))
    out += [one("vector-C68-rows300-split-tanh-mask", 300, 68, T, mask=(10, 2, 9), no_finalize=True, seed=190),
            one("vector-C8-rows8193-split-bf16dpre-none", 8193, 8, N, ddt="bf16", no_finalize=True, seed=191),
            one("vector-C4-rows1-split-relu", 1, 4, R, no_finalize=True, seed=192),
            one("vector-C68-rows300-sums-not-the-column-sums", 300, 68, T, mask=(10, 2, 9), wrong_sums=True, seed=193)]
    return out


def _bn_bwd_resum(c):
    """The given sums of a probe: the column sums of its own dy."""
    if not c["p"]["sums"]:
        return c
    p, b, off = c["p"], c["bufs"], c["p"]["off"]
    rows, C = p["rows"], p["C"]
    get = lambda k, n: b[k][0][off[k]:off[k] + n].astype(np.float64)
    valid = row_valid(rows, p["row_mask"])[:, None]
    dy = np.where(valid, get("dy", rows * C).reshape(rows, C), 0)
    xhat = np.where(valid, (get("z", rows * C).reshape(rows, C) - get("mean", C)) * get("istd", C), 0)
    for k, s in (("sum_dy", dy.sum(0)), ("sum_dyxh", (dy * xhat).sum(0))):
        x = b[k][0].copy()
        x[off[k]:off[k] + C] = s
        b[k] = (x, "f32")
    return c


def bn_bwd_probes():
    """dy = 0 but a single 1, on the count-128 exact cases (160 rows, rows 49, 99, 149 masked).  Scalar: 3 row blocks of 54,
    54 and 52 rows.  Vector forms: 2 row blocks of 80 rows - lane l of 16 takes rows l, l + 16, l + 32, l + 48 (the four
    unrolled slots) and l + 64 (a second trip) of its block - and columns 0 - 63 | 64 - 67.  A row counted twice or dropped
    makes s1 differ from 1 and shows in every dpre of the column; a masked row's 1 changes nothing."""
    out = []
    base = {c["name"]: c for c in bn_bwd_cases()}
    vec = [("block0-first", 0, 0), ("slot1", 16, 1), ("slot2", 32, 2), ("slot3", 48, 3), ("quad-first", 48, 4), ("lane15", 15, 7),
           ("lane15-slot3", 63, 8), ("second-trip", 64, 12), ("block0-last", 79, 63), ("block1-first", 80, 64),
           ("last-valid", 159, 67), ("masked", 99, 5), ("colblock-last", 100, 63), ("colblock-first", 100, 64)]
    for form in ("fallback", "vector"):
        at = [(k, MARGIN + r * 68 + ch) for k, r, ch in (vec if form == "fallback" else vec[::3] + vec[-3:-2])]
        out += probes(base[form + "-exact-C68-rows160-count128-none"], "dy", at)
    sc = [("block0-first", 0, 0), ("block0-last", 53, 5), ("block1-first", 54, 0), ("block1-last", 107, 2), ("block2-first", 108, 1),
          ("last-valid", 159, 5), ("masked", 99, 3)]
    out += probes(base["scalar-exact-C6-rows160-count128-none"], "dy", [(k, MARGIN + r * 6 + ch) for k, r, ch in sc])
    return [_bn_bwd_resum(c) for c in out]


ZERO_BYTES = (16, 48, 4096 + 16, (1 << 20) + 16)


def zero_cases():
    """ns_zero: one range per case.  ns_zero_many: 25 ranges (two launches) of unequal size, one of them empty, with
    sentinel gaps between them in one buffer."""
    out = [case("zero", "bytes%d" % b, dict(ranges=[(MARGIN, b // 4)], many=False),
                dict(buf=(framed(rounding_values(b // 4, 130) + np.float32(1)), "f32")), ["buf"]) for b in ZERO_BYTES]
    ranges, at = [], MARGIN
    for i in range(25):
        n = 0 if i == 7 else 4 * (1 + (i * 37) % 29) * (300 if i in (3, 24) else 1)
        ranges.append((at, n))
        at += n + MARGIN
    out.append(case("zero", "many25", dict(ranges=ranges, many=True),
                    dict(buf=(np.full(at, SENT, np.float32), "f32")), ["buf"]))
    return out


# ------------------------------------------------------------------------------------------------------ the check
def _margins(got, n):
    return Verdict(bool((got[:MARGIN] == SENT).all() and (got[MARGIN + n:] == SENT).all()), 0.0, "a margin was written")


def check(c, got, factor=2.0):
    """got {buffer: float32 array of the WHOLE buffer after the call} against the expectation -> {buffer: Verdict}.
    The rule of the CPU module's mutants and of the GPU module alike."""
    exp = expect(c)
    res = {}
    for o in c["outs"]:
        dt = c["bufs"][o][1]
        if c["op"] == "adam" and o == "shadow":        # RNE_bf16 of the kernel's OWN new weight, or untouched on a skip
            n = c["p"]["n"]
            want = c["bufs"][o][0].copy()
            if c["p"]["raised"] is None:
                want[MARGIN:MARGIN + n] = rne_bf16(got["p"][MARGIN:MARGIN + n])
            res[o] = accepts(got[o], want, None, "f32")
        elif c["op"] == "bn_fwd" and o in ("y_hi", "y_lo"):
            if o == "y_lo":
                continue
            p = c["p"]
            n = p["rows"] * p["C"]
            hi, lo = got["y_hi"][MARGIN:MARGIN + n], got["y_lo"][MARGIN:MARGIN + n]
            if "y" in c["outs"]:                       # beside the fp32 value: the exact split of the kernel's own y
                idx = (p["y_off"] + np.arange(p["rows"])[:, None] * (p["ld_y"] or p["C"]) + np.arange(p["C"])[None, :]).reshape(-1)
                whi, wlo = split_hi_lo(got["y"][idx])
                v = Verdict(bool(bits_equal(hi, whi).all() and bits_equal(lo, wlo).all()), 0.0, "not the split of the kernel's own y")
            else:
                v = pair_accepts(hi, lo, exp["y_value"][0].reshape(-1), exp["y_value"][1].reshape(-1), factor)
            m = Verdict(_margins(got["y_hi"], n).ok and _margins(got["y_lo"], n).ok, 0.0, "a margin was written")
            res["y_hi"] = v if not v.ok or m.ok else m
        elif c["op"] == "bn_bwd" and o == "work":      # 200 * C floats that the call may use as it likes; nothing beyond them
            at, n = c["p"]["off"]["work"], 200 * c["p"]["C"]
            same = bits_equal(got[o], c["bufs"][o][0])
            res[o] = Verdict(bool(same[:at].all() and same[at + n:].all()), 0.0, "written outside its 200 * C floats")
        elif c["op"] == "bn_bwd" and o == "dbias" and not c["exact"]:
            # += the column sums of dpre AS STORED BY THIS CALL (held to the reference on its own), in an unknown order
            p = c["p"]
            sl, at = _bn_bwd_slots(c)[o], p["off"]["dpre"]
            d = got["dpre"][at:at + p["rows"] * p["C"]].astype(np.float64).reshape(p["rows"], p["C"])
            val, err = c["bufs"][o][0].astype(np.float64), np.zeros(c["bufs"][o][0].shape)
            n = int(row_valid(p["rows"], p["row_mask"]).sum()) + 1                       # the prefill is a term
            with np.errstate(invalid="ignore", over="ignore"):                           # (a wrong kernel's infinities)
                err[sl] = sum_expect(None, np.abs(d).sum(0) + np.abs(val[sl]), n, False)
                val[sl] += d.sum(0)
            res[o] = accepts(got[o], val, err, dt, factor)
        else:
            val, err = exp[o]
            res[o] = accepts(got[o], val, err, dt, factor)
    return res


def rejected(c, got, factor=2.0):
    return any(not v.ok for v in check(c, got, factor).values())
