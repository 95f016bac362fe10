"""Float64 contract of ns_l1_loss_masked (include/nspeech_hip.h), stated from the header - not from the kernel.  Proven on
the CPU by tests/test_masked_loss_ref_cpu.py; tests/test_masked_loss_contract_gpu.py holds every kernel form to it, and the
model tests use masked_taco_loss, the same statement in torch float64 on the oracles' outputs.

  T_n = lengths[n] clamped into [1, T] (None: T);  d = pred - target over the frames t < T_n
  acc[0] = sum |d| over all bins, acc[1] = the same over bins < n_prio            (written, not accumulated)
  dpred[n, padl + t, f] = sign(d) (fp32(w_all) + (f < n_prio ? fp32(w_prio) : 0)) for t < T_n, sign(0) = 0: one fp32 add,
  then a product with -1, 0 or 1 - exact - and for a bf16 buffer its round-to-nearest-even;  0 for T_n <= t < T;
  every other element of the buffer - rows outside [padl, padl + T), columns F .. ldd, the margins - keeps its bits.

A CASE is a dict: name, p (the call's scalars), lengths (list or None), ddt ("f32" | "bf16" | None: no dpred), exact
(inputs are multiples of 1/4, so every partial sum in every order is an exact fp32 number and the sums are compared bit for
bit) or random (the sums are held to sum_bound), and the arrays pred / target / dpred / acc with sentinel margins as
tests/pointwise_ref.py frames them.  dpred is prefilled with the sentinel EVERYWHERE: outside the valid region it must
survive (the sentinel check), on the padded frames it must become zero (the stale-gradient check).

`mut` selects the WRONG kernels that the CPU module shows the comparison to reject; None is the contract."""
import numpy as np

from pointwise_ref import MARGIN, SENT, U, bits_equal, framed, store, unit_values

MUTANTS = ("off_by_one", "stale_rows", "no_clamp", "prio_all", "sign0")
BASE = dict(N=3, T=20, P=25, padl=2)
LENGTHS = (20, 12, 3)


def frames_of(lengths, N, T, mut=None):
    if lengths is None:
        return np.full(N, T, np.int64)
    fr = np.asarray(lengths, np.int64)
    return np.minimum(fr, T) if mut == "no_clamp" else np.clip(fr, 1, T)


def views(c):
    p = c["p"]
    N, T, P, padl, F = p["N"], p["T"], p["P"], p["padl"], p["F"]
    prow = np.arange(N)[:, None] * P + padl + np.arange(T)[None, :]                     # [N, T] rows of the padded layout
    pred = c["pred"][MARGIN + prow[:, :, None] * p["ldp"] + np.arange(F)[None, None, :]]
    tgt = c["target"][MARGIN:MARGIN + N * T * F].reshape(N, T, F)
    return prow, pred, tgt


def expect(c, mut=None):
    """{"acc": the two sums in float64 (their terms are magnitudes, so they are sum |terms| as well), "dpred": the whole
    expected buffer as float32 values, margins included (None without a gradient)}."""
    p = c["p"]
    N, T, F, n_prio = p["N"], p["T"], p["F"], p["n_prio"]
    prow, pred, tgt = views(c)
    fr = frames_of(c["lengths"], N, T, mut)
    live = np.arange(T)[None, :] < (fr[:, None] + (1 if mut == "off_by_one" else 0))   # [N, T]
    d32 = pred - tgt                                                                     # fp32: one rounding per term
    d = pred.astype(np.float64) - tgt
    prio = np.arange(F) < n_prio
    ab = np.abs(d) * live[:, :, None]
    acc = np.array([ab.sum(), ab[:, :, prio].sum()])
    out = dict(acc=acc, dpred=None)
    if c["ddt"]:
        w_hi = np.float32(p["w_all"]) + np.float32(p["w_prio"])
        w = np.where(prio | (mut == "prio_all"), w_hi, np.float32(p["w_all"]) + np.float32(0)).astype(np.float32)
        sg = np.sign(d32).astype(np.float32)
        if mut == "sign0":
            sg = np.where(d32 >= 0, 1, -1).astype(np.float32)
        g = store(sg * w[None, None, :], c["ddt"])
        buf = c["dpred"].copy()
        idx = MARGIN + prow[:, :, None] * p["ldd"] + np.arange(F)[None, None, :]
        old = buf[idx]
        buf[idx] = np.where(live[:, :, None], g, old if mut == "stale_rows" else np.float32(0))
        out["dpred"] = buf
    return out


def naive(c):
    """The contract once more as a triple loop over (n, t, f) in Python floats: the CPU module holds expect() to it."""
    p = c["p"]
    N, T, P, padl, F = p["N"], p["T"], p["P"], p["padl"], p["F"]
    pred, tgt = c["pred"][MARGIN:], c["target"][MARGIN:]
    buf = c["dpred"].copy() if c["ddt"] else None
    s_all = s_pr = 0.0
    for n in range(N):
        Tn = T if c["lengths"] is None else min(max(int(c["lengths"][n]), 1), T)
        for t in range(T):
            row = n * P + padl + t
            for f in range(F):
                if t >= Tn:
                    if buf is not None:
                        buf[MARGIN + row * p["ldd"] + f] = 0.0
                    continue
                a, b = pred[row * p["ldp"] + f], tgt[(n * T + t) * F + f]
                d = float(a) - float(b)
                s_all += abs(d)
                w = np.float32(p["w_all"])
                if f < p["n_prio"]:
                    s_pr += abs(d)
                    w = w + np.float32(p["w_prio"])
                if buf is not None:
                    g = np.float32(0) if d == 0 else (w if d > 0 else -w)
                    buf[MARGIN + row * p["ldd"] + f] = store(np.float32(g), c["ddt"])
    return dict(acc=np.array([s_all, s_pr]), dpred=buf)


def sum_depth(p):
    """The longest chain of fp32 adds a term of acc[0] can pass through, from the header's order of sums: a thread's own
    terms in loop order (K of them: its share of the N T F elements over the grid's threads, rounded up to whole rows or
    quads), the wave tree (6), the workgroup's 4 waves in index order (4), then the second launch: a thread's partials (at
    most 4 of the at most 1024), the wave tree (6) and 4 waves (4).  The grid is stated as an upper bound on K only: at
    least min(512, ceil(rows / 4)) workgroups of four waves for F >= 256 (a wave per row, a lane F / 64 columns of it
    rounded up to 4 per quad plus the tail), at least min(256, ceil(N T F / 1024)) workgroups of 256 threads otherwise."""
    N, T, F = p["N"], p["T"], p["F"]
    rows = N * T
    if F >= 256:
        waves = 4 * min(512, -(-rows // 4))
        k = -(-rows // waves) * (4 * -(-F // 256) + 8)
    else:
        threads = 256 * min(256, -(-(rows * F) // 1024))
        k = 4 * -(-(rows * F) // (4 * threads)) + 4
    return k + 6 + 4 + 4 + 6 + 4


def sum_bound(c, e):
    """|acc - float64 sum| <= (1 + depth) 2^-24 sum |d|, times 1.01 for the second-order terms: one rounding of each
    d = pred - target (2^-24 |d|), and each add on a term's path adds at most 2^-24 of the partial sum it forms, which
    sum |d| bounds (the terms are magnitudes)."""
    return 1.01 * (1 + sum_depth(c["p"])) * U * e["acc"]


def check(c, got_acc, got_dpred, e=None):
    """The list of failures (empty: the outputs meet the contract).  got_acc: the whole acc buffer as float32; got_dpred:
    the whole dpred buffer as float32 values (bf16 widened), or None."""
    e = e or expect(c)
    bad = []
    o = c["p"]["acc_off"]
    want_buf = c["acc"].copy()
    got_buf = np.asarray(got_acc, np.float32).copy()
    sums = got_buf[o:o + 2].astype(np.float64)
    got_buf[o:o + 2] = want_buf[o:o + 2]
    if not bits_equal(got_buf, want_buf).all():
        bad.append("acc: a word beside the two sums was written")
    if c["exact"]:
        assert float(e["acc"].max()) / 0.25 < 2 ** 24
        if not bits_equal(sums.astype(np.float32), e["acc"].astype(np.float32)).all():
            bad.append("acc: %r, exact sums %r" % (sums.tolist(), e["acc"].tolist()))
    else:
        err, bound = np.abs(sums - e["acc"]), sum_bound(c, e)
        c["worst"] = float(np.max(err / np.maximum(bound, 1e-300)))
        if not (err <= bound).all():
            bad.append("acc: error %r over the bound %r" % (err.tolist(), bound.tolist()))
    if c["ddt"]:
        same = bits_equal(np.asarray(got_dpred, np.float32), e["dpred"])
        if not same.all():
            i = int(np.flatnonzero(~same)[0])
            bad.append("dpred: %d elements differ, the first at %d: %r for %r" % (int((~same).sum()), i, float(got_dpred[i]),
                                                                              float(e["dpred"][i])))
    return bad


def mutant_outputs(c, mut):
    """What a kernel with the named defect would leave: (acc buffer, dpred buffer)."""
    e = expect(c, mut)
    acc = c["acc"].copy()
    o = c["p"]["acc_off"]
    acc[o:o + 2] = e["acc"].astype(np.float32)
    return acc, e["dpred"]


# ------------------------------------------------------------------------------------------------------ cases
SHAPES = [  # name, F, ldp, ldd, dpred dtype, n_prio, lengths, overrides of BASE
    ("wide-1025-f32", 1025, 1028, 1028, "f32", 205, LENGTHS, {}),
    ("wide-1025-bf16", 1025, 1028, 1028, "bf16", 205, LENGTHS, {}),             # the linear term of the mixed step
    ("wide-1025-nograd", 1025, 1028, 0, None, 205, LENGTHS, {}),
    ("wide-1025-ld1025", 1025, 1025, 1025, "f32", 1025, LENGTHS, {}),            # leading dimensions no multiple of 4: scalar
    ("wide-1025-ld1025-bf16", 1025, 1028, 1025, "bf16", 0, LENGTHS, {}),
    ("wide-1025-nolengths", 1025, 1028, 1028, "bf16", 205, None, {}),
    ("wide-257-bf16", 257, 260, 260, "bf16", 0, LENGTHS, {}),
    ("wide-257-f32", 257, 260, 264, "f32", 205, (20, 1, 3), {}),
    ("wide-256", 256, 260, 260, "f32", 205, LENGTHS, {}),
    ("wide-256-prioF", 256, 256, 256, "bf16", 256, LENGTHS, {}),
    ("narrow-80", 80, 84, 84, "f32", 0, LENGTHS, {}),                             # the mel term: quads
    ("narrow-80-prio", 80, 80, 80, "f32", 37, (20, 1, 3), {}),                    # n_prio inside a quad, a row with T_n = 1
    ("narrow-80-bf16", 80, 84, 84, "bf16", 80, LENGTHS, {}),                      # a bf16 gradient of narrow rows: flat
    ("narrow-80-nograd", 80, 80, 0, None, 0, LENGTHS, {}),
    ("narrow-80-ld81", 80, 81, 81, "f32", 0, LENGTHS, {}),
    ("narrow-78", 78, 80, 80, "f32", 78, LENGTHS, {}),                            # flat
    ("narrow-16", 16, 16, 20, "f32", 5, LENGTHS, {}),
    ("narrow-16-clamps", 16, 16, 16, "f32", 0, (0, -4, 99), {}),                  # -> 1, 1, 20
    ("wide-256-clamps", 256, 256, 256, "f32", 0, (99, 0, -4), {}),
    ("taco1-mel", 80, 80, 80, "f32", 0, LENGTHS, dict(P=25, padl=5)),             # P = (S + 1) r, padl = r; r 5, S 4
    # more rows than one pass of the grid: 1024 workgroups of 4 rows (wide), 512 x 256 quads or elements (narrow)
    ("wide-256-rows4250", 256, 256, 256, "bf16", 205, (850, 400, 1, 849, 13), dict(N=5, T=850, P=853, padl=3)),
    ("narrow-80-rows6800", 80, 80, 80, "f32", 0, (850, 400, 1, 849, 13, 850, 2, 700), dict(N=8, T=850, P=853, padl=3)),
    ("narrow-80-rows6800-bf16", 80, 80, 80, "bf16", 0, (850, 400, 1, 849, 13, 850, 2, 700), dict(N=8, T=850, P=853, padl=3)),
]
RANDOM = ("wide-1025-f32", "wide-1025-bf16", "wide-1025-ld1025", "wide-257-bf16", "wide-256", "narrow-80", "narrow-80-bf16",
          "narrow-78", "narrow-16", "wide-256-rows4250", "narrow-80-rows6800")


def make_case(name, random=False):
    name0, F, ldp, ldd, ddt, n_prio, lengths, over = next(s for s in SHAPES if s[0] == name)
    b = dict(BASE, **over)
    N, T, P, padl = b["N"], b["T"], b["P"], b["padl"]
    rng = np.random.RandomState(60)
    if random:
        pred, tgt = rng.randn(N * P * ldp).astype(np.float32), rng.randn(N, T, F).astype(np.float32)
    else:
        pred, tgt = unit_values(N * P * ldp, 61), unit_values((N, T, F), 62)      # pad rows carry values as well
    prow = np.arange(N)[:, None] * P + padl + np.arange(T)[None, :]
    same = rng.rand(N, T, F) < 0.1                                                # pred == target: sign(0) = 0
    same[:, 0, [0, F - 1]] = True
    tgt = np.where(same, pred[prow[:, :, None] * ldp + np.arange(F)[None, None, :]], tgt).astype(np.float32)
    fr = frames_of(lengths, N, T)
    C = int(fr.sum())
    c = dict(name=name + ("-random" if random else ""), exact=not random, lengths=None if lengths is None else list(lengths),
             ddt=ddt, pred=framed(pred), target=framed(tgt), acc=framed([3.25, -1.5, 2.0, 0.75]),
             p=dict(N=N, T=T, P=P, padl=padl, F=F, ldp=ldp, ldd=ldd, n_prio=n_prio, w_all=0.5 / (C * F),
                    w_prio=0.5 / (C * max(1, n_prio)), acc_off=MARGIN + (2 if "prio" in name else 0)))
    if ddt:
        c["dpred"] = framed(np.full(N * P * ldd, SENT))
    return c


def case_names(random=False):
    return [n + "-random" for n in RANDOM] if random else [s[0] for s in SHAPES]


PROBES = {  # (n, t, f) of the one differing element: the last real frame and the first padded one of a row, the edges of the
    # priority band, of a quad, of a lane's span and of the tail column
    "wide-1025-bf16": [(0, 19, 1024), (1, 11, 0), (1, 12, 0), (1, 11, 204), (1, 11, 205), (2, 2, 1023), (2, 3, 1023), (2, 0, 256)],
    "wide-1025-ld1025": [(1, 11, 1024), (1, 12, 1024), (2, 2, 512), (2, 3, 511)],
    "narrow-80": [(1, 11, 79), (1, 12, 0), (2, 2, 3), (2, 2, 4), (2, 3, 4)],
    "narrow-78": [(1, 11, 77), (1, 12, 77), (2, 3, 0)],
    "narrow-16-clamps": [(0, 0, 15), (0, 1, 0), (1, 0, 0), (1, 1, 15), (2, 19, 15)],
    "taco1-mel": [(0, 19, 79), (1, 11, 0), (1, 12, 79)],
    "wide-256-rows4250": [(1, 399, 255), (1, 400, 0), (4, 12, 204), (4, 13, 204), (3, 848, 205)],
    "narrow-80-rows6800": [(7, 699, 79), (7, 700, 0), (6, 1, 40), (6, 2, 40)],
}


def probe_names():
    return ["%s-probe-n%d-t%d-f%d" % ((k,) + pos) for k, v in PROBES.items() for pos in v]


def make_probe(name):
    """pred - target = 1 at one element and 0 everywhere else: the sums are exactly 1 or 0, the gradient has one non-zero."""
    base, pos = name.split("-probe-")
    n, t, f = (int(x[1:]) for x in pos.split("-"))
    c = make_case(base)
    _, pred, _ = views(c)
    tgt = pred.copy()
    tgt[n, t, f] -= 1.0
    c["target"] = framed(tgt)
    c["name"] = name
    return c


def build(name):
    if "-probe-" in name:
        return make_probe(name)
    return make_case(name[:-7], True) if name.endswith("-random") else make_case(name)


# ------------------------------------------------------------------------------------------------------ the models' loss
def masked_taco_loss(out, mel, lin, frames, n_prio):
    """(loss, mel_loss, linear_loss) of taco1_loss / taco2_loss over the frames t < frames[n] only, torch float64: the means
    divide by C = sum_n frames[n] (times the bins), the linear term keeps its half / half of all bins and the band."""
    import torch
    fr = torch.as_tensor(np.asarray(frames), dtype=torch.int64)
    To = mel.shape[1]
    fr = fr.clamp(1, To)
    live = (torch.arange(To)[None, :] < fr[:, None]).to(mel.dtype)[:, :, None]
    C = float(fr.sum())
    mel_loss = ((mel - out["mel_outputs"]).abs() * live).sum() / (C * mel.shape[2])
    l1 = (lin - out["linear_outputs"]).abs() * live
    linear_loss = 0.5 * l1.sum() / (C * lin.shape[2]) + 0.5 * l1[:, :, :n_prio].sum() / (C * n_prio)
    return mel_loss + linear_loss, mel_loss, linear_loss
