"""Every kernel body of csrc/elementwise.hip - but ns_dropout_rows, which tests/test_prenet_dropout_contract_gpu.py holds
to its own contract - and ns_zero / ns_zero_many of core.hip, against the float64 contract of tests/pointwise_ref.py
(itself proven by tests/test_pointwise_ref_cpu.py), through nspeech_amd.ops - and through the parameter block directly
where a form has no wrapper argument (ns_colsum without `work`).

For every case: every buffer the call sees sits between MARGIN sentinels, and the expectation covers the WHOLE buffer, so
the margins, the padding behind a row, the columns a leading dimension leaves out and the pad rows of a padded layout are
compared bit for bit like any other element; `+=` outputs are prefilled with non-zero values; every input is bit-identical
afterwards; nothing is excused.  The three kinds of expected value - exact, exact by construction, bounded at 2 x the
running-error bound, bf16 outputs by the bf16 store rule - are those of pointwise_ref.check(), the function the CPU module
shows to reject the mutants on these same inputs.  Kernels with arrival counters (embedding_bwd, colsum, sumsq) run twice
on the same scratch and must give the same bits: the counters were left at zero.

Which body a case takes is derived from the launchers' conditions (ns_* in elementwise.hip), beside each group below.

Worst error / bound on the MI355X (every test prints its own, `pytest -s`; the bound is 2 x the running-error bound, so
0.5 is a kernel at the first-order bound):
  exact, 0 of every element differs: copy3d, embedding_fwd, cast2d and CastBatch, split_hi_lo, zero / zero_many, the L1
  gradient, Adam's shadow and the skip on a raised status word, segment min / max, the pre-split pair of bn_fwd beside
  its y; and every exact-by-construction sum and one-hot probe of colsum, sumsq, segment_stats, l1_loss, embedding_bwd
  bounded, fp32 storage     bn_fwd mean 0.47  istd 0.15  moving mean / var 0.42 / 0.37  y 0.44     adam m 0.48  v 0.25
                            p 0.50     highway y 0.48  dhpre 0.50  dtpre 0.40  dx 0.49     act_bwd 0.39
                            gru_pointwise out 0.50  out2 0.40  dzg 0.39  carry 0.50
  random sums               colsum 0.20  l1_loss 0.013  segment_stats 0.009  embedding_bwd 0.004  sumsq 0.001
  bounded, bf16 storage     neighbours / computed values: gru_pointwise out 1 / 5632 (mode 2, N = 33), highway dtpre
                            4 / 1 048 202; every other value of every bf16 buffer is bf16(reference)
0.50 is a kernel whose single worst element sits at the first-order bound (one half-ulp rounding of an expression with
one operation: gru mode 0, highway dx); nothing exceeds it.

BatchNorm backward (ns_bn_bwd, ns_bn_bwd_finalize and their use of ns_stats_finalize; 51 cases and 27 one-hot probes, each
launched twice, the second time on the work area the first launch left; 80 tests in 2.1 s on the MI355X, the slowest
0.16 s).  `work` is 200 * C NaNs followed by a guard tail of sentinels, the gradients are prefilled, masked rows of dy and z
hold 1e30 and the columns of a wide dy outside the block NaN.  Worst error / bound per form:
                 dpre fp32   dpre bf16 (neighbours / computed)   dgamma   dbeta   dbias (against the call's own dpre)
  scalar           0.23          0 / 1 043                        0.35     0.36     0.32
  vector (sums)    0.46          0 / 89 955                       exact    exact    0.44
  fallback         0.06          1 / 24 523                       0.24     0.10     0.42
  and 0 of every element differs in the nine exact-by-construction cases and the probes, dbias included.
Found: no kernel computes a wrong value.  The scalar form's dbias met in one float atomicAdd per row block, against the
header's "every output is bitwise repeatable": on the parent commit 20 launches of the 32-block case gave 20 different bit
patterns of dbias (all within the bound; dpre, dgamma, dbeta repeated).  The row blocks park their partial sums in `work`
now and a third launch adds them in block order; test_bn_bwd_scalar_32_blocks_three_times guards that, and the proof is
that ns_bn_bwd reaches no float atomic.  A dpre_dtype outside the documented pair was ignored; it is refused now
(tests/test_bn_bwd_abi_cpu.py).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pointwise_ref as R
from pointwise_ref import MARGIN as M

pytestmark = pytest.mark.gpu

TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "i32": torch.int32, "i64": torch.int64}
WORST = {}


def _ops():
    from nspeech_amd import ops
    return ops


def upload(c, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(a)).to(TDT[dt]).to(dev) for k, (a, dt) in c["bufs"].items()}


def download(d):
    return {k: (t.float() if t.is_floating_point() else t).cpu().numpy() for k, t in d.items()}


def run(c, dev, twice=False):
    """Launch the case, check inputs and outputs, return the outputs.  twice: a second launch on fresh copies of the
    buffers but the wrappers' same scratch must give the same bits."""
    d = upload(c, dev)
    CALL[c["op"]](c, d)
    torch.cuda.synchronize()
    got = download(d)
    for k, (a, dt) in c["bufs"].items():
        if k not in c["outs"]:
            same = R.bits_equal(got[k], a).all() if dt in ("f32", "bf16") else np.array_equal(got[k], a)
            assert same, (c["name"], k, "an input was written")
    verdicts = R.check(c, got)
    for o, v in sorted(verdicts.items()):
        key = (c["op"], o, c["bufs"][o][1])
        WORST[key] = max(WORST.get(key, 0.0), v.worst)
        print("  %-14s %-52s %-12s %s" % (c["op"], c["name"], o, "error / bound %.3f" % v.worst if c["bufs"][o][1] == "f32" else
                                          "bf16 neighbours %d of %d" % (v.neighbours, v.counted)))
    bad = {o: v.why for o, v in verdicts.items() if not v.ok}
    assert not bad, (c["name"], bad)
    if twice:
        d2 = upload(c, dev)
        CALL[c["op"]](c, d2)
        torch.cuda.synchronize()
        again = download(d2)
        for o in c["outs"]:
            assert R.bits_equal(again[o], got[o]).all(), (c["name"], o, "a second launch on the same scratch differs")
    return got


@functools.lru_cache(maxsize=1)
def _built(fn):
    return {c["name"]: c for c in fn()}


def cases_of(*fns):
    """Parametrisation by case name; the cases themselves are rebuilt when a test runs (the largest hold 17 MB each)."""
    names = []
    for fn in fns:
        names += [(fn, c["name"]) for c in fn()]
    return pytest.mark.parametrize("fn,name", names, ids=[n for _, n in names])


def get(fn, name):
    return _built(fn)[name]


# ------------------------------------------------------------------------------------------------------ the calls
def _copy3d(c, d):
    p = c["p"]
    _ops().copy3d(d["src"], d["dst"], p["I"], p["J"], p["Cc"], p["src_strides"], p["dst_strides"], src_off=p["src_off"],
                  dst_off=p["dst_off"], accumulate=p["accumulate"])


def _embedding_fwd(c, d):
    p = c["p"]
    _ops().embedding_fwd(d["ids"], d["table"], d["out"][M:], p["N"], p["T"], p["P"], p["padl"], p["D"], p["V"], table_off=p["table_off"])


def _embedding_bwd(c, d):
    p = c["p"]
    _ops().embedding_bwd(d["ids"], d["dout"][M:], d["dtable"], p["N"], p["T"], p["P"], p["padl"], p["D"], p["V"], dtable_off=p["dtable_off"])


def _inner(d, k):
    return d[k][M:] if k in d else None


def _bn_fwd(c, d):
    p = c["p"]
    _ops().bn_fwd(d["z"][M:], d.get("y"), p["rows"], p["C"], _inner(d, "col_sum"), _inner(d, "col_sumsq"), p["count"], d["gamma"],
                  d["beta"], d.get("moving_mean"), d.get("moving_var"), d["mean_out"][M:], d["istd_out"][M:], p["training"],
                  row_mask=p["row_mask"], eps=p["eps"], momentum=p["momentum"], gamma_off=M, beta_off=M, mm_off=M, mv_off=M,
                  y_hi=_inner(d, "y_hi"), y_lo=_inner(d, "y_lo"), y_off=p["y_off"], ld_y=p["ld_y"], stats_final=p["stats_final"])


def _colsum(c, d):
    p = c["p"]
    ops = _ops()
    if p["work"]:
        return ops.colsum(d["x"], p["ld"], p["rows"], p["C"], d["out"], x_off=p["x_off"], out_off=p["out_off"])
    from nspeech_amd import _lib as L
    q = L.struct("ns_colsum_params")                     # ops.colsum always hands a work buffer out: the atomic forms
    ops._fill(q, x=ops.ptr(d["x"], p["x_off"]), dtype=ops.dt(d["x"]), ld=p["ld"], rows=p["rows"], C=p["C"],
              out=ops.ptr(d["out"], p["out_off"]))
    L.call("ns_colsum", q, ops.stream())


def _l1_loss(c, d):
    p = c["p"]
    _ops().l1_loss(d["pred"][M:], p["ldp"], d["target"][M:], _inner(d, "dpred"), p["ldd"], p["N"], p["T"], p["P"], p["padl"], p["F"],
                   p["n_prio"], p["w_all"], p["w_prio"], d["loss_acc"], acc_off=p["acc_off"])


_SUMSQ_WORK = {}


def _sumsq(c, d):
    p = c["p"]
    work = None
    if p["work"]:
        dev = d["x"].device
        if dev not in _SUMSQ_WORK:
            _SUMSQ_WORK[dev] = torch.zeros(1032, dtype=torch.float32, device=dev)      # zeroed ONCE, as the contract says
        work = _SUMSQ_WORK[dev]
    _ops().sumsq(d["x"][M:], p["n"], d["out"], out_off=p["out_off"], work=work)


def _segment_stats(c, d):
    _ops().segment_stats(d["x"][M:], d["offsets"], c["p"]["nseg"], d["out"][M:])


def _adam(c, d):
    p = c["p"]
    status = [torch.zeros(4, dtype=torch.int32, device=d["p"].device) for _ in range(p["status_n"])]
    if p["raised"] is not None:
        status[p["raised"]][0] = 3
    _ops().adam(d["p"][M:], d["g"][M:], d["m"][M:], d["v"][M:], p["n"], _inner(d, "gnorm_sq"), p["clip"], p["grad_scale"], p["lr_t"],
                p["beta1"], p["beta2"], p["eps"], shadow=_inner(d, "shadow"), status=status, skipped=d["skipped"][M:])
    torch.cuda.synchronize()
    for i, s in enumerate(status):
        assert s.tolist() == [3 if i == p["raised"] else 0, 0, 0, 0], "a status word was written"


def _cast2d(c, d):
    p = c["p"]
    _ops().cast2d(d["src"], p["rows"], p["cols"], p["ld_src"], d.get("dst"), p["ld_dst"], p["transpose"], src_off=p["src_off"],
                  dst_off=p["dst_off"], dst_hi=d.get("dst_hi"), dst_lo=d.get("dst_lo"))


def _split(c, d):
    _ops().split_hi_lo(d["src"][M:], d["hi"][M:], d["lo"][M:], c["p"]["n"])


def _gru_pointwise(c, d):
    p = c["p"]
    pair = lambda k: (d[k], M) if k in d else None
    _ops().gru_pointwise(p["mode"], torch.empty(0, dtype=TDT[p["dtype"]]), p["N"], p["H"], p["t"], d.get("lengths"), ru=pair("ru"),
                         ru_sn=p["ru_sn"], c=pair("c"), c_sn=p["c_sn"], h_prev=pair("h_prev"), hp_sn=p["hp_sn"], out=pair("out"),
                         out_sn=p["out_sn"], out2=pair("out2"), out2_sn=p["out2_sn"], dzg=pair("dzg"), dzg_sn=p["dzg_sn"],
                         dh=pair("dh"), dh_sn=p["dh_sn"], carry=pair("carry"), carry_sn=p["carry_sn"], dh_add=pair("dh_add"),
                         dha_sn=p["dha_sn"], h_init=pair("h_init"), hi_sn=p["hi_sn"], reverse=p["reverse"], T=p["T"])


def _highway(c, d):
    _ops().highway(d["h"][M:], d["t"][M:], d["x"][M:], c["p"]["n"], y=_inner(d, "y"), dy=_inner(d, "dy"), dhpre=_inner(d, "dhpre"),
                   dtpre=_inner(d, "dtpre"), dx=_inner(d, "dx"))


def _act_bwd(c, d):
    p = c["p"]
    _ops().act_bwd(d["dy"][M:], d["y"][M:], d["dpre"][M:], p["rows"], p["C"], p["act"], row_mask=p["row_mask"])


_BN_WORK = {}                          # case name -> the work area its first launch left behind


def _bn_bwd(c, d):
    """ops.bn_bwd (every NULL gradient and dpre_dtype are expressible through it).  The second launch of a case runs on
    the work area that the first one used, as it was left.  no_finalize: the three gradients are bit-identical after the
    first call; ops.bn_bwd_finalize on the returned block then adds them."""
    p, ops = c["p"], _ops()
    off = p["off"]
    d["work"] = _BN_WORK.setdefault(c["name"], d["work"])
    inner = lambda k: d[k][off[k]:] if k in d else None
    form = R.bn_bwd_form(c, lambda k: (d[k].data_ptr() + off[k] * d[k].element_size()) % 16)
    assert form == c["name"].split("-")[0] == R.bn_bwd_form(c), (c["name"], form)
    blk = ops.bn_bwd(d["dy"], inner("z"), inner("dpre"), p["rows"], p["C"], inner("mean"), inner("istd"), d["gamma"], d.get("dgamma"),
                     d.get("dbeta"), d.get("dbias"), inner("work"), p["count"], p["act"], row_mask=p["row_mask"],
                     gamma_off=off["gamma"], dgamma_off=off.get("dgamma", 0), dbeta_off=off.get("dbeta", 0),
                     dbias_off=off.get("dbias", 0), sums=(inner("sum_dy"), inner("sum_dyxh")) if p["sums"] else None,
                     dy_off=off["dy"], ld_dy=p["ld_dy"], no_finalize=p["no_finalize"])
    if p["no_finalize"]:
        torch.cuda.synchronize()
        for k in ("dgamma", "dbeta", "dbias"):
            assert R.bits_equal(d[k].cpu().numpy(), c["bufs"][k][0]).all(), (c["name"], k, "written before the finaliser ran")
        ops.bn_bwd_finalize(blk)


def _zero(c, d):
    ops, p, buf = _ops(), c["p"], d["buf"]
    if not p["many"]:
        (start, n), = p["ranges"]
        return ops.zero(buf[start:start + n])
    from nspeech_amd import _lib as L               # ops.zero_many drops empty tensors: the list as it is, the empty one too
    n = len(p["ranges"])
    ptrs = (ctypes.c_void_p * n)(*[ops.ptr(buf, s) for s, _ in p["ranges"]])
    nbytes = (ctypes.c_size_t * n)(*[4 * k for _, k in p["ranges"]])
    L.check(L.lib().ns_zero_many(ptrs, nbytes, n, ctypes.c_void_p(ops.stream())), "ns_zero_many")


CALL = dict(copy3d=_copy3d, embedding_fwd=_embedding_fwd, embedding_bwd=_embedding_bwd, bn_fwd=_bn_fwd, colsum=_colsum,
            l1_loss=_l1_loss, sumsq=_sumsq, segment_stats=_segment_stats, adam=_adam, cast2d=_cast2d, split_hi_lo=_split,
            gru_pointwise=_gru_pointwise, highway=_highway, act_bwd=_act_bwd, zero=_zero, bn_bwd=_bn_bwd)


# ------------------------------------------------------------------------------------------------------ the cases
# copy3d_kernel is the only body; the dtype pair and `accumulate` are run-time branches of it.  ns_copy3d launches
# min(4096, ceil(total / 256)) blocks of 256: 4096 * 256 + 3 elements are 4097 blocks' worth, so the last three elements are
# the second grid-stride trip of threads 0 - 2.  A zero source stride is a broadcast; the (3, 5, 7) cases skip columns of
# the destination (sentinels) and start at element offsets.
@cases_of(R.copy3d_cases)
def test_copy3d(dev, fn, name):
    run(get(fn, name), dev)


# embedding_fwd_kernel: one block of 64 threads per position, D / 64 trips (D = 4: lanes 4 - 63 idle; D = 260: a ragged
# fifth trip).  embedding_bwd_kernel: grid (V, N) of 256 threads; T = 300 is two 256-position chunks (the second one
# partly filled), D = 260 a second column per thread for threads 0 - 3 only, D = 1024 all four columns; the "one-id" table
# row gathers every position, the other rows none (an empty list: total = 0); ids -1 and V + 3 clamp to rows 0 and V - 1.
@cases_of(R.embedding_fwd_cases)
def test_embedding_fwd(dev, fn, name):
    run(get(fn, name), dev)


@cases_of(R.embedding_bwd_cases, R.embedding_bwd_probes)
def test_embedding_bwd(dev, fn, name):
    run(get(fn, name), dev, twice=True)


# ns_bn_fwd: bn_finalize_kernel unless stats_final; then bn_apply4_kernel when C % 4 == 0, ld_y % 4 == 0 and z, y, mean,
# istd, gamma, beta are 16-byte aligned (8 for bf16 z / y) - C = 8 and 132 here, every buffer starts MARGIN = 8 elements into
# its allocation - else bn_apply_kernel: C = 6, and C = 8 with y one element off alignment.  The pre-split pair exists in
# the vector kernel only.  "second-trip": total / 4 = 1 048 578 quads > 4096 blocks * 256 threads.
@cases_of(R.bn_fwd_cases)
def test_bn_fwd(dev, fn, name):
    run(get(fn, name), dev)


def test_bn_fwd_on_column_sums_from_colsum(dev):
    """The column sums that feed bn_fwd, formed by ops.colsum on exact-by-construction z: bit-equal to the float64 sums, and
    bn_fwd on them meets its bound."""
    rows, C = 70, 132
    z = R.unit_values((rows, C), 33, most=6)
    s = torch.zeros(C, dtype=torch.float32, device=dev)
    _ops().colsum(torch.from_numpy(z).to(dev), C, rows, C, s)
    z64 = z.astype(np.float64)
    R.assert_exact_sum(np.abs(z64).sum(0), R.UNIT)
    R.assert_exact_sum((z64 * z64).sum(0), R.UNIT * R.UNIT)
    assert R.bits_equal(s.cpu().numpy(), z64.sum(0).astype(np.float32)).all()
    c = [k for k in R.bn_fwd_cases() if k["name"] == "vector-C132-ld-pair"][0]
    c = dict(c, name="vector-C132-from-colsum", p=dict(c["p"], row_mask=None, count=float(rows)), bufs=dict(c["bufs"]))
    c["bufs"].update(z=(R.framed(z), "f32"), col_sum=(R.framed(s.cpu().numpy()), "f32"),
                     col_sumsq=(R.framed((z64 * z64).sum(0)), "f32"))
    run(c, dev)


# ns_bn_bwd / ns_bn_bwd_finalize: which of bn_bwd_reduce_kernel + bn_bwd_apply_kernel + bn_bwd_bias_kernel ("scalar-"),
# bn_bwd_apply4_kernel + bn_bwd_finalize_kernel ("vector-": the sums are given) and bn_bwd_reduce4_kernel +
# ns_stats_finalize in front of those two ("fallback-") a case takes is restated in pointwise_ref.bn_bwd_form beside the
# table of cases (its docstring has the row-block arithmetic) and asserted in _bn_bwd on the device addresses of the
# operands against the name's prefix.  Each case runs twice, the second time on the work area the first one left.
@cases_of(R.bn_bwd_cases, R.bn_bwd_probes)
def test_bn_bwd(dev, fn, name):
    run(get(fn, name), dev, twice=True)


def test_bn_bwd_scalar_32_blocks_three_times(dev):
    """The scalar form's dbias used to meet in one float atomicAdd per row block; the blocks' partial sums are parked in
    `work` now and added in block order.  Three launches of the 32-block case give the same bits in every output.  (A race
    cannot be made to show: this guards; the proof is that ns_bn_bwd reaches no float atomic.)"""
    c = [k for k in R.bn_bwd_cases() if k["name"] == "scalar-C6-rows2049-none-mask"][0]
    assert R.bn_bwd_row_blocks(c) == (32, 65)
    _BN_WORK.pop(c["name"], None)
    first = run(c, dev, twice=True)
    third = run(c, dev)
    for o in c["outs"]:
        assert R.bits_equal(third[o], first[o]).all(), o


# ns_colsum: colsum4_kernel when round_up(C, 4) <= ld, ld % 4 == 0 and x is aligned to four elements ("vector": grid
# (min(64, ceil(rows / 128)), ceil(C / 64)); (300, 66, 68) ends in a ragged quad that reads two padding elements per row;
# 8193 rows are 64 row blocks of 129 rows), else with `work` colsum_det_kernel ("column": 64 row blocks - of 5 rows, of 2
# rows with the last 29 blocks empty, and at rows = 5 of one row with 59 empty blocks - x ceil(C / 256) column blocks: C = 257
# has a second one), else colsum_kernel.  "atomic": `work` NULL, the float-atomic finish of the vector form, and
# colsum_kernel.  "shifted": an aligned shape one element off alignment.
@cases_of(R.colsum_cases, R.colsum_probes)
def test_colsum(dev, fn, name):
    run(get(fn, name), dev, twice=True)


@cases_of(lambda: R.colsum_cases(random=True))
def test_colsum_random(dev, fn, name):
    run(get(fn, name), dev)


# ns_l1_loss: F >= 256 is l1_loss_kernel<true>, one wave per row, min(512, ceil(rows / 4)) blocks: 2050 rows are more than
# 4 x 512 (rows 2048, 2049: a second trip).  Its quad body needs ldp % 4 == 0, 16-byte aligned pred, ldd % 4 == 0 and an
# aligned dpred: F = 257 / 259 / 1029 with ldp = 260 / 260 / 1032; F = 1029 has 257 quads, one more than 64 lanes x 4 in
# flight (second trip of the quad loop), and F % 4 tail columns.  ldp = 1025 takes the scalar wide body (F = 1025 > 2 x 512:
# a third trip of its eight-deep loop).  F < 256 is l1_loss_kernel<false>, min(256, ..) blocks: the quad body needs F % 4 ==
# 0, aligned operands and an fp32 (or no) gradient - F = 80; 3400 rows x 20 quads = 68 000 items > 65 536 threads: a second
# trip - and F = 78 or a bf16 gradient the flat body.
@cases_of(R.l1_loss_cases, R.l1_loss_probes)
def test_l1_loss(dev, fn, name):
    run(get(fn, name), dev)


@cases_of(lambda: R.l1_loss_cases(random=True))
def test_l1_loss_random(dev, fn, name):
    run(get(fn, name), dev)


# ns_sumsq: min(512, n / 4 / 256 + 1) blocks; n = 1, 3: the tail loop alone; 4, 5: one quad (+ one tail element); 600 001:
# all 512 blocks; 4 200 003: 1 050 000 quads > 512 x 256 x 8, the second trip of the eight-deep loop.  `work`: the ordered
# finish on parked partials; without: one float atomic per block.
@cases_of(R.sumsq_cases, R.sumsq_probes)
def test_sumsq(dev, fn, name):
    run(get(fn, name), dev, twice=True)


@cases_of(lambda: R.sumsq_cases(random=True))
def test_sumsq_random(dev, fn, name):
    run(get(fn, name), dev)


# segment_stats_kernel: one block of 1024 threads per segment - lengths 0 (no trip), 1, 1023 / 1024 / 1025 (either side of
# one trip), 5000 (five trips, the last one partial); segments abut; starts are unaligned.
@cases_of(R.segment_stats_cases)
def test_segment_stats(dev, fn, name):
    run(get(fn, name), dev)


# adam_kernel: min(4096, ceil(n / 256)) blocks; 4096 * 256 + 3 elements: a second grid-stride trip.  gnorm_sq absent: no clip
# factor.  A raised status word: the early return of every thread.
@cases_of(R.adam_cases)
def test_adam(dev, fn, name):
    run(get(fn, name), dev)


# ns_cast2d: cast2d_vec_kernel<transpose> when cols % 4 == 0, both leading dimensions % 4 == 0, rows % 4 == 0 if transposed,
# aligned operands and rows * cols >= 4096 - (64, 64): exactly 4096, one tile; (68, 132): 2 x 3 tiles with edge tiles in both
# directions - else cast2d_kernel (32 x 32 tiles: (5, 7) one partial tile, (33, 65) 2 x 3).
@cases_of(R.cast2d_cases)
def test_cast2d(dev, fn, name):
    run(get(fn, name), dev)


def test_cast_batch(dev):
    """cast2d_batch_kernel: five descriptors in one launch, each equal to its own reference."""
    ops = _ops()
    cases = R.cast_batch_cases()
    ds = [upload(c, dev) for c in cases]
    batch = ops.CastBatch(dev).record(lambda: [_cast2d(c, d) for c, d in zip(cases, ds)])
    assert batch.n == len(cases), "every descriptor qualifies for the batch"
    pre = [download(d) for d in ds]
    for c, g in zip(cases, pre):
        assert all(R.bits_equal(g[o], c["bufs"][o][0]).all() for o in c["outs"]), "recording launches nothing"
    batch.run()
    torch.cuda.synchronize()
    for c, d in zip(cases, ds):
        got = download(d)
        assert R.bits_equal(got["src"], c["bufs"]["src"][0]).all()
        bad = {o: v.why for o, v in R.check(c, got).items() if not v.ok}
        assert not bad, (c["name"], bad)


# split_kernel: min(4096, ceil(n / 256)) blocks; 4096 * 256 + 1: one element of a second trip.
@cases_of(R.split_cases)
def test_split_hi_lo(dev, fn, name):
    run(get(fn, name), dev)


# gru_pointwise_kernel<float | bf16_t>, the four modes as run-time branches; N H = 384 (2 blocks, the second half full)
# and 8448 (33 blocks).
@cases_of(R.gru_pointwise_cases)
def test_gru_pointwise(dev, fn, name):
    run(get(fn, name), dev)


# highway_kernel<T> / act_bwd_kernel<T>: min(4096, ceil(n / 256)) blocks; 4096 * 256 + 5 elements: a second trip.
@cases_of(R.highway_cases)
def test_highway(dev, fn, name):
    run(get(fn, name), dev)


@cases_of(R.act_bwd_cases)
def test_act_bwd(dev, fn, name):
    run(get(fn, name), dev)


# ns_zero_kernel: min(4096, ceil(bytes / 16 / 256)) blocks; ns_zero_many_kernel: 24 buffers per launch, so 25 are two
# launches; the grid's x extent follows the largest buffer, the others' blocks beyond their size do nothing.
@cases_of(R.zero_cases)
def test_zero(dev, fn, name):
    run(get(fn, name), dev)


def test_zz_report():
    """The worst ratios of this run, per kernel and output (the table of the module docstring)."""
    for (op, o, dt), w in sorted(WORST.items()):
        print("  %-14s %-12s %-5s %s %.3f" % (op, o, dt, "error / bound" if dt == "f32" else "neighbours / allowance", w))
