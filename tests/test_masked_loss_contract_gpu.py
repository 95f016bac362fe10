"""ns_l1_loss_masked through the C ABI against the float64 contract of tests/masked_loss_ref.py, on the smallest shapes at
which each form of the kernel can go wrong: F 1025 (a wave per row, quads plus one tail column, target rows only 4-byte
aligned), 257, 256, 80 (quads of narrow rows), 78 and 16 (flat), leading dimensions that are no multiple of 4 (the scalar
fall-backs), an fp32, a bf16 and no gradient, n_prio 0, inside a quad and F, lengths 0, negative, above T, NULL and 1,
Tacotron-1's mel layout, and shapes with more rows than one pass of the grid.

Exact: the gradient is float32(sign * w) or its bf16 rounding bit for bit, zeros on the padded frames included; the buffer
is prefilled with a sentinel everywhere, so one comparison of the whole buffer shows that the rows outside [padl, padl + T),
the columns >= F and the margins keep their bits and that a stale value on a padded frame becomes zero; the acc words
beside the two sums keep their bits, and the sums replace the prefill.  Sums of multiples of 1/4 and the one-hot probes are
exact in any order and compared bit for bit.

Random sums: |acc - float64 sum| <= 1.01 (1 + depth) 2^-24 sum |d| (masked_loss_ref.sum_bound), where depth is the longest
chain of adds between a term and the result: a thread's own terms in loop order, the wave's butterfly (6), the
workgroup's four waves in index order (4), and in the second launch a thread's at most 4 partials, 6 and 4 again; one more
2^-24 for the rounding of d = pred - target.  At (3, 20, 1025) that is 1.01 x 53 x 2^-24 = 3.2e-6 relative.

Every case runs twice on fresh buffers and one scratch that is never cleared (prefilled with NaN): equal bits."""
import ctypes

import numpy as np
import pytest
import torch

import masked_loss_ref as R
from masked_loss_ref import MARGIN as M

pytestmark = pytest.mark.gpu

TDT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _launch(c, dev):
    from nspeech_amd import ops
    p = c["p"]
    d = dict(pred=torch.from_numpy(c["pred"]).to(dev), target=torch.from_numpy(c["target"]).to(dev),
             acc=torch.from_numpy(c["acc"]).to(dev))
    if c["ddt"]:
        d["dpred"] = torch.from_numpy(c["dpred"]).to(TDT[c["ddt"]]).to(dev)
    lengths = None if c["lengths"] is None else torch.tensor(c["lengths"], dtype=torch.int32, device=dev)
    need = ops.l1_loss_masked_work_floats(p["N"], p["T"], p["F"])
    assert 0 < need <= 4096
    work = torch.full((need,), float("nan"), device=dev)
    ops.l1_loss_masked(d["pred"][M:], p["ldp"], d["target"][M:], d["dpred"][M:] if c["ddt"] else None, p["ldd"], p["N"], p["T"],
                       p["P"], p["padl"], p["F"], p["n_prio"], p["w_all"], p["w_prio"], lengths, d["acc"], work,
                       acc_off=p["acc_off"])
    torch.cuda.synchronize()
    got = {k: v.float().cpu().numpy() for k, v in d.items()}
    assert R.bits_equal(got["pred"], c["pred"]).all() and R.bits_equal(got["target"], c["target"]).all(), "an input was written"
    return got


def _run(c, dev):
    got = _launch(c, dev)
    bad = R.check(c, got["acc"], got.get("dpred"))
    if not c["exact"]:
        print("  %-34s sum error / bound %.3f" % (c["name"], c["worst"]))
    assert not bad, (c["name"], bad)
    again = _launch(c, dev)
    for k in ("acc", "dpred"):
        if k in got:
            assert R.bits_equal(again[k], got[k]).all(), (c["name"], k, "a second launch differs")


@pytest.mark.parametrize("name", R.case_names())
def test_exact_cases(dev, name):
    _run(R.build(name), dev)


@pytest.mark.parametrize("name", R.probe_names())
def test_one_hot_probes(dev, name):
    _run(R.build(name), dev)


@pytest.mark.parametrize("name", R.case_names(random=True))
def test_random_sums(dev, name):
    _run(R.build(name), dev)


def test_small_integer_sums_are_exact(dev):
    """pred - target = 1 on every real frame and 3 on every padded one: acc[0] = C F and acc[1] = C n_prio exactly."""
    c = R.build("wide-1025-f32")
    p = c["p"]
    N, T, F = p["N"], p["T"], p["F"]
    _, pred, _ = R.views(c)
    fr = R.frames_of(c["lengths"], N, T)
    live = np.arange(T)[None, :] < fr[:, None]
    c["target"] = R.framed(pred - np.where(live, 1.0, 3.0)[:, :, None].astype(np.float32))
    got = _launch(c, dev)
    o = p["acc_off"]
    assert got["acc"][o] == float(fr.sum() * F) and got["acc"][o + 1] == float(fr.sum() * p["n_prio"])
    assert not R.check(c, got["acc"], got["dpred"])


def test_null_operands_are_errors(dev):
    from nspeech_amd import _lib as L
    from nspeech_amd import ops
    c = R.build("narrow-16")
    p = c["p"]
    t = {k: torch.from_numpy(c[k]).to(dev) for k in ("pred", "target", "acc", "dpred")}
    work = torch.zeros(64, device=dev)

    def call(**null):
        q = L.struct("ns_l1_loss_masked_params")
        ops._fill(q, pred=ops.ptr(t["pred"], M), ldp=p["ldp"], target=ops.ptr(t["target"], M), dpred=ops.ptr(t["dpred"], M),
                  dpred_dtype=0, ldd=p["ldd"], N=p["N"], T=p["T"], P=p["P"], padl=p["padl"], F=p["F"], n_prio=p["n_prio"],
                  w_all=p["w_all"], w_prio=p["w_prio"], lengths=None, acc=ops.ptr(t["acc"], M), work=ops.ptr(work))
        for k, v in null.items():
            setattr(q, k, v)
        return L.lib().ns_l1_loss_masked(ctypes.byref(q), None)

    assert call() == 0
    for k in ("pred", "target", "acc", "work"):
        assert call(**{k: None}) == -1, k
        assert k.encode() in L.lib().ns_last_error()
    assert L.lib().ns_l1_loss_masked(None, None) == -1
    assert call(P=p["padl"] + p["T"] - 1) == -1 and call(ldp=p["F"] - 1) == -1 and call(dpred_dtype=7) == -1
    torch.cuda.synchronize()
