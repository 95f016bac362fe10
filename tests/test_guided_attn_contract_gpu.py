"""ns_guided_attention against the float64 contract of tests/guided_attn_ref.py (itself checked against autograd by
tests/test_guided_attn_ref_cpu.py), through nspeech_amd.ops.

Every case: `align` is random and row-normalised over each row's T_n positions, with junk (7.0) in slot 0, in the steps
>= S_n and in the columns >= T_n, so a kernel that reads outside the valid region shows in G_n / F_n; `da0` starts as
N(0,1) noise, and everything of it outside the valid region must keep its bits.  row_out and acc sit between sentinels.

Bounds (fixed before the kernel ran):
  increment   |got - ref| <= 2e-6 * grad_scale / (N S_n T_n) + 1.2e-7 * |da0 after|
              first term: the fp32 evaluation of W (measured on the CPU against float64, T up to 256, S up to 1000: within
              3.6e-7 at sigma 0.2, 2.3e-7 at 0.4, 6.7e-7 at 0.1) with room for the device's expf - a fast-math exp misses
              it; second term: the rounding of the fp32 add into a noise value of size ~1 (2^-24 = 6e-8, twice)
  G_n, F_n, L_att, focus   1e-5 relative
Worst on the MI355X (printed by every test, `pytest -s`): increment 0.41 / 0.49 / 0.45 of the bound (edges / bench_row /
rows33; the add's rounding term is what is used, W itself is far inside 2e-6), scores 1.1e-7 relative."""
import functools

import numpy as np
import pytest
import torch

import guided_attn_ref as R

pytestmark = pytest.mark.gpu

MARGIN = 8
SENT = -12345.0
JUNK = 7.0


def _lengths(name):
    if name == "edges":         # padding columns, short rows, length-1 edges
        return dict(N=3, S=7, Ti=13, Tia=16, Tn=[13, 5, 1], Sn=[7, 3, 1], sigma=0.2, scale=1.0)
    if name == "bench_row":     # the benchmark's per-row size: more steps than a workgroup has waves, three lane passes
        return dict(N=2, S=200, Ti=160, Tia=160, Tn=[160, 97], Sn=[200, 131], sigma=0.4, scale=2.5)
    if name == "rows33":        # more than 32 rows
        rng = np.random.RandomState(33)
        return dict(N=33, S=2, Ti=9, Tia=16, Tn=rng.randint(1, 10, 33).tolist(), Sn=rng.randint(1, 3, 33).tolist(),
                    sigma=0.1, scale=0.7)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name, with_steps=True):
    """Inputs (NumPy, never modified afterwards) and the float64 expectation, computed once per case."""
    c = _lengths(name)
    N, S, Tia = c["N"], c["S"], c["Tia"]
    Tn, Sn = np.asarray(c["Tn"], np.int32), np.asarray(c["Sn"], np.int32)
    if not with_steps:
        Sn = np.full(N, S, np.int32)
    rng = np.random.RandomState(len(name) * 101 + 7)
    align = np.full((N, S + 1, Tia), JUNK, np.float32)
    for n in range(N):
        a = rng.uniform(0.02, 1.0, size=(Sn[n], Tn[n]))
        align[n, 1:Sn[n] + 1, :Tn[n]] = (a / a.sum(axis=1, keepdims=True)).astype(np.float32)
    da0 = rng.standard_normal((N, S + 1, Tia)).astype(np.float32)
    inner = np.where(align[:, 1:] == JUNK, 0.0, align[:, 1:].astype(np.float64))       # the reference sees the valid part
    ref = R.guided_attention(inner, Tn, Sn, sigma=c["sigma"], weight=c["scale"])
    valid = np.zeros((N, S + 1, Tia), bool)
    for n in range(N):
        valid[n, 1:Sn[n] + 1, :Tn[n]] = True
    for a in (align, da0, valid):
        a.setflags(write=False)
    return dict(c, Tn=Tn, Sn=Sn, with_steps=with_steps, align=align, da0=da0, ref=ref, valid=valid)


def launch(c, dev, with_da0=True):
    from nspeech_amd import ops
    N = c["N"]
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)          # a copy: the cached inputs are read-only
    align, da0 = t(c["align"]), (t(c["da0"]) if with_da0 else None)
    row = torch.full((MARGIN + 2 * N + MARGIN,), SENT, dtype=torch.float32, device=dev)
    acc = torch.full((MARGIN + 2 + MARGIN,), SENT, dtype=torch.float32, device=dev)
    ops.guided_attention(N, c["S"], c["Tia"], t(c["Tn"]), t(c["Sn"]) if c["with_steps"] else None, c["sigma"], align, da0,
                         c["scale"], row[MARGIN:], acc, MARGIN)
    torch.cuda.synchronize()
    out = dict(align=align.cpu().numpy(), da0=None if da0 is None else da0.cpu().numpy(), row=row.cpu().numpy(),
               acc=acc.cpu().numpy())
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def check_scores(c, got):
    N, ref = c["N"], c["ref"]
    row, acc = got["row"], got["acc"]
    assert (row[:MARGIN] == SENT).all() and (row[MARGIN + 2 * N:] == SENT).all(), "row_out written outside [N][2]"
    assert (acc[:MARGIN] == SENT).all() and (acc[MARGIN + 2:] == SENT).all(), "acc written outside its two words"
    G, F = row[MARGIN:MARGIN + 2 * N:2].astype(np.float64), row[MARGIN + 1:MARGIN + 2 * N:2].astype(np.float64)
    eg = np.abs(G - ref["G"]) / np.abs(ref["G"]).clip(1e-30)
    ef = np.abs(F - ref["F"]) / ref["F"]
    # a row whose guided loss is exactly zero (one step, one position: W = 0) must come out as zero
    assert (G[ref["G"] == 0.0] == 0.0).all()
    eg = eg[ref["G"] > 0.0]
    el = abs(acc[MARGIN] - ref["loss"]) / ref["loss"]
    eo = abs(acc[MARGIN + 1] - ref["focus"]) / ref["focus"]
    print("%s: G_n %.2e  F_n %.2e  L_att %.2e  focus %.2e (relative; bound 1e-5)"
          % (c.get("label", ""), eg.max() if eg.size else 0.0, ef.max(), el, eo))
    assert (eg <= 1e-5).all() and (ef <= 1e-5).all() and el <= 1e-5 and eo <= 1e-5
    assert bits(got["align"]).tobytes() == bits(c["align"]).tobytes(), "align was written"


def check_increment(c, got):
    N, ref, valid = c["N"], c["ref"], c["valid"]
    after = got["da0"]
    same = bits(after) == bits(c["da0"])
    assert same[~valid].all(), "%d elements outside the valid region changed" % int((~same[~valid]).sum())
    inc = after.astype(np.float64) - c["da0"].astype(np.float64)
    want = np.zeros_like(inc)
    want[:, 1:] = ref["dalign"]
    per_row = 2e-6 * c["scale"] / (N * c["Sn"].astype(np.float64) * c["Tn"].astype(np.float64))
    bound = per_row[:, None, None] + 1.2e-7 * np.abs(after.astype(np.float64))
    ratio = (np.abs(inc - want) / bound)[valid]
    print("increment: worst |got - ref| / bound = %.3f over %d elements" % (ratio.max(), ratio.size))
    assert ratio.max() <= 1.0
    assert (inc[valid] != 0.0).mean() > 0.5, "the valid region was not written"


@pytest.mark.parametrize("name", ["edges", "bench_row", "rows33"])
def test_kernel_matches_the_float64_reference(dev, name):
    c = case(name)
    got = launch(c, dev)
    check_scores(c, got)
    check_increment(c, got)
    again = launch(c, dev)              # the same inputs: the same bits, in every output
    for k in ("da0", "row", "acc"):
        assert bits(got[k]).tobytes() == bits(again[k]).tobytes(), "%s differs between two launches" % k


def test_null_out_steps_means_every_step(dev):
    c = case("edges", with_steps=False)
    assert c["Sn"].tolist() == [7, 7, 7]
    got = launch(c, dev)
    check_scores(c, got)
    check_increment(c, got)


def test_null_da0_writes_only_the_scores(dev):
    c = case("edges")
    got = launch(c, dev, with_da0=False)
    check_scores(c, got)                # includes: sentinels around row_out / acc intact, align bit-unchanged
    with_grad = launch(c, dev)
    assert bits(got["row"]).tobytes() == bits(with_grad["row"]).tobytes()       # the scores do not depend on da0
    assert bits(got["acc"]).tobytes() == bits(with_grad["acc"]).tobytes()
