"""ns_stop_token against the float64 contract of tests/stop_token_ref.py (itself checked against autograd by
tests/test_stop_token_ref_cpu.py), through nspeech_amd.ops.

Every case: h is N(0,1) in a slot layout [N, S + 1 or S + 2, D] with junk (7.0) in slot 0 and in the slot behind the last
step, the kernel is pointed at slot 1; dh (same layout, fp32), dw and db start as N(0,1) noise to show the `+=`; logits,
acc and stop_steps sit between sentinels.  The reference is computed from the values the kernel reads: for bf16 h the
rounded values, widened to float64.

Bounds, fixed before the kernel ran.  u = 2^-24, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical
Algorithms, section 3.1: k roundings in a sum, in any order):
  z      |z - z64| <= ez := gamma_{D+2} (sum_d |h_d w_d| + |b|)     D/64 fused products per lane, the wave tree, + b
  dz     dz = c f(z) with |f'| <= max(1, pos_weight) / 4 (the sigmoid's slope), so
         |dz - dz64| <= edz := c max(1, pos_weight) ez / 4 + 16 u |dz64|      (the second term: expf, the division, c)
  dh     |increment - dz64 w_d| <= edz |w_d| + u |dz64 w_d| + u |dh after|   (one fused multiply-add)
  dw     |increment - dw64_d| <= gamma_{NS+2} sum_{n,s} |dz h_d| + sum_{n,s} edz |h_d| + u |dw after|
  db     |increment - db64|   <= gamma_{NS+2} sum |dz| + sum edz + u |db after|
  L_stop, acc[1] and dz itself (read back as dh / w at the largest |w| from a launch on a cleared dh): 1e-5 relative,
  the bound tests/test_guided_attn_contract_gpu.py holds its scalars to.
Synthesis form: the expected stop steps come from the float64 logits, after the test has asserted that no logit up to and
including each row's first crossing lies within 100 ez of the threshold."""
import functools

import numpy as np
import pytest
import torch

import stop_token_ref as R

pytestmark = pytest.mark.gpu

MARGIN = 8
SENT = -12345.0
JUNK = 7.0
U = 2.0 ** -24


def gamma(k):
    return k * U / (1.0 - k * U)


SHAPES = {                      # name: N, S, D, slots behind S, out_steps, pos_weight, grad_scale
    "w64": (3, 4, 64, 1, [4, 3, 1], 1.0, 1.0),              # one value per lane
    "w1024": (2, 7, 1024, 2, [1, 7], 5.0, 0.7),             # four 16-byte loads per lane
    "w192": (5, 33, 192, 1, None, 5.0, 2.5),                # three values per lane: no 16-byte loads; 6 workgroups
    "one": (1, 1, 64, 2, [1], 1.0, 1.0),
    "clamp": (3, 4, 64, 2, [0, 9, 2], 1.0, 1.0),            # out_steps outside [1, S] are clamped
}


def _round_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    """Inputs (NumPy, never modified afterwards) and the float64 expectation, computed once per case."""
    N, S, D, extra, steps, pw, gs = SHAPES[name]
    slots = S + extra
    rng = np.random.RandomState(len(name) * 131 + D + (7 if dtype == "bf16" else 0))
    h = np.full((N, slots, D), JUNK, np.float32)
    h[:, 1:S + 1] = rng.standard_normal((N, S, D)).astype(np.float32)
    if dtype == "bf16":
        h = _round_bf16(h)
    w = (rng.standard_normal(D) * (1.5 / np.sqrt(D))).astype(np.float32)
    b = np.asarray([0.3], np.float32)
    dh = rng.standard_normal((N, slots, D)).astype(np.float32)
    dw = rng.standard_normal(D).astype(np.float32)
    db = rng.standard_normal(1).astype(np.float32)
    ref = R.stop_token(h[:, 1:S + 1], w, b, steps, pos_weight=pw, grad_scale=gs)
    for a in (h, w, b, dh, dw, db):
        a.setflags(write=False)
    return dict(name=name, dtype=dtype, N=N, S=S, D=D, slots=slots, steps=steps, pw=pw, gs=gs, h=h, w=w, b=b, dh=dh, dw=dw,
                db=db, ref=ref)


def launch(c, dev, train=True, with_grad=True, clear_dh=False, threshold=None, logits=True):
    from nspeech_amd import ops
    N, S, D, slots = c["N"], c["S"], c["D"], c["slots"]
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)          # a copy: the cached inputs are read-only
    h = t(c["h"]).to(torch.bfloat16) if c["dtype"] == "bf16" else t(c["h"])
    w, b = t(c["w"]), t(c["b"])
    grad = train and with_grad
    dh = (torch.zeros(N, slots, D, device=dev) if clear_dh else t(c["dh"])) if grad else None
    dw, db = (t(c["dw"]), t(c["db"])) if grad else (None, None)
    lg = torch.full((MARGIN + N * S + MARGIN,), SENT, dtype=torch.float32, device=dev)
    acc = torch.full((MARGIN + 2 + MARGIN,), SENT, dtype=torch.float32, device=dev)
    st = torch.full((MARGIN + N + MARGIN,), -77, dtype=torch.int32, device=dev)
    work = torch.full((ops.stop_token_work_floats(N, S, D) + MARGIN,), SENT, dtype=torch.float32, device=dev)
    steps = None if (c["steps"] is None or not train) else t(np.asarray(c["steps"], np.int32))
    ops.stop_token(N, S, D, h, slots * D, D, w, b, work, h_off=D, logits=lg[MARGIN:] if logits else None,
                   out_steps=steps, pos_weight=c["pw"], grad_scale=c["gs"], dh=dh, dh_off=D, dh_sn=slots * D, dh_ss=D,
                   dw=dw, db=db, acc=acc if train else None, acc_off=MARGIN, threshold=threshold,
                   stop_steps=st[MARGIN:] if threshold is not None else None)
    torch.cuda.synchronize()
    assert (work[-MARGIN:] == SENT).all(), "work written behind ns_stop_token_work_floats"
    assert torch.equal(h.float().cpu(), torch.from_numpy(np.array(c["h"]))), "h was written"
    g = lambda x: None if x is None else x.cpu().numpy()
    return dict(dh=g(dh), dw=g(dw), db=g(db), logits=g(lg), acc=g(acc), steps=g(st))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def z_bound(c):
    N, S, D = c["N"], c["S"], c["D"]
    h = c["h"][:, 1:S + 1].astype(np.float64)
    return gamma(D + 2) * (np.abs(h * c["w"].astype(np.float64)).sum(axis=2) + abs(float(c["b"][0])))


def check_logits(c, got):
    N, S = c["N"], c["S"]
    lg = got["logits"]
    assert (lg[:MARGIN] == SENT).all() and (lg[MARGIN + N * S:] == SENT).all(), "logits written outside [N, S]"
    z = lg[MARGIN:MARGIN + N * S].reshape(N, S).astype(np.float64)
    ratio = np.abs(z - c["ref"]["z"]) / z_bound(c)
    print("%s/%s: z worst |got - ref| / bound = %.3f" % (c["name"], c["dtype"], ratio.max()))
    assert ratio.max() <= 1.0


def check_training(c, got, got0):
    N, S, D, ref = c["N"], c["S"], c["D"], c["ref"]
    h = c["h"][:, 1:S + 1].astype(np.float64)
    w = c["w"].astype(np.float64)
    acc = got["acc"]
    assert (acc[:MARGIN] == SENT).all() and (acc[MARGIN + 2:] == SENT).all(), "acc written outside its two words"
    el = abs(acc[MARGIN] - ref["loss"]) / ref["loss"]
    es = abs(acc[MARGIN + 1] - ref["step_error"]) / max(ref["step_error"], 1e-30)
    assert ref["step_error"] > 0.0 or acc[MARGIN + 1] == 0.0
    # dz from the launch on a cleared dh: dh = dz w rounded once, at the column of the largest |w|
    k = int(np.abs(w).argmax())
    dz = got0["dh"][:, 1:S + 1, k].astype(np.float64) / w[k]
    ed = (np.abs(dz - ref["dz"]) / np.abs(ref["dz"])).max()
    print("%s/%s: L_stop %.2e  step error %.2e  dz %.2e (relative; bound 1e-5)" % (c["name"], c["dtype"], el, es, ed))
    assert el <= 1e-5 and es <= 1e-5 and ed <= 1e-5
    ez = z_bound(c)
    edz = c["gs"] / (N * S) * max(1.0, c["pw"]) * ez / 4 + 16 * U * np.abs(ref["dz"])
    # dh: everything outside the N * S rows keeps its bits, the rows move by dz w
    after = got["dh"]
    same = bits(after) == bits(c["dh"])
    rows = np.zeros(after.shape, bool)
    rows[:, 1:S + 1] = True
    assert same[~rows].all(), "%d elements of dh outside the rows changed" % int((~same[~rows]).sum())
    inc = after[:, 1:S + 1].astype(np.float64) - c["dh"][:, 1:S + 1].astype(np.float64)
    bound = edz[:, :, None] * np.abs(w) + U * np.abs(ref["dh"]) + U * np.abs(after[:, 1:S + 1])
    r_dh = (np.abs(inc - ref["dh"]) / bound).max()
    assert (inc != 0.0).mean() > 0.5, "dh was not written"
    inc_w = got["dw"].astype(np.float64) - c["dw"].astype(np.float64)
    bound_w = (gamma(N * S + 2) * np.einsum("ns,nsd->d", np.abs(ref["dz"]), np.abs(h)) + np.einsum("ns,nsd->d", edz, np.abs(h))
               + U * np.abs(got["dw"]))
    r_dw = (np.abs(inc_w - ref["dw"]) / bound_w).max()
    inc_b = float(got["db"][0]) - float(c["db"][0])
    bound_b = gamma(N * S + 2) * np.abs(ref["dz"]).sum() + edz.sum() + U * abs(float(got["db"][0]))
    r_db = abs(inc_b - ref["db"]) / bound_b
    print("%s/%s: worst |got - ref| / bound: dh %.3f  dw %.3f  db %.3f" % (c["name"], c["dtype"], r_dh, r_dw, r_db))
    assert r_dh <= 1.0 and r_dw <= 1.0 and r_db <= 1.0
    assert np.abs(inc_w).max() > 0.0 and inc_b != 0.0


CASES = [(n, d) for n in SHAPES for d in ("fp32", "bf16")]


@pytest.mark.parametrize("name, dtype", CASES)
def test_training_form_matches_the_float64_reference(dev, name, dtype):
    c = case(name, dtype)
    got = launch(c, dev)
    got0 = launch(c, dev, clear_dh=True)
    check_logits(c, got)
    check_training(c, got, got0)
    again = launch(c, dev)              # the same inputs: the same bits, in every output
    for k in ("dh", "dw", "db", "logits", "acc"):
        assert bits(got[k]).tobytes() == bits(again[k]).tobytes(), "%s differs between two launches" % k
    assert (got["steps"] == -77).all(), "stop_steps written without being asked for"


def test_steps_outside_the_range_are_clamped(dev):
    c = case("clamp", "fp32")
    assert c["ref"]["y"].tolist() == [[1, 1, 1, 1], [0, 0, 0, 1], [0, 1, 1, 1]]


def test_scores_without_gradients_and_without_logits(dev):
    c = case("w192", "fp32")
    full = launch(c, dev)
    got = launch(c, dev, with_grad=False, logits=False)
    assert (got["logits"] == SENT).all()
    assert bits(got["acc"]).tobytes() == bits(full["acc"]).tobytes()        # the scores do not depend on dh


def test_grad_scale_zero_leaves_every_gradient_bit(dev):
    c = dict(case("w1024", "fp32"), gs=0.0)
    neg = np.array(c["dh"])
    neg[0, 1, :8] = -0.0                # the sign of a zero survives too
    c["dh"] = neg
    got = launch(c, dev)
    for k in ("dh", "dw", "db"):
        assert bits(got[k]).tobytes() == bits(c[k]).tobytes(), k
    assert abs(got["acc"][MARGIN] - c["ref"]["loss"]) <= 1e-5 * c["ref"]["loss"]


def _synthesis_case(name, dtype, t, spread):
    """w scaled (and b set) so that the rows cross the threshold at different steps."""
    c = dict(case(name, dtype))
    c["w"] = (c["w"] * spread).astype(np.float32)
    c["b"] = np.asarray([-0.5], np.float32)
    c["ref"] = R.stop_token(c["h"][:, 1:c["S"] + 1], c["w"], c["b"])
    thr = float(np.float32(R.threshold_logit(t)))       # the float the parameter block holds
    z, ez = c["ref"]["z"], z_bound(c)
    want = R.stop_steps(z, thr)
    for n in range(c["N"]):
        upto = int(want[n])             # steps 0 .. S^_n - 1: the ones that decide
        gap = np.abs(z[n, :upto] - thr) / ez[n, :upto]
        assert gap.min() > 100.0, "row %d: a deciding logit lies within %.1f bounds of the threshold" % (n, gap.min())
    return c, thr, want


@pytest.mark.parametrize("name, dtype, t, spread", [("w192", "fp32", 0.6, 2.0), ("w192", "bf16", 0.9, 1.0),
                                                    ("w1024", "fp32", 0.6, 2.0), ("w64", "bf16", 0.5, 2.0)])
def test_synthesis_form_finds_the_first_crossing(dev, name, dtype, t, spread):
    c, thr, want = _synthesis_case(name, dtype, t, spread)
    N, S = c["N"], c["S"]
    if name == "w192":
        assert len(set(want.tolist())) >= 3, want            # rows stop at different steps
    got = launch(c, dev, train=False, threshold=t)
    check_logits(c, got)
    st = got["steps"]
    assert (st[:MARGIN] == -77).all() and (st[MARGIN + N:] == -77).all(), "stop_steps written outside [N]"
    print("%s/%s: stop steps %s" % (name, dtype, st[MARGIN:MARGIN + N].tolist()))
    assert st[MARGIN:MARGIN + N].tolist() == want.tolist()
    assert (got["acc"] == SENT).all(), "acc written in the synthesis form"
    again = launch(c, dev, train=False, threshold=t)
    assert got["steps"].tobytes() == again["steps"].tobytes() and bits(got["logits"]).tobytes() == bits(again["logits"]).tobytes()


def test_hand_made_logits(dev):
    """z = h[.., 0] exactly (w = e_0, b = 0): no step over the threshold -> S; step 0 over -> 1; a logit exactly equal to
    the threshold does not count; the first crossing decides."""
    t = 0.7
    thr = np.float32(R.threshold_logit(t))
    N, S, D = 4, 5, 64
    h = np.zeros((N, S + 1, D), np.float32)
    h[:, 1:, 0] = thr - np.float32(1.0)
    h[1, 1, 0] = np.nextafter(thr, np.float32(np.inf))
    h[2, 4, 0] = thr
    h[3, 3, 0] = thr + np.float32(0.5)
    h[3, 5, 0] = thr + np.float32(2.0)
    w = np.zeros(D, np.float32)
    w[0] = 1.0
    c = dict(name="hand", dtype="fp32", N=N, S=S, D=D, slots=S + 1, steps=None, pw=1.0, gs=1.0, h=h, w=w,
             b=np.zeros(1, np.float32))
    got = launch(c, dev, train=False, threshold=t)
    z = got["logits"][MARGIN:MARGIN + N * S].reshape(N, S)
    assert bits(z).tobytes() == bits(h[:, 1:, 0]).tobytes()
    assert got["steps"][MARGIN:MARGIN + N].tolist() == [5, 1, 5, 3] == R.stop_steps(z, float(thr)).tolist()
