"""Proof of tests/pointwise_ref.py on the CPU: every restatement against an independent formulation (torch float64,
autograd for the backward halves), the running-error bounds against float32 emulations in several association orders with
and without FMA (within 1 x the bound; the GPU test allows 2 x), the exactness conditions, the bf16 store rule on the
references alone, and the mutants: float32 emulations of WRONG kernels, each of which the comparison that the GPU module
uses rejects on the GPU module's own inputs.  `pytest -s` prints the worst ratios."""
import numpy as np
import pytest
import torch

import pointwise_ref as R
from pointwise_ref import MARGIN, F32


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float64))


def logical(c, name, n=None, off=MARGIN):
    x = c["bufs"][name][0]
    return x[off:len(x) - MARGIN if n is None else off + n]


def find(cases, name):
    got = [c for c in cases if c["name"] == name]
    assert len(got) == 1, name
    return got[0]


# ------------------------------------------------------------------------------------------------------ emulation
def emulate(c, A=None, mut=None):
    """What a float32 kernel that evaluates the contract with arithmetic A leaves in every output buffer; `mut`: a wrong
    kernel.  The reductions' inputs are exact by construction, so their float64 sums ARE what float32 gives."""
    A = A or F32()
    op, p = c["op"], c["p"]
    if op == "bn_fwd":
        r = R.compute_bn_fwd(c, A, mut)
        got = {}
        for name in ("mean_out", "istd_out", "moving_mean", "moving_var"):
            if name in r and name in c["outs"]:
                got[name] = c["bufs"][name][0].copy()
                got[name][MARGIN:MARGIN + p["C"]] = A.out(r[name])
        y32 = np.broadcast_to(A.out(r["y_value"]), (p["rows"], p["C"])).reshape(-1)
        if "y" in c["outs"]:
            idx = (p["y_off"] + np.arange(p["rows"])[:, None] * (p["ld_y"] or p["C"]) + np.arange(p["C"])[None, :]).reshape(-1)
            got["y"] = c["bufs"]["y"][0].copy()
            got["y"][idx] = R.store(y32, c["bufs"]["y"][1])
            y32 = got["y"][idx]
        if "y_hi" in c["outs"]:
            for name, v in zip(("y_hi", "y_lo"), R.split_hi_lo(y32, mut)):
                got[name] = c["bufs"][name][0].copy()
                got[name][MARGIN:MARGIN + y32.size] = v
        return got
    if op == "adam":
        got = {o: c["bufs"][o][0].copy() for o in c["outs"]}
        if p["raised"] is not None and mut != "ignore_status":
            got["skipped"][MARGIN] = 1.0
            return got
        got.update(R.flat_emulate(c, R.compute_adam(c, A, mut), p["n"], A))
        if "shadow" in got:
            w = got["p"][MARGIN:MARGIN + p["n"]]
            got["shadow"][MARGIN:MARGIN + p["n"]] = R.trunc_bf16(w) if mut == "truncate" else R.rne_bf16(w)
        return got
    if op == "gru_pointwise":
        return R.scatter_rows(c, R.compute_gru_pointwise(c, A, mut), A)
    if op == "highway":
        return R.flat_emulate(c, R.compute_highway(c, A, mut), p["n"], A)
    if op == "act_bwd":
        return R.flat_emulate(c, R.compute_act_bwd(c, A, mut), p["rows"] * p["C"], A)
    if op == "bn_bwd":
        return R.emulate_bn_bwd(c, A, mut)
    exp = R.EXPECT[op](c, mut) if mut else R.expect(c)
    return {o: R.store(v.astype(np.float32), c["bufs"][o][1]) for o, (v, e) in exp.items() if o in c["outs"]}


ARITHMETICS = [F32(order, fma) for order in range(8) for fma in (False, True)]
WORST = {}


def small(cases, most=70000):
    return [c for c in cases if max(len(b[0]) for b in c["bufs"].values()) <= most]


# ------------------------------------------------------------------------------------------------------ roundings
def test_roundings_match_torch():
    x = np.concatenate([R.rounding_values(40000, 1), R.rounding_values(1000, 2, bf16=True)])
    t = torch.from_numpy(x)
    hi = t.to(torch.bfloat16).float()
    assert np.array_equal(R._u32(R.rne_bf16(x)), R._u32(hi.numpy()))
    lo = (t - hi).to(torch.bfloat16).float()
    h, l = R.split_hi_lo(x)
    assert np.array_equal(R._u32(l), R._u32(lo.numpy())) and np.array_equal(R._u32(h), R._u32(hi.numpy()))
    assert np.array_equal((t - hi).double().numpy(), x.astype(np.float64) - hi.double().numpy()), "x - hi is exact in fp32"
    # the inputs hold what the contract asks: ties both ways, their fp32 neighbours, -0.0, both signs, 2^-30 .. 2^30
    up, down = R.rne_bf16(x) > x, R.rne_bf16(x) < x
    tie = (R._u32(x) & 0xFFFF) == 0x8000
    assert (tie & up).sum() > 100 and (tie & down).sum() > 100
    assert (((R._u32(x) & 0xFFFF) == 0x8001).sum() > 100) and (((R._u32(x) & 0xFFFF) == 0x7FFF).sum() > 100)
    assert np.signbit(x[x == 0]).any() and (x < 0).any() and np.abs(x[x != 0]).min() <= 2.0 ** -29 and np.abs(x).max() >= 2.0 ** 29
    assert (R.trunc_bf16(x) != R.rne_bf16(x)).any()


# ------------------------------------------------------------------------------------------------------ independent formulations
def test_copy_cast_split_against_torch():
    for c in R.copy3d_cases():
        p = c["p"]
        if p["Cc"] > 1000:
            continue
        tdt = {"f32": torch.float32, "bf16": torch.bfloat16}
        src = torch.from_numpy(c["bufs"]["src"][0]).to(tdt[c["bufs"]["src"][1]])
        dst = torch.from_numpy(c["bufs"]["dst"][0].copy()).to(tdt[c["bufs"]["dst"][1]])
        sv = torch.as_strided(src, (p["I"], p["J"], p["Cc"]), (p["src_strides"][0], p["src_strides"][1], 1), p["src_off"])
        dv = torch.as_strided(dst, (p["I"], p["J"], p["Cc"]), (p["dst_strides"][0], p["dst_strides"][1], 1), p["dst_off"])
        dv.copy_((dv.float() + sv.float()).to(dst.dtype) if p["accumulate"] else sv.to(dst.dtype))
        want, _ = R.expect(c)["dst"]
        assert np.array_equal(R._u32(dst.float().numpy()), R._u32(want)), c["name"]
    for c in R.cast2d_cases() + R.cast_batch_cases():
        p = c["p"]
        src = torch.from_numpy(c["bufs"]["src"][0])
        m = torch.as_strided(src, (p["rows"], p["cols"]), (p["ld_src"], 1), p["src_off"])
        m = m.t() if p["transpose"] else m
        exp = R.expect(c)
        hi = m.to(torch.bfloat16)
        for name, want in (("dst", m.to(torch.bfloat16).float() if c["bufs"].get("dst", (0, ""))[1] == "bf16" else m),
                           ("dst_hi", hi.float()), ("dst_lo", (m - hi.float()).to(torch.bfloat16).float())):
            if name in exp:
                got = torch.as_strided(torch.from_numpy(exp[name][0]), tuple(m.shape), (p["ld_dst"], 1), p["dst_off"])
                assert np.array_equal(R._u32(got.numpy()), R._u32(want.contiguous().numpy())), (c["name"], name)
                rest = exp[name][0].copy()
                torch.as_strided(torch.from_numpy(rest), tuple(m.shape), (p["ld_dst"], 1), p["dst_off"]).fill_(R.SENT)
                assert (rest == R.SENT).all(), "everything else keeps the sentinel"


def test_embedding_against_torch():
    for c in R.embedding_fwd_cases():
        p = c["p"]
        ids = torch.from_numpy(c["bufs"]["ids"][0]).long().clamp(0, p["V"] - 1)
        table = torch.from_numpy(c["bufs"]["table"][0][p["table_off"]:p["table_off"] + p["V"] * p["D"]]).reshape(p["V"], p["D"])
        want = torch.full((p["N"], p["P"], p["D"]), R.SENT)
        want[:, p["padl"]:p["padl"] + p["T"]] = torch.nn.functional.embedding(ids.reshape(p["N"], p["T"]), table)
        if c["bufs"]["out"][1] == "bf16":
            want = want.to(torch.bfloat16).float()
        assert np.array_equal(R._u32(R.expect(c)["out"][0][MARGIN:-MARGIN]), R._u32(want.reshape(-1).numpy())), c["name"]
    for c in R.embedding_bwd_cases() + R.embedding_bwd_probes():
        p = c["p"]
        ids = torch.from_numpy(c["bufs"]["ids"][0]).long().clamp(0, p["V"] - 1)
        dout = T(logical(c, "dout")).reshape(p["N"], p["P"], p["D"])[:, p["padl"]:p["padl"] + p["T"]].reshape(-1, p["D"])
        tab = T(c["bufs"]["dtable"][0])
        sl = slice(p["dtable_off"], p["dtable_off"] + p["V"] * p["D"])
        tab[sl] = tab[sl].reshape(p["V"], p["D"]).index_add(0, ids, dout).reshape(-1)
        val, err = R.expect(c)["dtable"]
        assert np.allclose(val, tab.numpy(), rtol=1e-13, atol=1e-13), c["name"]
        assert (err is None) == c["exact"]
    hot = R.embedding_bwd_probes()
    for c in hot:                       # a probe's answer is its one element in its one word - or nothing, from a pad row
        delta = R.expect(c)["dtable"][0] - c["bufs"]["dtable"][0]
        assert delta.sum() == (0.0 if "pad" in c["name"] else 1.0) and np.count_nonzero(delta) == (0 if "pad" in c["name"] else 1)


def test_reductions_against_torch():
    for c in R.colsum_cases() + R.colsum_cases(random=True) + R.colsum_probes():
        p = c["p"]
        x = torch.as_strided(T(c["bufs"]["x"][0]), (p["rows"], p["C"]), (p["ld"], 1), p["x_off"])
        want = T(c["bufs"]["out"][0])
        want[p["out_off"]:p["out_off"] + p["C"]] += x.sum(0)
        assert np.allclose(R.expect(c)["out"][0], want.numpy(), rtol=1e-13, atol=1e-13), c["name"]
        if "probe" in c["name"]:
            delta = R.expect(c)["out"][0] - c["bufs"]["out"][0]
            assert delta.sum() == (0.0 if "padding" in c["name"] else 1.0), c["name"]
            assert np.count_nonzero(delta) == (0 if "padding" in c["name"] else 1), c["name"]
    for c in R.sumsq_cases() + R.sumsq_cases(random=True) + R.sumsq_probes():
        want = T(c["bufs"]["out"][0])
        want[c["p"]["out_off"]] += (T(logical(c, "x")) ** 2).sum()
        assert np.allclose(R.expect(c)["out"][0], want.numpy(), rtol=1e-12), c["name"]
        if "probe" in c["name"]:
            assert (R.expect(c)["out"][0] - c["bufs"]["out"][0]).sum() == 0.25
    for c in R.segment_stats_cases():
        x, offs = T(c["bufs"]["x"][0][MARGIN:]), c["bufs"]["offsets"][0]
        val = R.expect(c)["out"][0]
        for s in range(c["p"]["nseg"]):
            seg = x[offs[s]:offs[s + 1]]
            want = [seg.sum(), (seg * seg).sum(), seg.min() if len(seg) else np.inf, seg.max() if len(seg) else -np.inf]
            assert np.allclose(val[MARGIN + 4 * s:MARGIN + 4 * s + 4], np.array([float(w) for w in want]), rtol=1e-12), (c["name"], s)
        if "outside" in c["name"]:
            assert (val[MARGIN:-MARGIN].reshape(-1, 4)[:, :2] == 0).all(), "an element outside every segment counts for nothing"
        assert tuple(val[MARGIN:MARGIN + 4]) == (0.0, 0.0, np.inf, -np.inf), "the empty segment"


def test_l1_against_autograd():
    for c in R.l1_loss_cases() + R.l1_loss_cases(random=True) + R.l1_loss_probes()[:6]:
        p = c["p"]
        N, Tn, P, F = p["N"], p["T"], p["P"], p["F"]
        pred = T(logical(c, "pred")).requires_grad_(True)
        view = pred.reshape(N, P, p["ldp"])[:, p["padl"]:p["padl"] + Tn, :F]
        d = (view - T(logical(c, "target")).reshape(N, Tn, F)).abs()
        w_all, w_prio = float(np.float32(p["w_all"])), float(np.float32(p["w_prio"]))
        s_all, s_prio = d.sum(), d[:, :, :p["n_prio"]].sum()
        (w_all * s_all + w_prio * s_prio).backward()
        exp = R.expect(c)
        acc = c["bufs"]["loss_acc"][0].astype(np.float64)
        acc[p["acc_off"]:p["acc_off"] + 2] += [float(s_all.detach()), float(s_prio.detach())]
        assert np.allclose(exp["loss_acc"][0], acc, rtol=1e-12), c["name"]
        if "dpred" in exp:
            g = pred.grad.reshape(N, P, p["ldp"])[:, p["padl"]:p["padl"] + Tn, :F]
            got = torch.from_numpy(exp["dpred"][0][MARGIN:-MARGIN]).reshape(N, P, p["ldd"])
            want = g.numpy().astype(np.float32)              # one fp32 add: within one rounding of the float64 weight
            want = R.rne_bf16(want) if c["bufs"]["dpred"][1] == "bf16" else want
            inner = got[:, p["padl"]:p["padl"] + Tn, :F].numpy()
            assert np.abs(inner.astype(np.float64) - want).max() <= 2.0 ** (-8 if c["bufs"]["dpred"][1] == "bf16" else -23) * np.abs(want).max()
            assert (np.sign(inner) == np.sign(g.numpy())).all() and (inner[g.numpy() == 0] == 0).all()
            rest = got.clone()
            rest[:, p["padl"]:p["padl"] + Tn, :F] = R.SENT
            assert (rest == R.SENT).all(), "pad rows and the columns beyond F keep the sentinel"


def test_adam_against_the_formula():
    for c in R.adam_cases():
        p, n = c["p"], min(c["p"]["n"], 300)
        exp = R.expect(c)
        if p["raised"] is not None:
            assert all(np.array_equal(exp[o][0], c["bufs"][o][0]) for o in ("p", "m", "v")) and exp["skipped"][0][MARGIN] == 1
            continue
        assert exp["skipped"][0][MARGIN] == 0.5
        f = lambda x: float(np.float32(x))
        scale = f(p["grad_scale"])
        if "gnorm_sq" in c["bufs"]:
            norm = float(logical(c, "gnorm_sq")[0]) ** 0.5 * scale
            scale *= f(p["clip"]) / max(norm, f(p["clip"]))
        for i in range(n):
            g = float(logical(c, "g")[i]) * scale
            m = f(p["beta1"]) * float(logical(c, "m")[i]) + (1 - f(p["beta1"])) * g
            v = f(p["beta2"]) * float(logical(c, "v")[i]) + (1 - f(p["beta2"])) * g * g
            w = float(logical(c, "p")[i]) - f(p["lr_t"]) * m / (v ** 0.5 + f(p["eps"]))
            for name, want in (("m", m), ("v", v), ("p", w)):
                assert abs(exp[name][0][MARGIN + i] - want) <= 1e-13 * max(1.0, abs(want)), (c["name"], name, i)


def test_bn_fwd_against_torch():
    F = torch.nn.functional
    for c in R.bn_fwd_cases():
        p, b = c["p"], c["bufs"]
        rows, C = p["rows"], p["C"]
        if rows > 1000:
            continue
        exp = R.expect(c)
        z = T(logical(c, "z")).reshape(rows, C)
        valid = torch.from_numpy(R.row_valid(rows, p["row_mask"]))
        g, be = T(logical(c, "gamma")), T(logical(c, "beta"))
        yv = torch.from_numpy(exp["y_value"][0])
        assert (yv[~valid] == 0).all(), "rows that fail the mask are zero"
        cols = list(range(C))
        if p["stats_final"]:
            want = ((z - T(logical(c, "mean_out"))) * T(logical(c, "istd_out")) * g + be)[valid]
        elif p["training"]:                     # the batch's own statistics: those of the case up to their fp32 rounding
            want = F.batch_norm(z[valid], None, None, g, be, True, 0.0, p["eps"]) if valid.sum() > 1 else None
            cols = [k for k in cols if not (k == 2 and p["dtype"] == "f32")]             # column 2: made-up sums
        else:
            want = F.batch_norm(z, T(logical(c, "moving_mean")), T(logical(c, "moving_var")), g, be, False, 0.0, p["eps"])[valid]
        if want is not None:
            assert torch.allclose(yv[valid][:, cols], want[:, cols], rtol=1e-4, atol=1e-4), c["name"]
        if p["training"] and not p["stats_final"]:
            count = p["count"]
            mean = T(logical(c, "col_sum")) / count
            var = (T(logical(c, "col_sumsq")) / count - mean * mean).clamp(min=0)
            if C > 2 and p["dtype"] == "f32":
                assert var[2] == 0 and float(logical(c, "col_sumsq")[2]) / count - float(mean[2]) ** 2 < -1e-4
            assert np.allclose(exp["istd_out"][0][MARGIN:-MARGIN], (var + float(np.float32(p["eps"]))).rsqrt().numpy(), rtol=1e-13)
            if "moving_var" in c["outs"]:
                mom = float(np.float32(p["momentum"]))
                want_mv = T(logical(c, "moving_var")) * mom + var * (1 - mom)
                assert np.allclose(exp["moving_var"][0][MARGIN:-MARGIN], want_mv.numpy(), rtol=1e-13)
                assert np.allclose(exp["moving_mean"][0][MARGIN:-MARGIN], (T(logical(c, "moving_mean")) * mom + mean * (1 - mom)).numpy(), rtol=1e-13, atol=1e-15)


def test_highway_and_act_bwd_against_autograd():
    for c in small(R.highway_cases()):
        if not c["p"]["backward"]:
            h, t, x = (T(logical(c, k)) for k in "htx")
            assert np.allclose(R.expect(c)["y"][0][MARGIN:-MARGIN], (h * t + x * (1 - t)).numpy(), rtol=1e-14, atol=1e-15)
            continue
        h, t, x, dy = (T(logical(c, k)) for k in ("h", "t", "x", "dy"))
        a = torch.where(h > 0, h, torch.full_like(h, -1.0)).requires_grad_(True)          # H = relu(a), T = sigmoid(b)
        b = torch.log(t / (1 - t)).requires_grad_(True)
        xx = x.clone().requires_grad_(True)
        tt = torch.sigmoid(b)
        ((torch.relu(a) * tt + xx * (1 - tt)) * dy).sum().backward()
        exp = R.expect(c)
        for name, want in (("dhpre", a.grad), ("dtpre", b.grad), ("dx", xx.grad)):
            assert np.allclose(exp[name][0][MARGIN:-MARGIN], want.numpy(), rtol=1e-9, atol=1e-12), (c["name"], name)
        assert (exp["dhpre"][0][MARGIN:-MARGIN][logical(c, "h") == 0] == 0).all(), "h = 0: the ReLU passes nothing"
    for c in small(R.act_bwd_cases()):
        p = c["p"]
        y, dy = T(logical(c, "y")), T(logical(c, "dy"))
        act = p["act"]
        pre = {R.ACT_RELU: torch.where(y > 0, y, torch.full_like(y, -1.0)), R.ACT_TANH: torch.atanh(y),
               R.ACT_SIGMOID: torch.log(y / (1 - y)), R.ACT_SOFTSIGN: y / (1 - y.abs())}.get(act, y).clone().requires_grad_(True)
        out = {R.ACT_RELU: torch.relu, R.ACT_TANH: torch.tanh, R.ACT_SIGMOID: torch.sigmoid,
               R.ACT_SOFTSIGN: torch.nn.functional.softsign}.get(act, lambda v: v)(pre)
        valid = T(R.row_valid(p["rows"], p["row_mask"]).astype(np.float64)).repeat_interleave(p["C"])
        (out * dy * valid).sum().backward()
        assert np.allclose(R.expect(c)["dpre"][0][MARGIN:-MARGIN], pre.grad.numpy(), rtol=1e-8, atol=1e-12), c["name"]


def test_bn_bwd_against_autograd():
    """y = gamma * (act(pre) - mean) * istd + beta with the batch statistics of the valid rows INSIDE the graph (eps as in
    bn_fwd_cases): dpre, dgamma, dbeta of every activation under a mask, and dbias as the column sum of dpre."""
    eps = 1e-3
    for act in range(5):
        c = R._bn_bwd_case("fallback-C8-rows70-autograd-act%d" % act, 70, 8, act, mask=(10, 2, 9), seed=300 + act)
        p, b, off = c["p"], c["bufs"], c["p"]["off"]
        rows, C = p["rows"], p["C"]
        valid = R.row_valid(rows, p["row_mask"])
        z32 = logical(c, "z").reshape(rows, C).copy()
        lo, hi = {R.ACT_TANH: (-0.99, 0.99), R.ACT_SOFTSIGN: (-0.99, 0.99), R.ACT_SIGMOID: (0.01, 0.99)}.get(act, (-9, 9))
        z32[valid] = np.clip(z32[valid], lo, hi)             # the inverse activation must exist (the GPU cases keep |z| = 1)
        z = T(z32[valid])
        pre = {R.ACT_RELU: torch.where(z > 0, z, torch.full_like(z, -1.0)), R.ACT_TANH: torch.atanh(z),
               R.ACT_SIGMOID: torch.log(z / (1 - z)), R.ACT_SOFTSIGN: z / (1 - z.abs())}.get(act, z).clone().requires_grad_(True)
        a = {R.ACT_RELU: torch.relu, R.ACT_TANH: torch.tanh, R.ACT_SIGMOID: torch.sigmoid,
             R.ACT_SOFTSIGN: torch.nn.functional.softsign}.get(act, lambda v: v)(pre)
        gamma, beta = T(logical(c, "gamma")).requires_grad_(True), torch.zeros(C, dtype=torch.float64, requires_grad=True)
        mean = a.mean(0)
        istd = (((a - mean) ** 2).mean(0) + eps).rsqrt()
        dy = T(logical(c, "dy").reshape(rows, C)[valid])
        ((gamma * (a - mean) * istd + beta) * dy).sum().backward()
        c["bufs"] = dict(b, z=(R.framed(z32), "f32"), mean=(R.framed(mean.detach().numpy()), "f32"),
                         istd=(R.framed(istd.detach().numpy()), "f32"))
        exp = R.expect(c)
        dpre = exp["dpre"][0][MARGIN:-MARGIN].reshape(rows, C)
        assert (dpre[~valid] == 0).all() and not np.signbit(dpre[~valid]).any(), "masked rows are +0"
        assert np.allclose(dpre[valid], pre.grad.numpy(), rtol=1e-4, atol=1e-6), act
        for k, g in (("dgamma", gamma.grad), ("dbeta", beta.grad)):
            assert np.allclose(exp[k][0][MARGIN:-MARGIN] - logical(c, k), g.numpy(), rtol=1e-4, atol=1e-5), (act, k)
        got = emulate(c)
        assert not R.rejected(c, got, factor=1.0)
        assert np.allclose(got["dbias"][MARGIN:-MARGIN] - logical(c, "dbias"), pre.grad.sum(0).numpy(), rtol=1e-4, atol=1e-4), act


def test_bn_bwd_cases_hold_what_the_contract_asks():
    """Every form under its name, the inputs that make mistakes visible, and the exact bf16 case's point."""
    cases = R.bn_bwd_cases()
    forms = {}
    for c in cases:
        forms.setdefault(R.bn_bwd_form(c), []).append(c)
        assert c["name"].startswith(R.bn_bwd_form(c) + "-")
        p = c["p"]
        valid = R.row_valid(p["rows"], p["row_mask"])
        z = logical(c, "z", p["rows"] * p["C"], p["off"]["z"]).reshape(p["rows"], p["C"])
        assert (z[~valid] > 1e29).all() and np.isnan(c["bufs"]["work"][0][p["off"]["work"]:-MARGIN]).all()
        if not c["exact"]:
            want = {R.ACT_RELU: [0, 2.0 ** -126], R.ACT_TANH: [1, -1, 0], R.ACT_SIGMOID: [0, 1], R.ACT_SOFTSIGN: [1, -1]}.get(p["act"], [])
            assert all((z[valid] == v).any() for v in want), c["name"]
        if p["ld_dy"]:
            assert np.isnan(logical(c, "dy")).sum() == p["rows"] * (p["ld_dy"] - p["C"])
    for form in ("scalar", "vector", "fallback"):
        got = forms[form]
        assert {c["p"]["act"] for c in got} == set(range(5)), form
        assert {(c["p"]["dtype"], c["bufs"]["dpre"][1]) for c in got} == {("f32", "f32"), ("bf16", "bf16"), ("f32", "bf16")}, form
        assert any(c["exact"] for c in got) and any(c["p"]["count"] != c["p"]["rows"] for c in got)
        assert all(any(k not in c["bufs"] for c in got) for k in ("dgamma", "dbeta", "dbias"))
    assert R.bn_bwd_row_blocks(find(cases, "scalar-C6-rows65-relu")) == (2, 33)
    assert R.bn_bwd_row_blocks(find(cases, "scalar-C6-rows2049-none-mask")) == (32, 65)
    assert R.bn_bwd_row_blocks(find(cases, "vector-C132-rows129-sigmoid-mask")) == (2, 65)
    assert R.bn_bwd_row_blocks(find(cases, "fallback-C8-rows8193-relu-mask")) == (64, 129)
    for name, rpb in (("scalar-C6-rows2049-none-mask", 65), ("vector-C8-rows8193-relu-mask", 129)):      # a whole block invalid
        c = find(cases, name)
        valid = R.row_valid(c["p"]["rows"], c["p"]["row_mask"])
        assert any(not valid[k:k + rpb].any() for k in range(0, c["p"]["rows"], rpb)), name
    c = find(cases, "vector-exact-C8-rows160-bf16dpre-none")
    v = R.expect(c)["dpre"][0]
    assert (R.rne_bf16(v.astype(np.float32)) != v).sum() > 10, "fp32-exact values that bf16 rounds"


def test_gru_pointwise_against_the_cell():
    """Modes 0 - 3 chained through the candidate product reproduce one step of the cell of tests/test_gru_seq_gpu.py
    (ru = sigmoid(xg + h Wg), c = tanh(xc + (r h) Wc), h' = u h + (1 - u) c, masked past the length) and its autograd."""
    rng = np.random.RandomState(5)
    for reverse in (False, True):
        N, H, t, Tn = 3, 128, 4, 9
        lengths = np.array([5, 4, 7], np.int32)
        fr = lambda *s: rng.randn(*s).astype(np.float32)
        xg, xc, h0, wg, wc, dh = fr(N, 2 * H), fr(N, H), fr(N, H) * 0.5, fr(H, 2 * H) * 0.1, fr(H, H) * 0.1, fr(N, H)
        hprev_buf = fr(N, H)                                 # what h_prev points at; rows at their first step take h_init
        first = (t == lengths - 1) if reverse else np.zeros(N, bool)
        h_in = np.where(first[:, None], h0, hprev_buf)
        h = T(h_in).requires_grad_(True)
        xgt, xct = T(xg).requires_grad_(True), T(xc).requires_grad_(True)
        ru = torch.sigmoid(xgt + h @ T(wg))
        r, u = ru[:, :H], ru[:, H:]
        rh = r * h
        c = torch.tanh(xct + rh @ T(wc))
        m = T((t < lengths).astype(np.float64))[:, None]
        h2 = m * (u * h + (1 - u) * c)
        (h2 * T(dh)).sum().backward()
        fb = lambda x, dt="f32": (R.framed(x), dt)
        base = dict(N=N, H=H, t=t, T=Tn, reverse=reverse, dtype="f32", ru_sn=2 * H, c_sn=H, hp_sn=H, out_sn=H, out2_sn=H,
                    dzg_sn=2 * H, dh_sn=H, carry_sn=H, dha_sn=H, hi_sn=H)
        common = dict(ru=fb(ru.detach().numpy()), h_prev=fb(hprev_buf), lengths=(lengths, "i32"), h_init=fb(h0))
        inner = lambda e, name, n: e[name][0][MARGIN:MARGIN + n]
        c0 = R.case("gru_pointwise", "m0", dict(base, mode=0), dict(common, out=fb(np.zeros(N * H))), ["out"])
        assert np.allclose(inner(R.expect(c0), "out", N * H), rh.detach().numpy().reshape(-1), rtol=1e-6, atol=1e-7)
        c1 = R.case("gru_pointwise", "m1", dict(base, mode=1), dict(common, c=fb(c.detach().numpy()), out=fb(np.zeros(N * H))), ["out"])
        assert np.allclose(inner(R.expect(c1), "out", N * H), h2.detach().numpy().reshape(-1), rtol=1e-6, atol=1e-7)
        carry0 = fr(N, H)
        c2 = R.case("gru_pointwise", "m2", dict(base, mode=2),
                    dict(common, c=fb(c.detach().numpy()), dh=fb(dh * 0.25), dh_add=fb(dh * 0.75), out=fb(np.zeros(N * H)),
                         dzg=fb(np.zeros(N * 2 * H)), carry=fb(carry0)), ["out", "dzg", "carry"])
        e2 = R.expect(c2)
        dzc = inner(e2, "out", N * H).reshape(N, H)
        assert np.allclose(dzc, xct.grad.numpy(), rtol=1e-5, atol=1e-7)
        assert np.allclose(inner(e2, "dzg", 2 * N * H).reshape(N, 2 * H)[:, H:], xgt.grad.numpy()[:, H:], rtol=1e-5, atol=1e-7)
        carry = inner(e2, "carry", N * H).reshape(N, H)
        assert np.array_equal(carry[1], carry0[1].astype(np.float64)), "mode 2 leaves the carry of a masked row"
        drh = dzc @ wc.astype(np.float64).T
        c3 = R.case("gru_pointwise", "m3", dict(base, mode=3),
                    dict(common, dh=fb(drh), dzg=fb(np.zeros(N * 2 * H)), carry=fb(carry)), ["dzg", "carry"])
        e3 = R.expect(c3)
        assert np.allclose(inner(e3, "dzg", 2 * N * H).reshape(N, 2 * H)[:, :H], xgt.grad.numpy()[:, :H], rtol=1e-4, atol=1e-6)
        total = inner(e3, "carry", N * H).reshape(N, H)         # + the gate product's share = d / d h
        want = h.grad.numpy() - xgt.grad.numpy() @ wg.astype(np.float64).T
        live = lengths > t
        assert np.allclose(total[live], want[live], rtol=1e-4, atol=1e-6)
        assert np.allclose(total[1], carry0[1], rtol=1e-6), "mode 3 adds nothing to the carry of a masked row"


# ------------------------------------------------------------------------------------------------------ the bounds
BOUNDED = dict(bn_fwd=R.bn_fwd_cases, adam=R.adam_cases, highway=R.highway_cases, act_bwd=R.act_bwd_cases,
               gru_pointwise=R.gru_pointwise_cases, bn_bwd=R.bn_bwd_cases)


@pytest.mark.parametrize("op", sorted(BOUNDED))
def test_float32_emulations_stay_within_the_bound(op):
    """Every association order, with and without FMA, within 1 x the running-error bound on the GPU module's inputs (the
    largest cases once, on two arithmetics); bf16 outputs by the store rule with the band at 1 x."""
    worst = 0.0
    for c in BOUNDED[op]():
        big = max(len(b[0]) for b in c["bufs"].values()) > 70000
        for A in (ARITHMETICS[1::9] if big else ARITHMETICS):
            for o, v in R.check(c, emulate(c, A), factor=1.0).items():
                assert v.ok, (c["name"], o, A.order, A.fma, v.why)
                if c["bufs"][o][1] == "f32":
                    worst = max(worst, v.worst)
    WORST[op] = worst
    print("\n  %-14s worst float32 emulation / bound %.3f" % (op, worst))
    assert 0.05 < worst <= 1.0


def _f32_sums(x, rng):
    """float32 sums of x in several orders: forward, backward, shuffled, pairwise, blocks of 64 lanes."""
    x = np.asarray(x, np.float32)
    seq = lambda v: np.cumsum(v, dtype=np.float32)[-1]
    out = [seq(x), seq(x[::-1]), seq(rng.permutation(x)), np.add.reduce(x, dtype=np.float32)]
    pad = np.concatenate([x, np.zeros(-len(x) % 64, np.float32)]).reshape(-1, 64)
    out.append(seq(np.cumsum(pad, 0, dtype=np.float32)[-1]))
    return out


def test_random_sums_stay_within_the_bound():
    rng = np.random.RandomState(3)
    worst = 0.0
    for c in R.colsum_cases(random=True)[:1] + R.sumsq_cases(random=True) + R.segment_stats_cases()[1:2] + R.l1_loss_cases(random=True)[:3]:
        val, err = R.expect(c)[c["outs"][0]]
        if c["op"] == "colsum":
            p = c["p"]
            x = c["bufs"]["x"][0][p["x_off"] + np.arange(p["rows"])[:, None] * p["ld"] + np.arange(p["C"])[None, :]]
            for k in range(0, p["C"], 7):
                for s in _f32_sums(np.concatenate([[c["bufs"]["out"][0][p["out_off"] + k]], x[:, k]]), rng):
                    worst = max(worst, abs(float(s) - val[p["out_off"] + k]) / err[p["out_off"] + k])
        elif c["op"] == "sumsq":
            x = logical(c, "x")
            o = c["p"]["out_off"]
            for s in _f32_sums(np.concatenate([[c["bufs"]["out"][0][o]], x * x]), rng):
                worst = max(worst, abs(float(s) - val[o]) / err[o])
        elif c["op"] == "segment_stats":
            x, offs = c["bufs"]["x"][0][MARGIN:], c["bufs"]["offsets"][0]
            for s in range(2, c["p"]["nseg"]):
                seg = x[offs[s]:offs[s + 1]]
                for k, terms in enumerate((seg, seg * seg)):
                    for got in _f32_sums(terms, rng):
                        worst = max(worst, abs(float(got) - val[MARGIN + 4 * s + k]) / err[MARGIN + 4 * s + k])
        else:
            p = c["p"]
            prow = (np.arange(p["N"])[:, None] * p["P"] + p["padl"] + np.arange(p["T"])[None, :]).reshape(-1)
            pred = c["bufs"]["pred"][0][MARGIN + prow[:, None] * p["ldp"] + np.arange(p["F"])[None, :]]
            d = np.abs(pred - logical(c, "target").reshape(-1, p["F"])).reshape(-1)
            o = p["acc_off"]
            for s in _f32_sums(np.concatenate([[c["bufs"]["loss_acc"][0][o]], d]), rng):
                worst = max(worst, abs(float(s) - val[o]) / err[o])
    print("\n  random sums    worst float32 sum / bound %.3f" % worst)
    assert 0 < worst <= 1.0


# ------------------------------------------------------------------------------------------------------ exactness
def test_exact_by_construction_sums_are_order_free():
    """expect() asserts sum |terms| / unit < 2^24 on every exact case (assert_exact_sum); here: float32 sums of those
    terms in shuffled orders are bit-identical and equal the float64 sum."""
    rng = np.random.RandomState(4)
    n = 0
    for c in (R.colsum_cases() + R.sumsq_cases() + R.segment_stats_cases()[:1] + R.l1_loss_cases() + R.embedding_bwd_cases() +
              R.colsum_probes()[:3] + R.sumsq_probes()[:3] + R.l1_loss_probes()[:3] + R.embedding_bwd_probes()[:3] +
              R.bn_bwd_cases() + R.bn_bwd_probes()):
        if not c["exact"]:
            continue
        exp = R.expect(c)                                   # runs the assertions
        assert all(e is None for o, (v, e) in exp.items()), c["name"]
        n += 1
        if c["op"] == "bn_bwd":                             # every summation order and product association, fused or not
            assert set(exp) == set(c["outs"])
            for A in ARITHMETICS:
                got = emulate(c, A)
                assert all(R.bits_equal(got[o], R.store(exp[o][0].astype(np.float32), c["bufs"][o][1])).all() for o in c["outs"]), c["name"]
        if c["op"] == "sumsq":
            x = logical(c, "x")
            o = c["p"]["out_off"]
            sums = _f32_sums(np.concatenate([[c["bufs"]["out"][0][o]], x * x]), rng)
            assert len(set(float(s) for s in sums)) == 1 and float(sums[0]) == exp["out"][0][o], c["name"]
        if c["op"] == "colsum":
            p = c["p"]
            x = c["bufs"]["x"][0][p["x_off"] + np.arange(p["rows"])[:, None] * p["ld"] + np.arange(p["C"])[None, :]]
            k = p["C"] - 1
            sums = _f32_sums(np.concatenate([[c["bufs"]["out"][0][p["out_off"] + k]], x[:, k]]), rng)
            assert len(set(float(s) for s in sums)) == 1 and float(sums[0]) == exp["out"][0][p["out_off"] + k], c["name"]
    assert n > 60 + 8 + 27
    with pytest.raises(AssertionError):                     # an intermediate that fp32 would round
        R.Exact().mul(R.Exact().lift(np.float32(1 + 2.0 ** -20)), R.Exact().lift(np.float32(1 + 2.0 ** -20)))
    with pytest.raises(AssertionError):
        R.assert_exact_sum(2.0 ** 24 * R.UNIT, R.UNIT)
    bad = find(R.sumsq_cases(), "n4200003-work")
    bad = dict(bad, bufs=dict(bad["bufs"], x=(bad["bufs"]["x"][0] * 2, "f32")))
    with pytest.raises(AssertionError):                     # a case cannot silently stop being exact
        R.expect(bad)


def test_bf16_store_rule_on_the_references_alone():
    """Under the bf16 store rule (band = 2 x the bound, as on the GPU) the references alone - rounded to bf16 directly, and
    through float32 emulations of the contract in four arithmetics - give far fewer than 1 % neighbours on every bf16
    buffer of the chosen inputs: the allowance is not consumed before a kernel has run.  (A product of two bf16 inputs can
    sit exactly ON a rounding boundary; fp32 computes it exactly, so it rounds as the reference does.)"""
    seen, most = 0, 0.0
    for op, cases in BOUNDED.items():
        for c in small(cases()):
            exp = R.expect(c)
            outs = [o for o in c["outs"] if c["bufs"][o][1] == "bf16" and o in exp]
            for A in ARITHMETICS[::5] if outs else []:
                got = emulate(c, A)
                for o in outs:
                    val, err = exp[o]
                    assert R.accepts(R.rne_bf16(val.astype(np.float32)), val, err, "bf16").neighbours == 0
                    v = R.accepts(got[o], val, err, "bf16", 2.0)
                    assert v.ok, (c["name"], o, v.why)
                    if v.counted >= 100:
                        assert v.neighbours < 0.01 * v.counted, (c["name"], o, v.why)
                        most = max(most, v.neighbours / v.counted)
                        seen += 1
    print("\n  bf16 store rule: at most %.2f %% neighbours among the references' own float32 emulations" % (100 * most))
    assert seen > 50


# ------------------------------------------------------------------------------------------------------ the mutants
def _cases_of(op):
    return dict(colsum=lambda: R.colsum_cases() + R.colsum_probes(), l1_loss=R.l1_loss_cases, adam=R.adam_cases, bn_fwd=R.bn_fwd_cases,
                gru_pointwise=R.gru_pointwise_cases, embedding_fwd=R.embedding_fwd_cases, embedding_bwd=R.embedding_bwd_cases,
                cast2d=R.cast2d_cases, split_hi_lo=R.split_cases, copy3d=R.copy3d_cases, sumsq=R.sumsq_cases,
                highway=R.highway_cases, act_bwd=R.act_bwd_cases, bn_bwd=R.bn_bwd_cases)[op]()


# wrong kernel -> (op, mutation, a case of the GPU module that must reject it; None: some case of the op must)
MUTANTS = {
    "the last tail column dropped": ("colsum", "drop_tail", "vector-64-blocks-8193x130-ld132-f32-work-probe-last"),
    "one row of a row block dropped": ("colsum", "drop_row", "vector-64-blocks-8193x130-ld132-f32-work"),
    "a padding column added": ("colsum", "pad_column", "vector-ragged-300x66-ld68-bf16-atomic"),
    "the column sum overwrites its += output": ("colsum", "overwrite", "column-300x37-ld37-f32-work"),
    "the table gradient overwrites its += output": ("embedding_bwd", "overwrite", "ragged-exact"),
    "sumsq overwrites its += output": ("sumsq", "overwrite", "n1027-atomic"),
    "copy3d ignores accumulate": ("copy3d", "overwrite", "3x5x7-bf16-bf16-acc1"),
    "bf16 by truncation (copy3d)": ("copy3d", "truncate", "3x5x7-f32-bf16-acc0"),
    "bf16 by truncation (cast2d)": ("cast2d", "truncate", "vector-edge-68x132-T-bf16"),
    "bf16 by truncation (split)": ("split_hi_lo", "truncate", "n255"),
    "bf16 by truncation (Adam's shadow)": ("adam", "truncate", "n257-above-clip"),
    "lo computed from the unrounded hi (split)": ("split_hi_lo", "lo_unrounded", "n255"),
    "lo computed from the unrounded hi (cast2d)": ("cast2d", "lo_unrounded", "scalar-33x65-N-f32-pair"),
    "lo computed from the unrounded hi (bn_fwd)": ("bn_fwd", "lo_unrounded", "vector-C132-ld-pair"),
    "sign(0) = 1": ("l1_loss", "sign0", "narrow-flat-78"),
    "n_prio one too many": ("l1_loss", "prio_plus", "wide-quad-257"),
    "n_prio one too few": ("l1_loss", "prio_minus", "narrow-quad-80-rows3400"),
    "w_prio applied to all bins": ("l1_loss", "prio_all", "wide-scalar-1025"),
    "eps inside the square root": ("adam", "eps_inside", "n255-below-clip"),
    "the clip applied when the norm is below it": ("adam", "always_clip", "n255-below-clip"),
    "grad_scale left out of the norm": ("adam", "norm_unscaled", "n255-scaled-below-clip"),
    "beta2 used for m": ("adam", "beta2_for_m", "n1-no-norm"),
    "a raised status word ignored": ("adam", "ignore_status", "n257-raised-11"),
    "the momentum on the wrong term": ("bn_fwd", "momentum_swapped", "scalar-C6-train-mask"),
    "a negative variance not clamped": ("bn_fwd", "no_clamp", "vector-C132-ld-pair"),
    "a masked row not zeroed (bn_fwd)": ("bn_fwd", "mask_ignored", "scalar-C6-train-mask"),
    "a masked row not zeroed (act_bwd)": ("act_bwd", "mask_ignored", "257x1-f32-act2"),
    "the ReLU passes at h = 0": ("highway", "relu_at_zero", "n257-f32-bwd"),
    "h_init taken at t == 0 in the reverse direction": ("gru_pointwise", "init_at_zero", "N3-H128-f32-mode1-init-rev"),
    "an id outside [0, V) not clamped (forward)": ("embedding_fwd", "no_clamp", "ragged-bf16"),
    "an id outside [0, V) not clamped (backward)": ("embedding_bwd", "no_clamp", "ragged-exact"),
    "xhat without istd in the sum of dy * xhat": ("bn_bwd", "s2_no_istd", "fallback-C132-rows129-sigmoid-mask"),
    "count replaced by rows": ("bn_bwd", "count_rows", "scalar-C6-rows70-tanh-mask"),
    "masked rows included in the sums": ("bn_bwd", "sums_unmasked", "scalar-C6-rows70-tanh-mask"),
    "masked rows of dpre not zeroed": ("bn_bwd", "dpre_mask_ignored", "vector-C68-rows128-tanh-mask"),
    "the ReLU passes at z = 0 (bn_bwd)": ("bn_bwd", "relu_at_zero", "scalar-C6-rows65-relu"),
    "tanh factor 1 - z": ("bn_bwd", "tanh_linear", "vector-C68-rows128-tanh-mask"),
    "sigmoid factor z (1 + z)": ("bn_bwd", "sigmoid_plus", "vector-C132-rows129-sigmoid-mask"),
    "softsign factor unsquared": ("bn_bwd", "softsign_unsquared", "fallback-C68-rows300-bf16-softsign-mask"),
    "istd dropped from gamma * istd": ("bn_bwd", "no_istd_scale", "fallback-C68-rows128-tanh-mask"),
    "dgamma and dbeta swapped": ("bn_bwd", "swapped", "scalar-C6-rows70-tanh-mask"),
    "= in place of += (bn_bwd)": ("bn_bwd", "overwrite", "vector-C68-rows128-tanh-mask"),
    "ld_dy ignored": ("bn_bwd", "ld_ignored", "vector-C68-rows300-bf16dpre-relu-ld80-col8"),
    "the last row block dropped from the sums": ("bn_bwd", "drop_last_block", "fallback-C132-rows129-sigmoid-mask"),
    "given sums ignored for recomputed ones": ("bn_bwd", "recompute_sums", "vector-C68-rows300-sums-not-the-column-sums"),
    "dbias summed on unrounded values": ("bn_bwd", "dbias_unrounded", "vector-exact-C8-rows160-bf16dpre-none"),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_the_comparison_rejects_the_mutant(name):
    op, mut, which = MUTANTS[name]
    c = find(_cases_of(op), which)
    good = R.check(c, emulate(c))
    assert all(v.ok for v in good.values()), ("the correct emulation must pass", {o: v.why for o, v in good.items() if not v.ok})
    bad = R.check(c, emulate(c, mut=mut))
    assert any(not v.ok for v in bad.values()), "the comparison accepts: " + name
    print("\n  rejected: %-50s %s" % (name, "; ".join("%s: %s" % (o, v.why) for o, v in bad.items() if not v.ok)))


def test_every_probe_rejects_a_moved_element():
    """A one-hot probe's answer moved to the neighbouring column or word, or doubled, is rejected."""
    for c in R.colsum_probes()[:11] + R.embedding_bwd_probes() + R.sumsq_probes()[:4] + R.l1_loss_probes()[:5]:
        o = c["outs"][0]
        good = emulate(c)
        assert not R.rejected(c, good)
        delta = good[o] - c["bufs"][o][0]
        moved = dict(good)
        moved[o] = c["bufs"][o][0] + (np.roll(delta, 1) if delta.any() else np.eye(1, len(delta), MARGIN, dtype=np.float32)[0])
        assert R.rejected(c, moved), c["name"]
    for c in R.bn_bwd_probes():          # the column's sum of dy (dbeta) moved to the next column, its dpre to the next element
        good = emulate(c)
        assert not R.rejected(c, good)
        for o in ("dbeta", "dpre"):
            delta = good[o] - c["bufs"][o][0]
            moved = dict(good)
            moved[o] = c["bufs"][o][0] + (np.roll(delta, 1) if "masked" not in c["name"] else np.eye(1, len(delta), MARGIN, dtype=np.float32)[0])
            assert R.rejected(c, moved), (c["name"], o)
        s1 = (good["dbeta"] - c["bufs"]["dbeta"][0]).sum()
        assert s1 == (0.0 if "masked" in c["name"] else 1.0), c["name"]
