"""tests/attn_ref.py must not be wrong the way a kernel is.  No GPU.

The pure forward passes against explicit scalar loops; forward and gradients against torch.autograd on an independent
float64 forward chained from the oracle's cells (oracle/taco2_oracle.py: prenet, lstm_block_cell,
location_sensitive_alignments with the UNFOLDED location convolution and layer - so the folded Wcl filter is checked
too; oracle/taco1_oracle.py: gru_cell, bahdanau_alignments); the single-step functions against the recurrence; and, for
every case of tests/test_attn_contract_gpu.py, that no ReLU kink lies inside the noise, that the case's inputs
exercise what the case is there for and that its tolerances reject each of eight planted errors."""
import functools
import math

import pytest
import torch

import attn_ref as R
import test_attn_contract_gpu as G
from oracle import taco1_oracle as O1
from oracle import taco2_oracle as O2

pytestmark = []                                  # (the import above must not lend this module its gpu mark)
f64 = torch.float64


def _tiny(N, S, Ti, A, E, D1, D2, kw, Dsp, lengths, clip, seed, taco1=False):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=f64)
    XA = D2 + Dsp + A
    x = dict(keys=r(N, Ti, A), values=r(N, Ti, E), f1=r(N, S + 1, D1), W1c=r(E, D1) * 0.5, W2=r(D1, D2) * 0.5, b2=r(D2) * 0.3,
             Wq=r(A, A), v=r(A), lengths=torch.tensor(lengths), spk=r(N, Dsp) if Dsp else None, cell_clip=clip)
    if taco1:
        x.update(Wg=r(XA, 2 * A) * 0.7, bg=r(2 * A) * 0.2, Wc=r(XA, A) * 0.7, bc=r(A) * 0.2)
    else:
        x.update(Watt=r(XA, 4 * A) * 0.9, batt=r(4 * A) * 0.2, Wcl=r(kw, A))
    return x, r(N, S + 1, A + E)


# ------------------------------------------------------------------------------------------------- scalar restatements
def _scalar(x, taco1):
    """The header's sentences one number at a time.  Returns nested lists per history, [n][slot][column]."""
    L = lambda t: t.tolist()
    keys, values, f1, W1c, W2, b2, Wq, v = (L(x[k]) for k in ("keys", "values", "f1", "W1c", "W2", "b2", "Wq", "v"))
    spk = L(x["spk"]) if x.get("spk") is not None else None
    N, Ti, A = x["keys"].shape
    E, S, D1, D2 = x["values"].shape[2], x["f1"].shape[1] - 1, x["W1c"].shape[1], x["W2"].shape[1]
    sg = lambda a: 1.0 / (1.0 + math.exp(-a))
    dot = lambda a, W, col: sum(a[i] * W[i][col] for i in range(len(a)))
    if taco1:
        Wg, bg, Wc, bc = (L(x[k]) for k in ("Wg", "bg", "Wc", "bc"))
        kw = 0
    else:
        Watt, batt, Wcl = (L(x[k]) for k in ("Watt", "batt", "Wcl"))
        kw, clip = len(Wcl), float(x["cell_clip"])
        half = (kw - 1) // 2
    out = {k: [] for k in (R.TACO1_HIST if taco1 else R.TACO2_HIST)}
    for n in range(N):
        length = int(x["lengths"][n])
        h, c, ctx, al = [0.0] * A, [0.0] * A, [0.0] * E, [0.0] * Ti
        rows = {k: [None] for k in out}
        for s in range(S):
            p1 = [max(0.0, f1[n][s + 1][d] + dot(ctx, W1c, d)) for d in range(D1)]
            p2 = [max(0.0, dot(p1, W2, j) + b2[j]) for j in range(D2)]
            xin = p2 + (spk[n] if spk else [])
            xa = xin + h
            if taco1:
                ru = [sg(dot(xa, Wg, k) + bg[k]) for k in range(2 * A)]
                xc = xin + [ru[u] * h[u] for u in range(A)]
                cc = [math.tanh(dot(xc, Wc, u) + bc[u]) for u in range(A)]
                h = [ru[A + u] * h[u] + (1 - ru[A + u]) * cc[u] for u in range(A)]
            else:
                z = [dot(xa, Watt, k) + batt[k] for k in range(4 * A)]
                ga = [sg(z[u]) for u in range(A)] + [math.tanh(z[A + u]) for u in range(A)] + \
                     [sg(z[2 * A + u] + 1.0) for u in range(A)] + [sg(z[3 * A + u]) for u in range(A)]
                c = [ga[2 * A + u] * c[u] + ga[u] * ga[A + u] for u in range(A)]
                if clip > 0:
                    c = [min(max(cu, -clip), clip) for cu in c]
                h = [ga[3 * A + u] * math.tanh(c[u]) for u in range(A)]
            q = [dot(h, Wq, u) for u in range(A)]
            e = []
            for t in range(length):
                acc = 0.0
                for u in range(A):
                    a = keys[n][t][u] + q[u]
                    for k in range(kw):
                        tt = t + k - half
                        if 0 <= tt < Ti:
                            a += al[tt] * Wcl[k][u]
                    acc += v[u] * math.tanh(a)
                e.append(acc)
            m = max(e)
            w = [math.exp(a - m) for a in e]
            al = [a / sum(w) for a in w] + [0.0] * (Ti - length)
            ctx = [sum(al[t] * values[n][t][j] for t in range(Ti)) for j in range(E)]
            step = dict(p1=p1, xa=xa, hc=h + ctx, q=q, align=al)
            step.update(dict(xc=xc, ru=ru, cc=cc) if taco1 else dict(ca=c, ga=ga))
            for k in rows:
                rows[k].append(step[k])
        for k in rows:
            rows[k][0] = [0.0] * len(rows[k][1])
            out[k].append(rows[k])
    return out


@pytest.mark.parametrize("taco1", [False, True])
@pytest.mark.parametrize("kw,Dsp,lengths,clip", [(3, 0, (4, 4), 0.0), (4, 2, (4, 1), 0.0), (1, 0, (3, 4), 0.3), (2, 1, (1, 2), 0.3)])
def test_pure_forward_matches_scalar_loops(taco1, kw, Dsp, lengths, clip):
    x, _ = _tiny(2, 3, 4, 3, 2, 4, 3, kw, Dsp, lengths, clip, seed=kw * 10 + Dsp, taco1=taco1)
    got = (R.taco1 if taco1 else R.taco2)(x)
    want = _scalar(x, taco1)
    for k, w in want.items():
        assert float((got[k] - torch.tensor(w, dtype=f64)).abs().max()) <= 1e-12, k
    if clip and not taco1:
        assert bool((got["ca"].abs() == clip).any())


# ------------------------------------------------------------------------------------------- the oracle's cells, chained
def _oracle_taco2(x, dhc, F=5, seed=0):
    """An independent forward from the oracle's building blocks, and autograd on it.  Leaves that stand where the
    kernels' gradient outputs are defined: f1 (p1's pre-activation), a per-step dense_2 bias (p2's), a per-step LSTM
    bias (the gates'), a per-step shift of the keys (the query).  The location filter is UNFOLDED: conv [kw, 1, F] and
    layer [F, A] whose product is Wcl."""
    N, Ti, A = x["keys"].shape
    E, S, D1, D2 = x["values"].shape[2], x["f1"].shape[1] - 1, x["W1c"].shape[1], x["W2"].shape[1]
    kw = x["Wcl"].shape[0]
    g = torch.Generator().manual_seed(seed)
    conv = torch.randn(kw, 1, F, generator=g, dtype=f64)
    layer = torch.linalg.lstsq(conv[:, 0], x["Wcl"]).solution if kw <= F else None       # conv . layer = Wcl exactly
    assert layer is not None and float((conv[:, 0] @ layer - x["Wcl"]).abs().max()) < 1e-10
    leaf = lambda t: t.clone().requires_grad_(True)
    keys, values, f1, v, conv, layer = leaf(x["keys"]), leaf(x["values"]), leaf(x["f1"]), leaf(x["v"]), leaf(conv), leaf(layer)
    zb2 = [torch.zeros(N, D2, dtype=f64, requires_grad=True) for _ in range(S)]
    zb = [torch.zeros(N, 4 * A, dtype=f64, requires_grad=True) for _ in range(S)]
    zq = [torch.zeros(N, 1, A, dtype=f64, requires_grad=True) for _ in range(S)]
    p = {"att/location_conv/kernel": conv, "att/location_layer/kernel": layer, "att/query_layer/kernel": x["Wq"], "att/attention_v": v}
    O2.CELL_CLIP = x["cell_clip"] or None
    try:
        h, c, ctx, al = (torch.zeros(N, w, dtype=f64) for w in (A, A, E, Ti))
        hcs = []
        for s in range(S):
            pp = {"pre/dense_1/kernel": torch.cat([torch.eye(D1, dtype=f64), x["W1c"]], 0), "pre/dense_1/bias": torch.zeros(D1, dtype=f64),
                  "pre/dense_2/kernel": x["W2"], "pre/dense_2/bias": x["b2"] + zb2[s]}
            p2 = O2.prenet(torch.cat([f1[:, s + 1], ctx], 1), pp, "pre")
            xin = torch.cat([p2, x["spk"]], 1) if x.get("spk") is not None else p2
            c, h = O2.lstm_block_cell(xin, c, h, x["Watt"], x["batt"] + zb[s])
            al = O2.location_sensitive_alignments(h, al, keys + zq[s], x["lengths"], p, "att")
            ctx = torch.einsum("nt,nte->ne", al, values)
            hcs.append(torch.cat([h, ctx], 1))
    finally:
        O2.CELL_CLIP = None
    hc = torch.stack(hcs, 1)
    (hc * dhc[:, 1:]).sum().backward()
    st = lambda ts: torch.stack([t.grad.reshape(N, -1) for t in ts], 1)
    dwcl_conv = conv.grad[:, 0]                   # = dWcl . layer^T
    return dict(hc=hc.detach(), df1=f1.grad[:, 1:], dp2=st(zb2), dga=st(zb), dq=st(zq), dkeys=keys.grad, dvalues=values.grad,
                dv=v.grad, dconv=dwcl_conv, dlayer=layer.grad, conv=conv.detach()[:, 0], layer=layer.detach())


@pytest.mark.parametrize("kw,Dsp,lengths,clip", [(3, 0, (5, 5, 5), 0.0), (4, 2, (5, 1, 3), 0.0), (5, 0, (2, 5, 4), 0.3), (1, 1, (5, 4, 1), 0.3)])
def test_taco2_matches_autograd_on_the_oracle(kw, Dsp, lengths, clip):
    x, dhc = _tiny(3, 4, 5, 4, 3, 6, 4, kw, Dsp, lengths, clip, seed=kw + 7 * Dsp)
    got = R.taco2(x, dhc)
    want = _oracle_taco2(x, dhc)
    tol = lambda t: 1e-10 * max(1.0, float(t.abs().max()))
    assert float((got["hc"][:, 1:] - want["hc"]).abs().max()) <= tol(want["hc"])
    for k in ("df1", "dp2", "dga", "dq"):
        assert float((got[k][:, 1:] - want[k]).abs().max()) <= tol(want[k]), k
        assert float(got[k][:, 0].abs().max()) == 0.0, k
    for k in ("dkeys", "dvalues", "dv"):
        assert float((got[k] - want[k]).abs().max()) <= tol(want[k]), k
    # the folded filter's gradient, unfolded: d conv = dWcl . layer^T, d layer = conv^T . dWcl
    assert float((got["dwcl"] @ want["layer"].t() - want["dconv"]).abs().max()) <= tol(want["dconv"])
    assert float((want["conv"].t() @ got["dwcl"] - want["dlayer"]).abs().max()) <= tol(want["dlayer"])
    assert float(got["de"][~got["valid"][:, None, :].expand_as(got["de"])].abs().max() if (~got["valid"]).any() else 0) == 0.0
    if clip:
        assert bool((got["ca"].abs() == clip).any())


@pytest.mark.parametrize("Dsp,lengths", [(0, (5, 5, 5)), (2, (5, 1, 3))])
def test_taco1_matches_autograd_on_the_oracle(Dsp, lengths):
    x, dhc = _tiny(3, 4, 5, 4, 3, 6, 4, 0, Dsp, lengths, 0.0, seed=11 + Dsp, taco1=True)
    N, Ti, A = x["keys"].shape
    S, D1, D2 = 4, 6, 4
    got = R.taco1(x, dhc)
    f1 = x["f1"].clone().requires_grad_(True)
    zb2 = [torch.zeros(N, D2, dtype=f64, requires_grad=True) for _ in range(S)]
    zg = [torch.zeros(N, 2 * A, dtype=f64, requires_grad=True) for _ in range(S)]
    zc = [torch.zeros(N, A, dtype=f64, requires_grad=True) for _ in range(S)]
    zq = [torch.zeros(N, 1, A, dtype=f64, requires_grad=True) for _ in range(S)]
    p = {"att/query_layer/kernel": x["Wq"], "att/attention_v": x["v"]}
    h, ctx = torch.zeros(N, A, dtype=f64), torch.zeros(N, 3, dtype=f64)
    hcs = []
    for s in range(S):
        pp = {"pre/dense_1/kernel": torch.cat([torch.eye(D1, dtype=f64), x["W1c"]], 0), "pre/dense_1/bias": torch.zeros(D1, dtype=f64),
              "pre/dense_2/kernel": x["W2"], "pre/dense_2/bias": x["b2"] + zb2[s]}
        p2 = O2.prenet(torch.cat([f1[:, s + 1], ctx], 1), pp, "pre")
        xin = torch.cat([p2, x["spk"]], 1) if Dsp else p2
        h = O1.gru_cell(xin, h, x["Wg"], x["bg"] + zg[s], x["Wc"], x["bc"] + zc[s])
        al = O1.bahdanau_alignments(h, x["keys"] + zq[s], x["lengths"], p, "att")
        ctx = torch.einsum("nt,nte->ne", al, x["values"])
        hcs.append(torch.cat([h, ctx], 1))
    hc = torch.stack(hcs, 1)
    (hc * dhc[:, 1:]).sum().backward()
    st = lambda ts: torch.stack([t.grad.reshape(N, -1) for t in ts], 1)
    assert float((got["hc"][:, 1:] - hc.detach()).abs().max()) <= 1e-10
    for k, want in (("df1", f1.grad[:, 1:]), ("dp2", st(zb2)), ("dzg", st(zg)), ("dzc", st(zc)), ("dq", st(zq))):
        assert float((got[k][:, 1:] - want).abs().max()) <= 1e-10 * max(1.0, float(want.abs().max())), k


# --------------------------------------------------------------------------- hoisted operands and the single-step functions
def test_projected_memory_and_hoisted_da0_are_the_same_function():
    x, dhc = _tiny(3, 4, 5, 4, 3, 6, 4, 3, 0, (5, 2, 4), 0.0, seed=5)
    a, b = R.taco2(x, dhc), R.taco2(dict(x, pv=R.project_memory(x["values"], x["W1c"])), dhc)
    for k in R.TACO2_HIST + R.TACO2_GRAD:
        assert float((a[k] - b[k]).abs().max()) <= 1e-12, k
    # da0 is the part of d align that needs no recurrence: at the last step it is all of it
    da0 = R.hoisted_da0(dhc, x["values"], 4)
    al = a["align"][:, -1]
    da = da0[:, -1]
    want = al * (da - (al * da).sum(1, keepdim=True))
    assert float((a["de"][:, -1] - want).abs().max()) <= 1e-12


def test_single_step_functions_are_the_recurrence_one_step_at_a_time():
    kw, A, E = 4, 4, 3
    x, dhc = _tiny(3, 3, 6, A, E, 5, 4, kw, 0, (6, 2, 5), 0.0, seed=9)
    full = R.taco2(x, dhc)
    gk, carry = None, None
    for slot in (3, 2, 1):
        fw = R.attention_step(x["keys"], x["values"], full["q"][:, slot], full["align"][:, slot - 1], x["Wcl"], x["v"], x["lengths"])
        assert float((fw["align"] - full["align"][:, slot]).abs().max()) <= 1e-12
        assert float((fw["ctx"] - full["hc"][:, slot, A:]).abs().max()) <= 1e-12
        bw = R.attention_step_bwd(x["keys"], x["values"], full["q"][:, slot], full["align"][:, slot - 1], x["Wcl"], x["v"],
                                  x["lengths"], dhc[:, slot, A:], dctx_carry=carry, gk_next=gk)
        for k in ("de", "dq"):
            assert float((bw[k] - full[k][:, slot]).abs().max()) <= 1e-12, (k, slot)
        gk, carry = bw["gk"], full["df1"][:, slot] @ x["W1c"].t()


# ---------------------------------------------------------------------- the GPU module's shapes, tolerances and inputs
def _keys():
    seen = {}
    for c in G.ALL_CASES:
        seen.setdefault(G._data_key(c), c)
    return list(seen.values())


@pytest.mark.parametrize("c", _keys(), ids=G.case_id)
def test_no_relu_kink_lies_inside_the_noise(c):
    _, _, pure, _, emu32 = G.inputs(c)
    for z, (got, need) in G.kink_margin(c, pure, emu32).items():
        assert got >= need, (z, got, need)
    assert int((pure["z1"][:, 1:] > 0).sum()) > 0 and int((pure["z1"][:, 1:] < 0).sum()) > 0      # both branches are taken
    assert int((pure["z2"][:, 1:] > 0).sum()) > 0 and int((pure["z2"][:, 1:] < 0).sum()) > 0


def test_gpu_cases_cover_every_family_form_and_edge_shape():
    cases = G.ALL_CASES
    assert len(set(cases)) == len(cases)
    assert {c.family for c in cases} == {"step2", "cluster2", "cluster1"}
    step = [c for c in cases if c.family == "step2"]
    assert {(c.pv, c.fp, c.bp) for c in step} == {(pv, fp, bp) for pv in (False, True) for fp, bp in ((0, 0), (3, 3), (3, 1))}
    assert any(c.A % 16 for c in step)
    assert {(c.A, c.dtype) for c in cases if c.family == "cluster2"} == {(A, d) for A in (64, 256) for d in (G.f32, G.bf)}
    assert {(c.A, c.dtype) for c in cases if c.family == "cluster1"} == {(256, G.f32), (256, G.bf)}
    want = {(1, 1, 1, 7), (3, 4, 9, 7), (2, 5, 70, 8), (2, 5, 70, 5), (2, 3, 256, 7), (2, 3, 13, 1), (4, 9, 20, 7)}
    for fam in ("step2", "cluster2", "cluster1"):
        have = {(c.shape.N, c.shape.S, c.shape.Ti, c.shape.kw) for c in cases if c.family == fam}
        assert want <= have, (fam, want - have)
        assert {c.shape.N for c in cases if c.family == fam} >= ({33} if fam != "cluster1" else {32, 1})
    assert all(c.shape.S <= 9 and c.shape.N <= 33 for c in cases)
    assert any(G.tia_of(c.shape) > (c.shape.Ti + 7) // 8 * 8 for c in cases)
    assert {o.dtype for o in G.ONE_CASES} == {G.f32, G.bf} and {bool(o.E2) for o in G.ONE_CASES} == {False, True}
    assert {o.out2 for o in G.ONE_CASES} == {False, True}


@pytest.mark.parametrize("c", _keys(), ids=G.case_id)
def test_gpu_inputs_exercise_what_the_cases_are_for(c):
    x, dhc, pure, _, _ = G.inputs(c)
    s = c.shape
    L = x["lengths"]
    assert int(L.max()) == s.Ti and int(L.min()) >= 1
    if s.clip and c.family != "cluster1":          # the clip is reached, and not everywhere
        at = float((pure["ca"][:, 1:].abs() == s.clip).double().mean())
        assert 0.05 <= at <= 0.8, at
    if s.name in ("n3s4t9", "n4s9t20-spk-clip") or s.N >= 32:      # a row with fewer valid positions than workgroups
        assert int(L.min()) < 8 and int(L.max()) >= 9
    if s.Ti == 256:                                # a slice of the cluster holds ceil(length / 8) = 32 = TSMAX positions
        assert all((int(l) + 7) // 8 == 32 for l in L) and any(int(l) % 32 for l in L)
    if s.name == "n1s1t1":
        assert (s.N, s.S, s.Ti) == (1, 1, 1)
    if s.Dsp:                                      # the speaker rows matter
        bad = G._ref_fn(c)(x, dhc, plant=("no_speaker_rows",))
        assert float((bad["hc"] - pure["hc"]).abs().max()) > 1e-2
    for k in G.hist_names(c) + G.grad_names(c):    # nothing compared later is all but zero
        if s.Ti == 1 and k in ("dq", "de", "dkeys", "dv", "dwcl"):
            continue                               # one position: the softmax is constant, its gradients are exactly 0
        assert float(G._cut(c, k, pure[k]).abs().max()) >= 1e-4, k


def _applies(plant, c):
    s = c.shape
    taco2 = c.family != "cluster1"
    return dict(taps_shifted=taco2 and s.S >= 2 and s.Ti >= 2, mask_len_plus1=min(s.lengths) < s.Ti,
                drop_slice_last=c.family != "step2" and s.Ti >= 2, no_energy_carry=taco2 and s.S >= 2 and s.Ti >= 2,
                no_clip_bwd=taco2 and s.clip > 0, no_speaker_rows=s.Dsp > 0, gru_rh_is_h=not taco2 and s.S >= 2,
                dwcl_no_padding=taco2 and s.S >= 2 and s.Ti >= 2 and s.kw >= 2)[plant]


@functools.lru_cache(maxsize=None)
def _planted(key, plant):
    c = next(c for c in G.ALL_CASES if G._data_key(c) == key)
    x, dhc, _, _, _ = G.inputs(c)
    return G._ref_fn(c)(x, dhc, plant=(plant,))


def _caught(c, plant):
    """Would the GPU test of case c fail on a kernel that computes the planted function (to within its own error)?  As in
    test_lstm_ref_cpu.py: the plant is caught when it moves a buffer by more than bound + e against the pure
    reference, e = the error the bound grants a correct kernel (fp32 rule: the bound itself; bf16 rule: the
    storage-exact reference's own distance), in the maximum or in the mean - or leaves something other than 0 from a
    row's length on, which the GPU test asserts exactly."""
    ref = G.references(c)
    bad = _planted(G._data_key(c), plant)
    pure = ref["pure"]
    past = ~pure["valid"]
    for k in G.hist_names(c) + G.grad_names(c):
        if k in ("align", "de") and bool((bad[k][:, 1:][past[:, None, :].expand_as(bad[k][:, 1:])] != 0).any()):
            return True
        pmax, pmean = G._dist(G._cut(c, k, bad[k]), G._cut(c, k, pure[k]))
        against, bmax, bmean = ref["bounds"][k][-1]
        assert against == "pure"
        fig = ref["figures"].get(k)
        if pmax > bmax + (fig["storage_max"] if fig else bmax):
            return True
        if bmean is not None and pmean > bmean + fig["storage_mean"]:
            return True
    return False


@pytest.mark.parametrize("plant", R.PLANTS)
def test_planted_errors_are_caught_at_every_gpu_shape(plant):
    missed, tried = [], 0
    for c in G.ALL_CASES:
        if _applies(plant, c):
            tried += 1
            if not _caught(c, plant):
                missed.append(G.case_id(c))
    assert tried and not missed, missed


@pytest.mark.parametrize("o", G.ONE_CASES, ids=G.one_id)
def test_planted_errors_are_caught_by_the_single_step_cases(o):
    x = G.one_inputs(o)
    a = (x["keys"], x["values"], x["q"], x["aprev"], x["Wcl"], x["v"], x["lengths"])
    ref = R.attention_step(*a, pv=x["pv"])
    names = ["align", "ctx"]
    emu = R.attention_step(*a, pv=x["pv"], dtype=torch.float32)
    bounds = G._one_bounds(ref, emu, names, names, stored_bf16=("ctx",) if o.dtype == G.bf else ())["bounds"]
    for plant in ("taps_shifted", "mask_len_plus1"):
        if plant == "mask_len_plus1" and min(o.lengths) == o.Ti:
            continue
        bad = R.attention_step(*a, pv=x["pv"], plant=(plant,))
        assert any(G._dist(bad[k], ref[k])[0] > 2 * bounds[k][-1][1] for k in names), plant
    rb = R.attention_step_bwd(*a, x["dctx"], dctx_carry=x["carry"], gk_next=x["gk"])
    bb = R.attention_step_bwd(*a, x["dctx"], dctx_carry=x["carry"], gk_next=x["gk"], plant=("no_energy_carry",))
    names = ["da", "de", "dq", "gk"]
    eb = R.attention_step_bwd(*a, x["dctx"], dctx_carry=x["carry"], gk_next=x["gk"], dtype=torch.float32)
    bounds = G._one_bounds(rb, eb, names, (), stored_bf16=("dq",) if o.dtype == G.bf else ())["bounds"]
    assert any(G._dist(bb[k], rb[k])[0] > 2 * bounds[k][-1][1] for k in names)
