"""tests/gru_ref.py must not be wrong the way a kernel is.  No GPU.

The pure forward against explicit scalar loops; the pure backward against torch.autograd on an independent float64
forward (oracle/taco1_oracle.py: gru_cell under the masking loop of bigru) for every combination of reverse, lengths and
h_init; the windowed evaluation against the whole-sequence one; and, for every case of tests/test_gru_contract_gpu.py,
that the case's shape and tolerances catch each of thirteen planted errors its features can show, that its inputs
exercise what the case is there for, and that the float32 emulation in other summation orders stays inside the bounds
the GPU module derives from one."""
import functools
import math

import pytest
import torch

import gru_ref as R
import test_gru_contract_gpu as G
from oracle import taco1_oracle as O

pytestmark = []                                  # (the import above must not lend this module its gpu mark)


# ------------------------------------------------------------------------------------------------- scalar restatement
def _scalar_forward(xg, xc, Wg, Wc, lengths, reverse, h0):
    """The header's sentences one number at a time: nested lists h [N][T][H] (zeros past the length)."""
    N, T, H = len(xg), len(xg[0]), len(Wc)
    sg = lambda v: 1.0 / (1.0 + math.exp(-v))
    h = [[[0.0] * H for _ in range(T)] for _ in range(N)]
    ru = [[None] * T for _ in range(N)]
    for n in range(N):
        length = T if lengths is None else lengths[n]
        hp = [0.0] * H if h0 is None else list(h0[n])
        for t in (range(length - 1, -1, -1) if reverse else range(length)):      # the reverse direction starts at length - 1
            z = [xg[n][t][k] + sum(hp[v] * Wg[v][k] for v in range(H)) for k in range(2 * H)]
            r, u = [sg(v) for v in z[:H]], [sg(v) for v in z[H:]]
            c = [math.tanh(xc[n][t][k] + sum(r[v] * hp[v] * Wc[v][k] for v in range(H))) for k in range(H)]
            hp = [u[k] * hp[k] + (1 - u[k]) * c[k] for k in range(H)]
            h[n][t], ru[n][t] = hp, r + u
    return h, ru


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("with_h0", [False, True])
@pytest.mark.parametrize("N,T,lengths", [(1, 1, None), (3, 3, None), (4, 3, [3, 1, 2, 0]), (2, 4, [2, 4])])
def test_pure_forward_matches_scalar_loops(N, T, lengths, with_h0, reverse):
    H = 4
    g = torch.Generator().manual_seed(N * 10 + T)
    xg, xc = (torch.randn(N, T, k * H, generator=g, dtype=torch.float64) * 2 for k in (2, 1))
    Wg, Wc = (torch.randn(H, k * H, generator=g, dtype=torch.float64) for k in (2, 1))
    h0 = torch.randn(N, H, generator=g, dtype=torch.float64) if with_h0 else None
    L = None if lengths is None else torch.tensor(lengths)
    got = R.gru_seq(xg, xc, Wg, Wc, lengths=L, reverse=reverse, h_init=h0)
    h, ru = _scalar_forward(xg.tolist(), xc.tolist(), Wg.tolist(), Wc.tolist(), lengths, reverse, None if h0 is None else h0.tolist())
    assert float((got["h"] - torch.tensor(h, dtype=torch.float64)).abs().max()) <= 1e-12
    for n in range(N):
        for t in range(T):
            assert bool(got["valid"][n, t]) == (ru[n][t] is not None)
            if ru[n][t] is not None:
                assert float((got["ru"][n, t] - torch.tensor(ru[n][t], dtype=torch.float64)).abs().max()) <= 1e-12


# --------------------------------------------------------------------------------------------- the backward, by autograd
def _oracle_run(xg, xc, Wg, Wc, lengths, reverse, h0, dh):
    """An independent float64 forward - the oracle's bigru (gru_cell under its masking loop) - and autograd.  The cell
    takes [x, h] . kernel: x = [xg | xc] with kernel = [selector; W] makes the hoisted input halves."""
    N, T, H = xc.shape
    x = torch.cat([xg, xc], 2).clone().requires_grad_(True)
    h0v = None if h0 is None else h0.clone().requires_grad_(True)
    eye = torch.eye(3 * H, dtype=torch.float64)
    p = {}
    for d in ("fw", "bw"):
        pre = "s/%s/gru_cell" % d
        p[pre + "/gates/kernel"], p[pre + "/candidate/kernel"] = torch.cat([eye[:, :2 * H], Wg], 0), torch.cat([eye[:, 2 * H:], Wc], 0)
        p[pre + "/gates/bias"], p[pre + "/candidate/bias"] = torch.zeros(2 * H, dtype=torch.float64), torch.zeros(H, dtype=torch.float64)
    y = O.bigru(x, lengths, p, "s", H, h0=h0v)[:, :, H:] if reverse else O.bigru(x, lengths, p, "s", H, h0=h0v)[:, :, :H]
    (y * dh).sum().backward()
    return y.detach(), x.grad[:, :, :2 * H], x.grad[:, :, 2 * H:], None if h0v is None else h0v.grad


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("with_h0", [False, True])
@pytest.mark.parametrize("N,T,H", [(1, 1, 4), (5, 7, 8), (6, 9, 16)])
def test_pure_backward_matches_autograd_on_the_oracle(N, T, H, with_h0, masked, reverse):
    g = torch.Generator().manual_seed(N + T + H)
    xg, xc = (torch.randn(N, T, k * H, generator=g, dtype=torch.float64) for k in (2, 1))
    Wg, Wc = (torch.randn(H, k * H, generator=g, dtype=torch.float64) / H ** 0.5 for k in (2, 1))
    dh = torch.randn(N, T, H, generator=g, dtype=torch.float64)
    h0 = torch.randn(N, H, generator=g, dtype=torch.float64) if with_h0 else None
    lengths = None
    if masked:
        lengths = torch.randint(1, T + 1, (N,), generator=g)
        lengths[0], lengths[-1] = T, 1
        if N > 2:
            lengths[1] = 0
    got = R.gru_seq(xg, xc, Wg, Wc, lengths=lengths, reverse=reverse, h_init=h0, dh=dh)
    h, dxg, dxc, dh0 = _oracle_run(xg, xc, Wg, Wc, lengths, reverse, h0, dh)
    for k, want in (("h", h), ("dzg", dxg), ("dzc", dxc)) + ((("dh_init", dh0),) if with_h0 else ()):
        assert float((got[k] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), k
    past = ~got["valid"]
    for k in ("h", "dzg", "dzc"):
        assert not past.any() or float(got[k][past].abs().max()) == 0.0, k


@pytest.mark.parametrize("with_h0", [False, True])
def test_windowed_evaluation_is_the_whole_sequence(with_h0):
    N, T, H = 3, 11, 8
    g = torch.Generator().manual_seed(5)
    xg, xc = (torch.randn(N, T, k * H, generator=g, dtype=torch.float64) for k in (2, 1))
    Wg, Wc = (torch.randn(H, k * H, generator=g, dtype=torch.float64) / H ** 0.5 for k in (2, 1))
    dh = torch.randn(N, T, H, generator=g, dtype=torch.float64)
    h0 = torch.randn(N, H, generator=g, dtype=torch.float64) if with_h0 else None
    whole = R.gru_seq(xg, xc, Wg, Wc, h_init=h0, dh=dh)
    cut = R.gru_seq(xg, xc, Wg, Wc, h_init=h0, dh=dh, windows=G.WINDOWS)
    for k in G.BUFFERS:
        assert float((whole[k] - cut[k]).abs().max()) <= 1e-13, k
    # with a bf16 history the window edges round the state: the arrangement is another function
    a, b = (R.gru_seq(xg, xc, Wg, Wc, h_init=h0, dh=dh, rounding=R.PRESETS["bf16"], windows=w) for w in (None, G.WINDOWS))
    assert torch.equal(a["h"][:, :3], b["h"][:, :3]) and not torch.equal(a["c"][:, 3:], b["c"][:, 3:])


# ------------------------------------------------------------------------- the GPU module's shapes, tolerances and inputs
def _shape_key(c):
    return (c.H, G.FORMS[c.form][0] == G.bf) + tuple(c[2:8])     # what the pure reference depends on (bf16: rounded weights)


@functools.lru_cache(maxsize=None)
def _planted(key, plant, di):
    """The pure reference of a case's direction with one error planted (shared by the forms of a shape)."""
    c = next(c for c in G.CASES if _shape_key(c) == key)
    lengths, dirs = G.inputs(c)
    d = dirs[di]
    return R.gru_seq(d["xg"], d["xc"], d["Wg"], d["Wc"], lengths=lengths, reverse=c.dirs[di], h_init=d["h0"], dh=d["dh"],
                     windows=G.windows_of(c), plant=(plant,), dh_init_prefill=G.SENTINEL)


def _applies(plant, c, reverse):
    """Can the case's direction show the planted error at all?"""
    lengths, _ = G.inputs(c)
    short = c.masked and bool((lengths < c.T).any())
    return dict(mask_gt=short, state_zeroed_masked=short and reverse, reverse_start_T=short and reverse,
                first_hprev_from_history=c.h0, swap_u=True, reset_after=c.T >= 2 or c.h0, swap_ru=True, dzu_from_h=True,
                carry_no_drh_r=True, carry_no_dh_u=True, dh_on_masked=short, dh_init_accumulate=True,
                window_no_handover=c.opt == "windows")[plant]


def _caught(c, di, plant):
    """Would the GPU test of case c fail on a kernel that computes the planted reference (to within its own error)?
    A kernel that meets a bound b against the pure reference while computing the planted function has the planted
    function within b + e of the pure one, e = the error the bound grants a correct kernel (fp32 rule: b itself; bf16
    rule: the storage-exact reference's own distance).  So the plant is caught when it moves a buffer by more than
    b + e in the maximum or in the mean - or leaves something other than 0 past a row's length in h, dzg or dzc, which
    the GPU test asserts exactly."""
    ref = G.references(c)[di]
    bad = _planted(_shape_key(c), plant, di)
    pure = ref["pure"]
    for k in G.BUFFERS:
        if k in ("h", "dzg", "dzc") and bool((bad[k][~pure["valid"]] != 0).any()):
            return True
        valid = G._valid(pure, k)
        pmax, pmean, _ = G._dist(bad[k], pure[k], valid)
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
    for c in G.CASES:
        for di, reverse in enumerate(c.dirs):
            if _applies(plant, c, reverse):
                tried += 1
                if not _caught(c, di, plant):
                    missed.append((G.case_id(c), di))
    assert tried and not missed, missed


def test_gpu_cases_cover_what_the_issue_lists():
    cases = G.CASES
    assert len(set(c[:8] for c in cases)) == len(cases) and all(c.why for c in cases)
    assert {c.N for c in cases} == {1, 5, 16, 17, 33} and {c.T for c in cases} == {1, 2, 3, 4, 13, 11, 40}
    for H in (128, 256):
        for form in G.FORMS:
            mine = [c for c in cases if (c.H, c.form) == (H, form)]
            assert {1, 2, 3} <= {c.T for c in mine}, (H, form)
            assert any(c.N % 16 for c in mine if c.N > 16) and any(c.N < 16 for c in mine), (H, form)
            assert any(c.masked for c in mine) and any(c.masked and c.h0 and True in c.dirs for c in mine), (H, form)
            assert any(len(c.dirs) == 1 for c in mine) and any(c.dirs == G.FB for c in mine), (H, form)
            assert sum(c.opt == "windows" for c in mine) == 1, (H, form)
        assert any(c.H == H and c.dirs == G.FF for c in cases) and any(c.H == H and c.opt == "len0" for c in cases)
    for form in G.FORMS:
        assert sum(c.T == 40 and c.form == form for c in cases) == 1
    assert all(G.windows_of(c) == [(0, 3), (3, 4), (4, 11)] and c.T == 11 for c in cases if c.opt == "windows")


def test_gpu_inputs_exercise_what_the_cases_are_for():
    for c in G.CASES:
        lengths, dirs = G.inputs(c)
        if c.masked:
            assert int(lengths.max()) == c.T and 1 in lengths.tolist() and c.N > 1, G.case_id(c)
            assert (0 in lengths.tolist()) == (c.opt == "len0"), G.case_id(c)
        if c.dirs == G.FF:
            assert not torch.equal(dirs[0]["Wg"], dirs[1]["Wg"]) and not torch.equal(dirs[0]["Wc"], dirs[1]["Wc"])
        for d, ref in zip(dirs, G.references(c)):
            pure = ref["pure"]
            if c.masked and (lengths < c.T).any():                   # dh past the length is there to be ignored
                assert float(d["dh"][~pure["valid"]].abs().min()) > 0
            for k in G.BUFFERS:                  # nothing compared later is all but zero
                valid = G._valid(pure, k)
                if c.T == 1 and not c.h0 and k == "rh":
                    continue                     # r * 0
                assert G._dist(pure[k], pure[k], valid)[2] >= (1e-3 if k in ("dzg", "dzc", "dh_init") else 1e-1), (G.case_id(c), k)


def test_float32_emulation_in_other_orders_stays_inside_the_bounds():
    """What the GPU module allows a kernel, an fp32 evaluation of the arrangement meets in any summation order."""
    worst = 0.0
    for c in G.CASES:
        lengths, dirs = G.inputs(c)
        preset = R.PRESETS[c.form]
        for di, (d, ref) in enumerate(zip(dirs, G.references(c))):
            for seed in (1, 2, 3):
                perm = torch.randperm(c.H, generator=torch.Generator().manual_seed(seed))
                emu = R.gru_seq(d["xg"], d["xc"], d["Wg"], d["Wc"], lengths=lengths, reverse=c.dirs[di], h_init=d["h0"], dh=d["dh"],
                                windows=G.windows_of(c), rounding=preset, dtype=torch.float32, perm=perm)
                for k in G.BUFFERS:
                    for against, bmax, bmean in ref["bounds"][k]:
                        emax, emean, _ = G._dist(emu[k], ref[against][k], G._valid(ref["pure"], k))
                        ratio = max(G.ratio(emax, bmax), G.ratio(emean, bmean) if bmean is not None else 0.0)
                        worst = max(worst, ratio)
                        assert ratio <= 1.0, (G.case_id(c), di, seed, k, against, emax, bmax, emean, bmean)
    print("worst float32 emulation / bound: %.2f" % worst)
