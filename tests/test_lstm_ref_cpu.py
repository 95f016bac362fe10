"""tests/lstm_ref.py must not be wrong the way a kernel is.  No GPU.

The pure forward against explicit scalar loops; the pure backward against torch.autograd on an independent float64
forward (oracle/taco2_oracle.py: lstm_block_cell / zoneout_cell under the masking loop of bilstm); the mask generator
against the oracle's and against ns_zone_keep restated in scalar Python; and, for every case of
tests/test_lstm_contract_gpu.py, that the case's shape and tolerances catch each of nine planted errors and that its
inputs exercise what the case is there for."""
import functools
import math

import numpy as np
import pytest
import torch

import lstm_ref as R
import test_lstm_contract_gpu as G
from oracle import taco2_oracle as O

pytestmark = []                                  # (the import above must not lend this module its gpu mark)


# ------------------------------------------------------------------------------------------------- scalar restatements
def _fmix(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    return x ^ (x >> 16)


def _keep(seed, t, n, u, thr):
    """csrc/common.h: ns_zone_keep, one (t, n, u) at a time in Python integers."""
    x = _fmix(seed ^ ((t * 0x9E3779B9) & 0xFFFFFFFF))
    x = _fmix(x ^ ((n * 0x7FEB352D) & 0xFFFFFFFF))
    x = _fmix(x ^ ((u * 0x846CA68B) & 0xFFFFFFFF))
    return (x >> 8) < thr


def _scalar_forward(xg, W, lengths, reverse, fb, clip, zone):
    """The header's sentences one number at a time: nested lists h, c [N][T][H] and gates [N][T][4H]."""
    N, T, H = len(xg), len(xg[0]), len(W)
    sg = lambda v: 1.0 / (1.0 + math.exp(-v))
    h = [[[0.0] * H for _ in range(T)] for _ in range(N)]
    c = [[[0.0] * H for _ in range(T)] for _ in range(N)]
    gates = [[[0.0] * 4 * H for _ in range(T)] for _ in range(N)]
    for n in range(N):
        length = T if lengths is None else lengths[n]
        hp, cp = [0.0] * H, [0.0] * H            # zero before the first step; the reverse direction starts at length - 1
        for t in (range(length - 1, -1, -1) if reverse else range(length)):
            z = [xg[n][t][k] + sum(hp[v] * W[v][k] for v in range(H)) for k in range(4 * H)]
            hn, cn = [0.0] * H, [0.0] * H
            for u in range(H):
                i, j, f, o = sg(z[u]), math.tanh(z[H + u]), sg(z[2 * H + u] + fb), sg(z[3 * H + u])
                c2 = f * cp[u] + i * j
                if clip > 0:
                    c2 = min(max(c2, -clip), clip)
                h2 = o * math.tanh(c2)
                if zone is not None:
                    thr_c, thr_h, seed_c, seed_h = zone
                    if _keep(seed_c, t, n, u, thr_c):
                        c2 = cp[u]
                    if _keep(seed_h, t, n, u, thr_h):
                        h2 = hp[u]
                hn[u], cn[u] = h2, c2
                gates[n][t][u], gates[n][t][H + u], gates[n][t][2 * H + u], gates[n][t][3 * H + u] = i, j, f, o
            h[n][t], c[n][t] = hn, cn
            hp, cp = hn, cn
    return h, c, gates


ZONE = (R.zone_threshold(0.4), R.zone_threshold(0.3), 0xC0FFEE, 0xFACADE)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("N,T,lengths,fb,clip,zone", [
    (1, 1, None, 1.0, 0.0, None), (3, 3, None, 0.25, 0.0, None), (3, 3, [3, 1, 2], 0.25, 0.0, None),
    (2, 3, [2, 3], 1.0, 0.4, None), (3, 3, None, 0.25, 0.0, ZONE), (3, 3, [1, 3, 2], 0.25, 0.4, ZONE)])
def test_pure_forward_matches_scalar_loops(N, T, lengths, fb, clip, zone, reverse):
    H = 4
    g = torch.Generator().manual_seed(N * 10 + T)
    xg = torch.randn(N, T, 4 * H, generator=g, dtype=torch.float64) * 2
    W = torch.randn(H, 4 * H, generator=g, dtype=torch.float64)
    L = None if lengths is None else torch.tensor(lengths)
    got = R.lstm_seq(xg, W, lengths=L, reverse=reverse, forget_bias=fb, cell_clip=clip, zoneout=zone)
    h, c, gates = _scalar_forward(xg.tolist(), W.tolist(), lengths, reverse, fb, clip, zone)
    for k, want in (("h", h), ("c", c), ("gates", gates)):
        assert float((got[k] - torch.tensor(want, dtype=torch.float64)).abs().max()) <= 1e-12, k
    if zone is not None:                         # the case does keep units, and not all of them
        kept = [_keep(zone[2], t, n, u, zone[0]) for t in range(T) for n in range(N) for u in range(H)]
        assert 0 < sum(kept) < len(kept)


# --------------------------------------------------------------------------------------------- the backward, by autograd
def _oracle_run(xg, W, lengths, reverse, clip, zone, dh, monkeypatch):
    """An independent float64 forward - the oracle's cells under bilstm's masking loop (the state freezes past the
    length) - and autograd for d sum(h dh) / d xg.  The cell takes [x, h].kernel: kernel = [identity; W] makes x = xg."""
    monkeypatch.setattr(O, "CELL_CLIP", clip)
    N, T, G4 = xg.shape
    H = G4 // 4
    x = xg.clone().requires_grad_(True)
    kernel = torch.cat([torch.eye(G4, dtype=torch.float64), W], 0)
    bias = torch.zeros(G4, dtype=torch.float64)
    L = torch.full((N,), T) if lengths is None else lengths.long()
    c, h = x.new_zeros(N, H), x.new_zeros(N, H)
    if zone is not None:
        kc, kh = O.zoneout_masks(zone[2], zone[0], T, N, H), O.zoneout_masks(zone[3], zone[1], T, N, H)
    hs, cs = [None] * T, [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        if zone is None:
            c2, h2 = O.lstm_block_cell(x[:, t], c, h, kernel, bias)
        else:
            c2, h2 = O.zoneout_cell(x[:, t], c, h, kernel, bias, keep_c=kc[t], keep_h=kh[t])
        m = (t < L).to(x.dtype)[:, None]
        c, h = m * c2 + (1 - m) * c, m * h2 + (1 - m) * h
        hs[t], cs[t] = m * h2, m * c2
    hh = torch.stack(hs, 1)
    (hh * dh).sum().backward()
    return hh.detach(), torch.stack(cs, 1).detach(), x.grad


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("N,T,H,masked,clip,zone", [(1, 1, 4, False, 0.0, False), (4, 6, 8, False, 0.0, False),
                                                      (5, 7, 8, True, 0.0, False), (5, 7, 8, True, 0.6, False),
                                                      (5, 7, 8, True, 0.0, True), (6, 9, 16, True, 0.6, True)])
def test_pure_backward_matches_autograd_on_the_oracle(N, T, H, masked, clip, zone, reverse, monkeypatch):
    g = torch.Generator().manual_seed(N + T + H)
    xg = torch.randn(N, T, 4 * H, generator=g, dtype=torch.float64) * (2 if clip else 1)
    W = torch.randn(H, 4 * H, generator=g, dtype=torch.float64) / H ** 0.5
    dh = torch.randn(N, T, H, generator=g, dtype=torch.float64)
    lengths = None
    if masked:
        lengths = torch.randint(1, T + 1, (N,), generator=g)
        lengths[0], lengths[-1] = T, 1
    z = ZONE if zone else None
    got = R.lstm_seq(xg, W, lengths=lengths, reverse=reverse, forget_bias=1.0, cell_clip=clip, zoneout=z, dh=dh)
    h, c, dxg = _oracle_run(xg, W, lengths, reverse, clip, z, dh, monkeypatch)
    for k, want in (("h", h), ("c", c), ("dgates", dxg)):
        assert float((got[k] - want).abs().max()) <= 1e-12 * float(want.abs().max()), k
    if clip:
        assert bool((got["c"].abs() == clip).any())


# ------------------------------------------------------------------------------------------------------ the mask generator
def test_mask_generator_is_the_oracles_and_the_kernels():
    for seed, rate, T, N, H in ((0, 0.25, 5, 3, 16), (0xFFFFFFFF, 0.5, 70, 40, 8), (0x9E3779B9, 0.1, 3, 130, 1024)):
        thr = R.zone_threshold(rate)
        m = R.zone_masks(seed, thr, T, N, H)
        assert m.dtype == np.bool_ and np.array_equal(m, O.zoneout_masks(seed, thr, T, N, H))
        for t, n, u in ((0, 0, 0), (T - 1, N - 1, H - 1), (T // 2, 1, 3), (1, N // 2, H - 2), (T - 1, 0, 7)):
            assert bool(m[t, n, u]) == _keep(seed, t, n, u, thr), (seed, t, n, u)
    from nspeech_amd import ops
    assert R.zone_threshold(0.25) == ops.zoneout_threshold(0.25) == 1 << 22


# ------------------------------------------------------------------------- the GPU module's shapes, tolerances and inputs
def _shape_key(c):
    return c[2:10]                               # N, T, H, dirs, masked, fb, clip, zone: what the pure reference depends on


@functools.lru_cache(maxsize=None)
def _planted(key, form_dtype_is_bf16, plant, di):
    """The pure reference of a case's direction with one error planted (shared by the forms of a shape)."""
    c = next(c for c in G.ALL_CASES if _shape_key(c) == key and (G.FORMS[c.form].dtype == G.bf) == form_dtype_is_bf16)
    lengths, dirs = G.inputs(c)
    d = dirs[di]
    return R.lstm_seq(d["xg"], d["W"], lengths=lengths, reverse=c.dirs[di], forget_bias=c.fb, cell_clip=c.clip,
                      zoneout=G.zone_of(c), dh=d["dh"], plant=(plant,))


def _applies(plant, c, reverse):
    return dict(no_forget_bias=True, swap_jf=True, mask_gt=c.masked, no_reverse_restart=c.masked and reverse,
                clip_masked_grad=bool(c.clip), zone_by_step=c.zone and reverse, zone_swap_masks=c.zone, no_dh_carry=c.zone,
                dc_carry_no_f=c.T >= 2)[plant]


def _caught(c, di, plant):
    """Would the GPU test of case c fail on a kernel that computes the planted reference (to within its own error)?
    A kernel that meets a bound b against the pure reference while computing the planted function has the planted
    function within b + e of the pure one, e = the error the bound grants a correct kernel (fp32 rule: b itself; bf16
    rule: the storage-exact reference's own distance).  So the plant is caught when it moves a buffer by more than
    b + e in the maximum or in the mean - or leaves something other than 0 past a row's length, which the GPU test
    asserts exactly."""
    ref = G.references(c)[di]
    bad = _planted(_shape_key(c), G.FORMS[c.form].dtype == G.bf, plant, di)
    pure = ref["pure"]
    for k in G.BUFFERS:
        if bool((bad[k][~pure["valid"]] != 0).any()):
            return True
        pmax, pmean, _ = G._dist(bad[k], pure[k], pure["valid"])
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
        for di, reverse in enumerate(c.dirs):
            if _applies(plant, c, reverse):
                tried += 1
                if not _caught(c, di, plant):
                    missed.append((G.case_id(c), di))
    assert tried and not missed, missed


def test_gpu_cases_cover_what_the_issue_lists():
    cases = G.ALL_CASES
    assert len(set(cases)) == len(cases)
    assert sum(c.padl > 0 and c.tail > 0 for c in cases) * 2 >= len(cases) and any(c.padl == 0 for c in cases)
    for fam in ("step", "cluster", "wide"):
        assert sum(c.T == 25 for c in cases if c.family == fam) >= 1
        assert all(c.T <= 13 or c.T == 25 for c in cases if c.family == fam)
    step = [c for c in cases if c.family == "step"]
    assert {c.form for c in step} == {"f32x0", "f32x3", "f32x3s", "f32x1", "f32x1b", "bf16"}
    assert {(c.N, c.H) for c in step} >= {(1, 16), (33, 48), (33, 16), (17, 256), (129, 256)} and {1, 2, 3} <= {c.T for c in step}
    assert any(c.zone and c.dirs == G.B and c.masked for c in step) and any(c.zone and c.dirs == G.F for c in step)
    clu = [c for c in cases if c.family == "cluster"]
    assert {c.H for c in clu if c.form == "bf16"} >= {64, 128, 192, 512} and {c.N for c in clu} >= {1, 5, 17}
    assert {c.H for c in clu if c.form == "f32state"} == {64, 256} and {c.T for c in clu} >= {2, 3, 9, 25}
    assert sorted(c.opt for c in clu if c.opt) == [4, 8, 16]
    wide = [c for c in cases if c.family == "wide"]
    assert {c.H for c in wide} == {256, 1024} and {c.N for c in wide} >= {1, 17, 32, 60} and {c.T for c in wide} >= {2, 3, 9}
    for form in ("wide_bf16", "wide_mixed", "wide_planes"):
        assert any(c.form == form and c.zone for c in wide), form
    assert all(c.dirs == G.F for c in wide)      # ns_lstm_wide_* take reverse == 0 only


def test_gpu_inputs_exercise_what_the_cases_are_for():
    seen = set()
    for c in G.ALL_CASES:
        key = (_shape_key(c), G.FORMS[c.form].dtype == G.bf)
        if key in seen:
            continue
        seen.add(key)
        lengths, _ = G.inputs(c)
        if c.masked:
            assert int(lengths.min()) == 1 and int(lengths.max()) == c.T and c.N > 1, G.case_id(c)
        if c.zone:
            for thr, seed in zip(G.zone_of(c)[:2], G.zone_of(c)[2:]):
                kept = R.zone_masks(seed, thr, c.T, c.N, c.H).mean()
                assert 0.15 <= kept <= 0.35, (G.case_id(c), kept)
        for ref in G.references(c):
            pure = ref["pure"]
            v = pure["valid"][:, :, None].expand_as(pure["c"])
            if c.clip:
                at = float((pure["c"][v].abs() == c.clip).double().mean())
                assert at >= 0.05 and 1 - at >= 0.20, (G.case_id(c), at)
            for k in G.BUFFERS:                  # nothing compared later is all but zero
                assert float(pure[k][pure["valid"]].abs().max()) >= (1e-3 if k == "dgates" else 1e-1), (G.case_id(c), k)
