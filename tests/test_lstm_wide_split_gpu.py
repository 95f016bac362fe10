"""The split form of the wide forward kernel (csrc/lstm_wide.hip: with fp32 storage and the planes h_bf16 / h_lo_bf16 the
state travels pre-split as hi = bf16(h), lo = bf16(h - hi) instead of as fp32, and the planes are outputs) against the
same call without planes, in the same build: h, c and the gates bit for bit, the planes bit for bit what
ops.split_hi_lo makes of the fp32 h.  Pad rows and rows behind a row's length stay zero in both planes, no sentinel is
left, the status word is 0 and a second launch writes the same bits.  Shapes: H = 256 (one K chunk per sweeper) with one row, a short row group, a second row group of one row and
the full batch, from the first step that sweeps (T = 2) on; one case at H = 1024 for the chunk loop."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _lengths(N, T):
    # hand-set: a row of length 1, full rows and every length between
    return torch.tensor([(1, T, max(1, T - 1), max(1, T // 2))[i % 4] for i in range(N)], dtype=torch.int32)


def _data(dev, N, T, H, seed, masked):
    g = torch.Generator().manual_seed(seed)
    rows = N * (T + 1)
    whT = (torch.randn(4 * H, H, generator=g) / H ** 0.5).to(dev)
    hi = whT.bfloat16()
    return dict(N=N, T=T, H=H, xg=torch.randn(rows, 4 * H, generator=g).to(dev), whT=whT, hi=hi,
                lo=(whT - hi.float()).bfloat16(), lengths=_lengths(N, T).to(dev) if masked else None)


def _fwd(dev, d, planes, zoneout=None, forget_bias=1.0, launches=1):
    from nspeech_amd import ops
    N, T, H = d["N"], d["T"], d["H"]
    P, padl = T + 1, 1                       # the decoder's slot layout: slot 0 = zero initial state
    rows = N * P
    out = dict(h=torch.zeros(rows * H, device=dev), c=torch.zeros(rows * H, device=dev), g=torch.zeros(rows * 4 * H, device=dev))
    kw = {}
    if planes:
        out["pl"] = torch.zeros(2 * rows * H, dtype=torch.bfloat16, device=dev)      # both planes: halves of one buffer
        kw = dict(h_bf16=out["pl"], ld_h_bf16=H, h_lo_bf16=out["pl"], h_lo_bf16_off=rows * H)
    ops.F32_PASSES = 3
    p = ops.lstm_seq_params(N, T, H, P, padl, d["xg"], 4 * H, d["whT"], None, d["lengths"], False, out["h"], H, out["c"],
                            out["g"], whT_hi=d["hi"], whT_lo=d["lo"], zoneout=zoneout, forget_bias=forget_bias, **kw)
    ops.F32_PASSES = 0
    assert ops.lstm_wide_supported(p, False)
    w = torch.zeros(ops.lstm_wide_work_floats(p), device=dev)
    for _ in range(launches):
        ops.lstm_wide("fwd", p, w)
    torch.cuda.synchronize()
    assert int(w[:1].view(torch.int32).item()) == 0
    return out


def _check(dev, d, **kw):
    from nspeech_amd import ops
    N, T, H = d["N"], d["T"], d["H"]
    P, rows = T + 1, N * (T + 1)
    ref = _fwd(dev, d, planes=False, **kw)
    got = _fwd(dev, d, planes=True, **kw)
    again = _fwd(dev, d, planes=True, launches=2, **kw)         # the second launch fills the sentinel again itself
    for k in ("h", "c", "g"):
        assert torch.equal(got[k], ref[k]), (k, (got[k] - ref[k]).abs().max().item())
        assert torch.equal(again[k], got[k]), k
    assert torch.isfinite(ref["h"]).all() and ref["h"].abs().max().item() > 0.0
    bits = got["pl"].view(torch.int16)
    assert torch.equal(again["pl"].view(torch.int16), bits)
    assert not (bits == -1).any()                                # 0xffff: no sentinel left, in pad rows neither
    hi = torch.zeros(rows * H, dtype=torch.bfloat16, device=dev)
    lo = torch.zeros(rows * H, dtype=torch.bfloat16, device=dev)
    ops.split_hi_lo(ref["h"], hi, lo, rows * H)
    torch.cuda.synchronize()
    assert torch.equal(bits[:rows * H], hi.view(torch.int16))
    assert torch.equal(bits[rows * H:], lo.view(torch.int16))
    # pad rows (slot 0) and the rows behind a row's length are zero in both planes
    pl = bits.view(2, N, P, H)
    assert not pl[:, :, 0].any()
    if d["lengths"] is not None:
        t = torch.arange(T, device=dev)[None, :] >= d["lengths"][:, None].long()        # [N, T]
        assert t.any() and not pl[:, :, 1:][:, t].any()


@pytest.mark.parametrize("T", [2, 3, 9])
@pytest.mark.parametrize("N", [1, 5, 17, 32])
def test_split_form_matches_the_fp32_exchange(dev, N, T):
    _check(dev, _data(dev, N, T, 256, seed=100 * N + T, masked=(N + T) % 2 == 1))


def test_split_form_with_cell_clip_and_forget_bias(dev):
    from nspeech_amd import ops
    old = ops.CELL_CLIP
    ops.CELL_CLIP = 0.5
    try:
        _check(dev, _data(dev, 17, 5, 256, seed=7, masked=True), forget_bias=0.25)
    finally:
        ops.CELL_CLIP = old


def test_split_form_with_zoneout(dev):
    from nspeech_amd import ops
    thr = ops.zoneout_threshold(0.25)
    _check(dev, _data(dev, 5, 9, 256, seed=8, masked=True), zoneout=(thr, thr, 11, 12))


def test_split_form_chunk_loop(dev):
    _check(dev, _data(dev, 17, 3, 1024, seed=9, masked=True))

