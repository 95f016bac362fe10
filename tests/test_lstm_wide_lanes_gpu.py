"""The all-lane publish of the wide backward kernel (csrc/lstm_wide.hip, lstm_wide_bwd_ps_kernel<.., LANES = true>: every
lane group stores one granule per tile, groups 2 and 3 from replicas of rows 0 .. 7) against the publish by lane groups
0 and 1 (NS_WIDE_LANES=0, read per call) on the same operands: the gate gradients, their bf16 copy and the carry in
`work` bit for bit, and a second launch writes the same bits.  H = 256 with one row, a full 8-row group, a second group of
one row and the full batch; one case at H = 1024, where a product wave has a second group of four tiles."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _data(dev, N, T, H, seed, masked):
    from nspeech_amd import ops
    g = torch.Generator().manual_seed(seed)
    P, padl = T + 1, 1
    rows = N * P
    d = dict(N=N, T=T, H=H)
    d["lengths"] = torch.tensor([(1, T, max(1, T - 1))[i % 3] for i in range(N)], dtype=torch.int32).to(dev) if masked else None
    d["xg"] = torch.randn(rows, 4 * H, generator=g).to(dev)
    d["dh"] = (torch.randn(rows, H, generator=g) * 0.1).to(dev)
    d["wh"] = (torch.randn(H, 4 * H, generator=g) / H ** 0.5).to(dev)
    d["wh16"] = d["wh"].bfloat16()
    whT = d["wh"].t().contiguous()
    hi = whT.bfloat16()
    d["h"], d["c"], d["g"] = (torch.zeros(rows * H, device=dev), torch.zeros(rows * H, device=dev), torch.zeros(rows * 4 * H, device=dev))
    ops.F32_PASSES = 3                       # the forward pass once: the saved gates and cell states of every case
    ops.lstm_seq_call("fwd", ops.lstm_seq_params(N, T, H, P, padl, d["xg"], 4 * H, whT, None, d["lengths"], False, d["h"], H, d["c"],
                                                 d["g"], whT_hi=hi, whT_lo=(whT - hi.float()).bfloat16()))
    ops.F32_PASSES = 0
    torch.cuda.synchronize()
    return d


def _bwd(dev, d, launches=1):
    from nspeech_amd import ops
    N, T, H = d["N"], d["T"], d["H"]
    P, rows = T + 1, N * (T + 1)
    out = dict(dg=torch.zeros(rows * 4 * H, device=dev), dgb=torch.zeros(rows * 4 * H, dtype=torch.bfloat16, device=dev),
               work=torch.zeros(N * H + 64, device=dev))
    ops.F32_PASSES = 1
    p = ops.lstm_seq_params(N, T, H, P, 1, d["xg"], 4 * H, None, d["wh"], d["lengths"], False, d["h"], H, d["c"], d["g"],
                            dh=d["dh"], ld_dh=H, dgates=out["dg"], work=out["work"], wh_bf16=d["wh16"], dgates_bf16=out["dgb"])
    ops.F32_PASSES = 0
    assert ops.lstm_wide_supported(p, True)
    w = torch.zeros(ops.lstm_wide_work_floats(p), device=dev)
    for _ in range(launches):
        ops.lstm_wide("bwd", p, w)
    torch.cuda.synchronize()
    assert int(w[:1].view(torch.int32).item()) == 0
    return out


def _check(dev, monkeypatch, d):
    monkeypatch.delenv("NS_WIDE_LANES", raising=False)
    got = _bwd(dev, d)
    again = _bwd(dev, d, launches=2)
    monkeypatch.setenv("NS_WIDE_LANES", "0")
    ref = _bwd(dev, d)
    monkeypatch.delenv("NS_WIDE_LANES", raising=False)
    assert ref["dg"].abs().max().item() > 0.0 and torch.isfinite(ref["dg"]).all()
    for k in ("dg", "work"):
        assert torch.equal(got[k], ref[k]), (k, (got[k] - ref[k]).abs().max().item())
        assert torch.equal(again[k], got[k]), k
    assert torch.equal(got["dgb"].view(torch.int16), ref["dgb"].view(torch.int16))
    assert torch.equal(again["dgb"].view(torch.int16), got["dgb"].view(torch.int16))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("T", [2, 5])
@pytest.mark.parametrize("N", [1, 8, 9, 32])
def test_all_lane_publish_matches_the_two_group_publish(dev, monkeypatch, N, T, masked):
    _check(dev, monkeypatch, _data(dev, N, T, 256, seed=10 * N + T, masked=masked))


def test_all_lane_publish_second_tile_group(dev, monkeypatch):
    _check(dev, monkeypatch, _data(dev, 9, 3, 1024, seed=3, masked=True))
