"""Lane ownership in the narrow forms of the role-split BiLSTM kernels.  At 8 and 4 rows per chain the padding columns of
the MFMA tile hold replicas of the live rows and the element-wise work of a slot is dealt over all 64 lanes (forward: a
lane keeps 2 or 1 of its column's 4 units; backward: a lane group keeps 2 or 1 of the chain's rows).  Who computes an
element changes, what is computed does not: every buffer must hold the SAME BITS as after the 16-row form
(NS_CLUSTER_ROWS=16) - torch.equal, no tolerance - with the status word 0 and the forced form reported after every launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("h", "c_fw", "c_bw", "g_fw", "g_bw", "dg_fw", "dg_bw")


def _form(work):
    return int(work[1:2].view(torch.int32).item()) or 16


def _status(work):
    return int(work[:1].view(torch.int32).item())


def _data(dev, N, T, H, lengths=None, xg_scale=1.0, forget_bias=1.0):
    g = torch.Generator().manual_seed(N * 977 + T * 31 + H)
    P, padl = T + 4, 2
    rows = N * P
    bf = torch.bfloat16
    data = dict(N=N, T=T, H=H, P=P, padl=padl, lengths=None, forget_bias=forget_bias)
    if lengths == "random":
        lengths = torch.randint(1, T + 1, (N,), generator=g, dtype=torch.int32)
        lengths[0] = T
    if lengths is not None:
        data["lengths"] = torch.as_tensor(lengths, dtype=torch.int32).to(dev)
    for d in ("fw", "bw"):
        data["xg_" + d] = (torch.randn(rows, 4 * H, generator=g) * xg_scale).to(dev)
        w = torch.randn(H, 4 * H, generator=g) / H ** 0.5
        data["wh_" + d] = w.to(bf).to(dev).contiguous()
        data["whT_" + d] = w.t().contiguous().to(bf).to(dev)
    data["dh"] = (torch.randn(rows, 2 * H, generator=g) * 0.1).to(dev)
    return data


def _run(dev, data, rows, cell_clip=0.0):
    """Forward and backward through the cluster kernels; the status word and the form are checked after EVERY launch.  The
    caller has set NS_CLUSTER_ROWS=rows.  The grid of a shape used here is a few workgroups, so the forced form always runs."""
    from nspeech_amd import ops
    N, T, H, P, padl = (data[k] for k in ("N", "T", "H", "P", "padl"))
    n = N * P
    bf = torch.bfloat16
    out = dict(h=torch.zeros(n * 2 * H, dtype=bf, device=dev))
    fp, bp = [], []
    saved = ops.CELL_CLIP
    ops.CELL_CLIP = cell_clip
    try:
        for di, d in enumerate(("fw", "bw")):
            out["c_" + d] = torch.zeros(n * H, device=dev)
            out["g_" + d] = torch.zeros(n * 4 * H, dtype=bf, device=dev)
            out["dg_" + d] = torch.zeros(n * 4 * H, dtype=bf, device=dev)
            work = torch.zeros(N * H + 64, device=dev)
            fp.append(ops.lstm_seq_params(N, T, H, P, padl, data["xg_" + d], 4 * H, data["whT_" + d], None, data["lengths"],
                                          d == "bw", out["h"], 2 * H, out["c_" + d], out["g_" + d], h_off=di * H,
                                          forget_bias=data["forget_bias"]))
            bp.append(ops.lstm_seq_params(N, T, H, P, padl, data["xg_" + d], 4 * H, None, data["wh_" + d], data["lengths"],
                                          d == "bw", out["h"], 2 * H, out["c_" + d], out["g_" + d], dh=data["dh"],
                                          ld_dh=2 * H, dgates=out["dg_" + d], work=work, dh_off=di * H, h_off=di * H,
                                          forget_bias=data["forget_bias"]))
    finally:
        ops.CELL_CLIP = saved
    assert ops.lstm_cluster_supported(fp[0]) and ops.lstm_cluster_supported(bp[0], bp[1], True)
    w = torch.zeros(ops.lstm_cluster_work_floats(fp[0]), device=dev)
    for direction, pair in (("fwd", fp), ("bwd", bp)):
        for _ in range(2):      # the second launch re-initialises the exchange state itself
            ops.lstm_cluster(direction, pair[0], pair[1], w)
            torch.cuda.synchronize()
            assert _status(w) == 0, (rows, direction, _status(w))
            assert _form(w) == rows, (rows, direction, _form(w))
    return out


def _against_16(dev, monkeypatch, data, cell_clip=0.0):
    monkeypatch.delenv("NS_CLUSTER_DBG", raising=False)
    monkeypatch.setenv("NS_CLUSTER_ROWS", "16")
    ref = _run(dev, data, 16, cell_clip)
    assert ref["h"].float().abs().max().item() > 0 and ref["dg_fw"].float().abs().max().item() > 0
    assert ref["dg_bw"].float().abs().max().item() > 0
    for rows in (8, 4):
        monkeypatch.setenv("NS_CLUSTER_ROWS", str(rows))
        got = _run(dev, data, rows, cell_clip)
        for k in KEYS:
            assert torch.equal(got[k], ref[k]), (rows, k, (got[k].float() - ref[k].float()).abs().max().item())
    return ref


# last chain with 3 / 2 / 3 / 1 / 2 live rows at 4 rows per chain (N % 4) and 1 live row at 8 (N 9); 2, 4, 1, 3 and 4
# workgroups per chain (H / 64; one = no exchange, the own block only); T 2 is the shortest sequence the kernels accept
@pytest.mark.parametrize("N,T,H", [(3, 4, 128), (6, 5, 256), (7, 6, 64), (9, 5, 192), (2, 2, 256)])
def test_ownership_edges(dev, monkeypatch, N, T, H):
    _against_16(dev, monkeypatch, _data(dev, N, T, H, lengths="random"))


def test_last_chain_with_one_live_row_of_four(dev, monkeypatch):
    """N 5: the second 4-row chain carries one live row (the edge list above has 2 and 3, and 1 only at 8 rows)."""
    _against_16(dev, monkeypatch, _data(dev, 5, 4, 128, lengths="random"))


def test_mask_follows_its_row(dev, monkeypatch):
    """Hand-set lengths: every row of a chain (8 rows: one chain; 4 rows: two) stops at a different slot in each direction."""
    _against_16(dev, monkeypatch, _data(dev, 8, 9, 256, lengths=[9, 1, 2, 8, 3, 7, 4, 5]))


def test_cell_clip_and_forget_bias_on_narrow_forms(dev, monkeypatch):
    """cell_clip 0.5 with pre-activations large enough that the clip acts (some |c| is exactly 0.5 in the 16-row result),
    and a forget bias other than the default."""
    data = _data(dev, 6, 7, 128, lengths="random", xg_scale=3.0, forget_bias=2.0)
    ref = _against_16(dev, monkeypatch, data, cell_clip=0.5)
    c = torch.cat([ref["c_fw"], ref["c_bw"]]).abs()
    assert c.max().item() == 0.5 and int((c == 0.5).sum().item()) > 16, (c.max().item(), int((c == 0.5).sum().item()))


def test_four_row_form_repeats_bit_for_bit(dev, monkeypatch):
    monkeypatch.delenv("NS_CLUSTER_DBG", raising=False)
    monkeypatch.setenv("NS_CLUSTER_ROWS", "4")
    data = _data(dev, 10, 12, 256, lengths="random")
    first = _run(dev, data, 4)
    for _ in range(2):
        again = _run(dev, data, 4)
        for k in KEYS:
            assert torch.equal(again[k], first[k]), k
