"""Rows per chain of the persistent BiLSTM kernels.  A chain of the role-split kernels carries 16, 8 or 4 batch rows
(NS_CLUSTER_ROWS forces a form; the default picks one from the grid it needs).  Batch rows are independent recurrences
and the backward sums keep their order (own block, then the peers' in workgroup order), so every form must write the
SAME BITS as the 16-row form into every output buffer - torch.equal, no tolerance."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(16, 9, 64, False), (20, 33, 256, True), (32, 61, 256, False), (5, 12, 128, True), (40, 21, 256, True),
          (48, 17, 192, False), (1, 7, 256, True), (1, 50, 256, False), (13, 10, 64, True), (32, 1000, 256, True)]


def _form(work):
    """The row count the last launch reported in the second int of its work buffer (0 = the 16-row form)."""
    return int(work[1:2].view(torch.int32).item()) or 16


def _status(work):
    return int(work[:1].view(torch.int32).item())


def _bf16_data(dev, N, T, H, masked):
    g = torch.Generator().manual_seed(N * 131 + T)
    P, padl = T + 4, 2
    rows = N * P
    bf = torch.bfloat16
    data = dict(N=N, T=T, H=H, P=P, padl=padl, lengths=None)
    if masked:
        lengths = torch.randint(1, T + 1, (N,), generator=g, dtype=torch.int32)
        lengths[0] = T
        data["lengths"] = lengths.to(dev)
    for d in ("fw", "bw"):
        data["xg_" + d] = torch.randn(rows, 4 * H, generator=g).to(dev)
        w = torch.randn(H, 4 * H, generator=g) / H ** 0.5
        data["wh_" + d] = w.to(bf).to(dev).contiguous()
        data["whT_" + d] = w.t().contiguous().to(bf).to(dev)
    data["dh"] = (torch.randn(rows, 2 * H, generator=g) * 0.1).to(dev)
    return data


def _run_bf16(dev, data):
    """Forward and backward of the bf16 BiLSTM through the cluster kernels; returns the outputs and the forms that ran."""
    from nspeech_amd import ops
    N, T, H, P, padl = (data[k] for k in ("N", "T", "H", "P", "padl"))
    rows = N * P
    bf = torch.bfloat16
    out = dict(h=torch.zeros(rows * 2 * H, dtype=bf, device=dev))
    fp, bp = [], []
    for di, d in enumerate(("fw", "bw")):
        out["c_" + d] = torch.zeros(rows * H, device=dev)
        out["g_" + d] = torch.zeros(rows * 4 * H, dtype=bf, device=dev)
        out["dg_" + d] = torch.zeros(rows * 4 * H, dtype=bf, device=dev)
        work = torch.zeros(N * H + 64, device=dev)
        fp.append(ops.lstm_seq_params(N, T, H, P, padl, data["xg_" + d], 4 * H, data["whT_" + d], None, data["lengths"],
                                      d == "bw", out["h"], 2 * H, out["c_" + d], out["g_" + d], h_off=di * H))
        bp.append(ops.lstm_seq_params(N, T, H, P, padl, data["xg_" + d], 4 * H, None, data["wh_" + d], data["lengths"],
                                      d == "bw", out["h"], 2 * H, out["c_" + d], out["g_" + d], dh=data["dh"],
                                      ld_dh=2 * H, dgates=out["dg_" + d], work=work, dh_off=di * H, h_off=di * H))
    assert ops.lstm_cluster_supported(fp[0]) and ops.lstm_cluster_supported(bp[0], bp[1], True)
    w = torch.zeros(ops.lstm_cluster_work_floats(fp[0]), device=dev)
    forms = []
    for direction, pair in (("fwd", fp), ("bwd", bp)):
        for _ in range(2):      # the second launch re-initialises the exchange state itself
            ops.lstm_cluster(direction, pair[0], pair[1], w)
        torch.cuda.synchronize()
        assert _status(w) == 0, (direction, _status(w))
        forms.append(_form(w))
    return out, forms


def _fp32_data(dev, N, T, H, masked):
    g = torch.Generator().manual_seed(N * 7 + T)
    P, padl = T + 4, 2
    rows = N * P
    bf = torch.bfloat16
    data = dict(N=N, T=T, H=H, P=P, padl=padl, lengths=None)
    if masked:
        lengths = torch.randint(1, T + 1, (N,), generator=g, dtype=torch.int32)
        lengths[0] = T
        data["lengths"] = lengths.to(dev)
    for d in ("fw", "bw"):
        data["xg_" + d] = torch.randn(rows, 4 * H, generator=g).to(dev)
        w = torch.randn(H, 4 * H, generator=g) / H ** 0.5
        data["whT_" + d] = w.t().contiguous().to(dev)
        data["hi_" + d] = data["whT_" + d].to(bf)
        data["lo_" + d] = (data["whT_" + d] - data["hi_" + d].float()).to(bf)
    return data


def _run_fp32(dev, data):
    """Forward of the fp32-state BiLSTM (lstm_cluster3_fwd_kernel): fp32 h, its bf16 copy, c, bf16 gates."""
    from nspeech_amd import ops
    N, T, H, P, padl = (data[k] for k in ("N", "T", "H", "P", "padl"))
    rows = N * P
    bf = torch.bfloat16
    out = dict(h=torch.zeros(rows * 2 * H, device=dev), hb=torch.zeros(rows * 2 * H, dtype=bf, device=dev))
    pair = []
    ops.F32_PASSES = 3
    for di, d in enumerate(("fw", "bw")):
        out["c_" + d] = torch.zeros(rows * H, device=dev)
        out["g_" + d] = torch.zeros(rows * 4 * H, dtype=bf, device=dev)
        pair.append(ops.lstm_seq_params(N, T, H, P, padl, data["xg_" + d], 4 * H, data["whT_" + d], None, data["lengths"],
                                        d == "bw", out["h"], 2 * H, out["c_" + d], out["g_" + d], h_off=di * H,
                                        whT_hi=data["hi_" + d], whT_lo=data["lo_" + d], h_bf16=out["hb"],
                                        h_bf16_off=di * H, ld_h_bf16=2 * H))
    ops.F32_PASSES = 0
    assert ops.lstm_cluster_supported(pair[0], pair[1], False)
    w = torch.zeros(ops.lstm_cluster_work_floats(pair[0]), device=dev)
    for _ in range(2):
        ops.lstm_cluster("fwd", pair[0], pair[1], w)
    torch.cuda.synchronize()
    assert _status(w) == 0, _status(w)
    return out, [_form(w)]


def _grid_fits(dev, N, rows, wgs_per_chain):
    return 2 * ((N + rows - 1) // rows) * wgs_per_chain <= torch.cuda.get_device_properties(dev).multi_processor_count


@pytest.mark.parametrize("N,T,H,masked", SHAPES)
def test_narrow_chains_bit_equal_bf16(dev, monkeypatch, N, T, H, masked):
    """lstm_cluster2_fwd_kernel and lstm_cluster2p_bwd_kernel at 8 and 4 rows per chain against 16: h, c, gates and
    dgates of both directions, bit for bit."""
    data = _bf16_data(dev, N, T, H, masked)
    monkeypatch.setenv("NS_CLUSTER_ROWS", "16")
    ref, forms = _run_bf16(dev, data)
    assert forms == [16, 16], forms
    assert ref["h"].float().abs().max().item() > 0 and ref["dg_fw"].float().abs().max().item() > 0
    for rows in (8, 4):
        monkeypatch.setenv("NS_CLUSTER_ROWS", str(rows))
        got, forms = _run_bf16(dev, data)
        if _grid_fits(dev, N, rows, H // 64):
            assert forms == [rows, rows], (rows, forms)
        for k in ("h", "c_fw", "c_bw", "g_fw", "g_bw", "dg_fw", "dg_bw"):
            assert torch.equal(got[k], ref[k]), (rows, k, (got[k].float() - ref[k].float()).abs().max().item())


@pytest.mark.parametrize("N,T,H,masked", SHAPES)
def test_narrow_chains_bit_equal_fp32_state(dev, monkeypatch, N, T, H, masked):
    """lstm_cluster3_fwd_kernel at 8 and 4 rows per chain against 16: fp32 h, its bf16 copy, c and the gates."""
    data = _fp32_data(dev, N, T, H, masked)
    monkeypatch.setenv("NS_CLUSTER_ROWS", "16")
    ref, forms = _run_fp32(dev, data)
    assert forms == [16], forms
    assert ref["h"].abs().max().item() > 0
    for rows in (8, 4):
        monkeypatch.setenv("NS_CLUSTER_ROWS", str(rows))
        got, forms = _run_fp32(dev, data)
        if _grid_fits(dev, N, rows, H // 32):
            assert forms == [rows], (rows, forms)
        for k in ("h", "hb", "c_fw", "c_bw", "g_fw", "g_bw"):
            assert torch.equal(got[k], ref[k]), (rows, k, (got[k].float() - ref[k].float()).abs().max().item())


def test_default_form_is_narrow_at_the_benchmark_width(dev, monkeypatch):
    """No override: batch 32 at H 256 runs a narrow form in all three kernels (the narrowest whose grid stays within
    half of the device)."""
    monkeypatch.delenv("NS_CLUSTER_ROWS", raising=False)
    monkeypatch.delenv("NS_CLUSTER_DBG", raising=False)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count

    def rule(N, wgs):
        for rows in (4, 8):
            if 2 * ((N + rows - 1) // rows) * wgs <= cus // 2:
                return rows
        return 16

    _, forms = _run_bf16(dev, _bf16_data(dev, 32, 25, 256, True))
    assert forms == [rule(32, 4), rule(32, 4)] and all(f < 16 for f in forms), forms
    _, forms = _run_fp32(dev, _fp32_data(dev, 32, 25, 256, True))
    assert forms == [rule(32, 8)] and forms[0] < 16, forms      # the fp32 form: H / 32 workgroups per chain
