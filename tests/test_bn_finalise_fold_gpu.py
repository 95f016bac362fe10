"""BatchNorm's small finalisers off the main stream's launch queue.

Forward: ns_gemm with the `bn` block finishes mean / 1/std and the moving statistics in the statistics' second stage
(gemm_stats_finalize_kernel), and ns_bn_fwd with stats_final launches the apply pass alone - against today's two calls,
bit for bit.  Backward: ns_bn_bwd with no_finalize + ns_bn_bwd_finalize against one ns_bn_bwd, bit for bit, the
finaliser also on a second stream behind an event."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ACT_RELU = 1
# rows x C: 2200 rows are more than 32 statistics slots of 64 rows (the strided slot loop of the second stage runs), 36
# columns leave a ragged last block of 32; 130 rows are fewer slots than slot lanes
SHAPES = [(2200, 36), (2200, 128), (130, 512)]
PERIOD, LO, HI = 110, 3, 104           # 2200 = 20 x 110; 130 = 110 + a cut-off second period


def _product(dev, rows, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    K = 64
    A = (torch.randn(rows, K, generator=g) * 0.3).to(dtype).to(dev)
    B = (torch.randn(C, K, generator=g) * 0.3).to(dtype).to(dev)
    bias = (torch.randn(C, generator=g) * 0.1).to(dev)
    gamma = (1.0 + 0.1 * torch.randn(C, generator=g)).to(dev)
    beta = (0.1 * torch.randn(C, generator=g)).to(dev)
    mm0 = (0.1 * torch.randn(C, generator=g)).to(dev)
    mv0 = (1.0 + 0.2 * torch.rand(C, generator=g)).to(dev)
    m = torch.arange(rows)
    count = int((((m % PERIOD) >= LO) & ((m % PERIOD) < HI)).sum())
    return A, B, K, bias, gamma, beta, mm0, mv0, count


@pytest.mark.parametrize("rows,C", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("training", [True, False])
def test_forward_finaliser_folded_into_the_statistics_stage(dev, rows, C, dtype, training):
    from nspeech_amd import ops
    A, B, K, bias, gamma, beta, mm0, mv0, count = _product(dev, rows, C, dtype, rows + C)
    res = []
    for fold in (False, True):
        z = torch.full((rows, C), float("nan"), dtype=dtype, device=dev)
        y = torch.full((rows, C), float("nan"), dtype=dtype, device=dev)
        st = torch.full((4 * C,), float("nan"), device=dev)
        mm, mv = mm0.clone(), mv0.clone()
        bn = dict(count=count, training=training, moving_mean=mm, moving_var=mv, mean_out=st[2 * C:], istd_out=st[3 * C:])
        ops.gemm(A, B, z, rows, C, K, K, K, C, a_mode=0, b_mode=0, bias=bias, act=ACT_RELU, row_mask=(PERIOD, LO, HI, 0),
                 col_sum=st, col_sumsq=st[C:], f32_passes=0, bn=bn if fold else None)
        ops.bn_fwd(z, y, rows, C, st, st[C:], count, gamma, beta, mm, mv, st[2 * C:], st[3 * C:], training,
                   row_mask=(PERIOD, LO, HI), stats_final=fold)
        torch.cuda.synchronize()
        res.append(dict(col_sum=st[:C].clone(), col_sumsq=st[C:2 * C].clone(), mean=st[2 * C:3 * C].clone(),
                        istd=st[3 * C:].clone(), moving_mean=mm, moving_var=mv, y=y))
    for k in res[0]:
        assert not bool(torch.isnan(res[0][k].float()).any()), k
        assert torch.equal(res[0][k], res[1][k]), k
    moved = not torch.equal(res[1]["moving_mean"], mm0)
    assert moved == training                     # the moving statistics move in training only
    if not training:
        assert torch.equal(res[1]["mean"], mm0)


def test_fold_argument_errors(dev):
    """The block needs both sums and takes no stat_z: an error, not a silent skip."""
    from nspeech_amd import _lib, ops
    A, B, K, bias, gamma, beta, mm0, mv0, count = _product(dev, 130, 64, torch.float32, 1)
    z = torch.zeros(130, 64, device=dev)
    st = torch.zeros(4 * 64, device=dev)
    bn = dict(count=count, training=True, moving_mean=mm0, moving_var=mv0, mean_out=st[128:], istd_out=st[192:])
    with pytest.raises(_lib.NSError):
        ops.gemm(A, B, z, 130, 64, K, K, K, 64, bn=bn)
    with pytest.raises(_lib.NSError):
        ops.gemm(A, B, z, 130, 64, K, K, K, 64, col_sum=st, bn=bn)


@pytest.mark.parametrize("rows,C", SHAPES)
@pytest.mark.parametrize("dtype,side", [(torch.float32, False), (torch.bfloat16, False), (torch.float32, True)])
def test_backward_finaliser_as_its_own_entry_point(dev, rows, C, dtype, side):
    """side: the finaliser on a second stream behind an event, as the deferred weight gradients run it."""
    from nspeech_amd import ops
    g = torch.Generator().manual_seed(rows * 3 + C)
    z = torch.relu(torch.randn(rows, C, generator=g)).to(dtype).to(dev)
    dy = (torch.randn(rows, C, generator=g) * 0.3).to(dev)
    mean = (torch.randn(C, generator=g) * 0.1).to(dev)
    istd = (1.0 + 0.2 * torch.rand(C, generator=g)).to(dev)
    gamma = (1.0 + 0.1 * torch.randn(C, generator=g)).to(dev)
    m = torch.arange(rows, device=dev)
    valid = (((m % PERIOD) >= LO) & ((m % PERIOD) < HI)).float()[:, None]
    xh = (z.float() - mean) * istd
    sums = torch.cat([(dy * valid).sum(0), (dy * xh * valid).sum(0)]).contiguous()
    count = float(valid.sum())
    start = torch.randn(3 * C, generator=g).to(dev)          # the outputs accumulate: start from something
    res = []
    for split in (False, True):
        dpre = torch.full((rows, C), float("nan"), dtype=dtype, device=dev)
        gr = start.clone()
        work = torch.zeros(200 * max(1024, C), device=dev)
        blk = ops.bn_bwd(dy, z, dpre, rows, C, mean, istd, gamma, gr, gr, gr, work, count, ACT_RELU,
                         row_mask=(PERIOD, LO, HI), dgamma_off=0, dbeta_off=C, dbias_off=2 * C,
                         sums=(sums[:C], sums[C:]), no_finalize=split)
        if split:
            assert blk is not None
            if side:
                assert torch.equal(gr, start)                # nothing added yet
                ev = torch.cuda.Event()
                ev.record()
                s2 = torch.cuda.Stream()
                s2.wait_event(ev)
                with torch.cuda.stream(s2):
                    ops.bn_bwd_finalize(blk)
            else:
                ops.bn_bwd_finalize(blk)
        else:
            assert blk is None
        torch.cuda.synchronize()
        res.append((dpre, gr))
    assert torch.equal(res[0][0], res[1][0]), "dpre"
    for name, lo in (("dgamma", 0), ("dbeta", C), ("dbias", 2 * C)):
        assert torch.equal(res[0][1][lo:lo + C], res[1][1][lo:lo + C]), name
    assert not torch.equal(res[0][1], start)


def test_no_finalize_needs_the_fused_sums(dev):
    from nspeech_amd import _lib, ops
    rows, C = 130, 64
    z = torch.zeros(rows, C, device=dev)
    v = torch.ones(C, device=dev)
    gr = torch.zeros(3 * C, device=dev)
    with pytest.raises(_lib.NSError):
        ops.bn_bwd(z, z, torch.zeros_like(z), rows, C, v, v, v, gr, gr, gr, torch.zeros(200 * 1024, device=dev), 100.0,
                   ACT_RELU, dgamma_off=0, dbeta_off=C, dbias_off=2 * C, sums=None, no_finalize=True)
