"""The products of tests/test_gemm_plan_cpu.py: parameter blocks over made-up (aligned) addresses, and the case list whose
plans tests/golden/gemm_plan.json pins.  ns_gemm_plan is pure host code that follows no pointer, so no device is needed.

Run as a program it prints the plans of the cases named on the command line as JSON (the test starts one child per value
of NS_GEMM_HALF, which the library reads once per process):
    python tests/gemm_plan_cases.py [--lib PATH --func NAME] id ...
--lib / --func name another build of the library and its query function; the fixture was recorded that way."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nspeech_amd import _lib                                              # noqa: E402

BF16, F32 = _lib.NS_BF16, _lib.NS_F32
A0, B0, C0 = 0x10000000, 0x20000000, 0x30000000
X = [0x40000000 + i * 0x01000000 for i in range(12)]                     # further operands, 16 MB apart
ENV = ("NS_GEMM_DMA", "NS_GEMM_BK32", "NS_GEMM_NO256")                   # read per call
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plan.json")


def product(dtype=BF16, M=136, N=136, K=72, a_mode=0, b_mode=0, **kw):
    """A plain store into fp32 C with tight leading dimensions; kw sets or overrides fields of ns_gemm_params
    (bn_* those of the embedded ns_gemm_bn_params)."""
    p = _lib.struct("ns_gemm_params")
    p.dtype, p.M, p.N, p.K = dtype, M, N, K
    p.A, p.lda, p.a_mode = A0, (K if a_mode == 0 else M), a_mode
    p.B, p.ldb, p.b_mode = B0, (K if b_mode == 0 else N), b_mode
    p.C, p.ldc, p.c_dtype = C0, N, F32
    p.alpha = 1.0
    for k, v in kw.items():
        if k.startswith("bn_"):
            setattr(p.bn, k[3:], v)
        else:
            setattr(p, k, v)
    return p


def plan(p, lib=None, func="ns_gemm_plan"):
    """[kernel, loop, [grid], block, lds_bytes, stat_slots, return code, error text ("" on success)] of a block (or None)"""
    lib = lib or _lib.lib()
    info = _lib.struct("ns_gemm_plan_info")
    rc = getattr(lib, func)(ctypes.byref(p) if p is not None else None, ctypes.byref(info))
    s = lambda a: ctypes.cast(a, ctypes.c_char_p).value.decode() if a else None      # noqa: E731
    return [s(info.kernel), s(info.loop), [info.grid_x, info.grid_y, info.grid_z], info.block, info.lds_bytes,
            info.stat_slots, rc, lib.ns_last_error().decode() if rc else ""]


def plan_case(case, lib=None, func="ns_gemm_plan"):
    """plan() of a case of CASES under the case's per-call environment switches"""
    saved = {k: os.environ.pop(k, None) for k in ENV}
    os.environ.update(case["env"])
    try:
        return plan(product(**case["p"]) if case["p"] is not None else None, lib, func)
    finally:
        for k in ENV:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


CASES = []


def _case(cid, env=None, half=None, **p):
    assert all(c["id"] != cid for c in CASES), cid
    CASES.append(dict(id=cid, env=dict(env or {}), half=half, p=p))


STATS = dict(col_sum=X[0], col_sumsq=X[1], stat_part=X[2])
KSLOW = dict(a_mode=1, b_mode=1, accumulate=2)            # a weight gradient: both operands k-slow, atomic accumulation
X256 = dict(M=1024, N=6144, K=128)                        # 4 x 24 = 96 tiles of 256 x 256
LO = dict(A_lo=X[3], B_lo=X[4])


def _cases():
    # ---- the skinny kernel: M <= 32, N below / from 32 * 128
    for M in (32, 33):
        _case("skinny_M%d" % M, M=M, N=72, K=104)
    for N in (4095, 4096):
        _case("skinny_N%d" % N, M=5, N=N, K=64)
    _case("skinny_with_stats_goes_on", M=17, N=72, K=104, **STATS)
    # ---- the 256-tile kernel
    for M in (1023, 1024):
        _case("x256_M%d" % M, **dict(X256, M=M))
    _case("x256_96_tiles", M=1536, N=4096, K=128)
    _case("x256_95_tiles", M=1280, N=4864, K=128)
    for K in (64, 128, 160, 192):
        _case("x256_K%d" % K, **dict(X256, K=K))
    _case("x256_N_not_128", **dict(X256, N=6208))
    _case("x256_A_below_4e9_bytes", **dict(X256, lda=1953120))
    _case("x256_A_at_4e9_bytes", **dict(X256, lda=1953128))
    _case("x256_B_at_4e9_bytes", **dict(X256, ldb=325528))                # 6144 * 325528 * 2 >= 4e9
    _case("x256_B_below_4e9_bytes", **dict(X256, ldb=325520))
    _case("x256_split_k", **dict(X256, split_k=2, accumulate=2))
    _case("x256_batch_2", **dict(X256, batch=2, batch_stride_a=1024 * 128, batch_stride_b=0, batch_stride_c=1024 * 6144))
    _case("x256_b_seg_64", **dict(X256, b_seg_len=64, b_seg_stride=8 * 128))
    _case("x256_stats", **dict(X256, **STATS))
    for passes in (2, 3):
        _case("x256_presplit_passes%d" % passes, **dict(X256, f32_passes=passes, **LO))
    _case("x256_presplit_lo_unaligned", **dict(X256, f32_passes=3, A_lo=X[3] + 8, B_lo=X[4]))
    _case("presplit_refused_M512", **dict(X256, M=512, f32_passes=3, **LO))
    _case("presplit_refused_one_low_part", **dict(X256, f32_passes=3, A_lo=X[3]))
    _case("presplit_refused_skinny", M=32, N=128, K=64, **LO)
    _case("presplit_refused_fp32", dtype=F32, f32_passes=3, **dict(X256, **LO))
    # ---- half-height tiles: tiles * batch <= 256 and M > 64, with the vector epilogue and k-contiguous A
    _case("half_256_tiles", M=2048, N=2048, K=64)
    _case("half_257_tiles", M=32896, N=128, K=64)
    for b in (256, 257):
        _case("half_batch_%d" % b, M=128, N=128, K=64, batch=b, batch_stride_a=128 * 64, batch_stride_b=128 * 64, batch_stride_c=128 * 128)
    for M in (64, 65):
        for b_mode in (0, 1):
            _case("half_M%d_b%d" % (M, b_mode), M=M, N=136, K=72, b_mode=b_mode)
    _case("half_not_with_k_slow_A", M=136, N=136, K=72, a_mode=1)
    _case("half_batch_stride_c_not_4", M=128, N=128, K=64, batch=2, batch_stride_a=128 * 64, batch_stride_b=0, batch_stride_c=128 * 128 + 2)
    for v, M in (("0", 65), ("1", 64), ("300", 65)):
        _case("half_env%s_M%d" % (v, M), half=v, M=M, N=136, K=72)
    _case("half_env300_300_tiles", half="300", M=128 * 300, N=128, K=64)
    _case("half_env300_301_tiles", half="300", M=128 * 301, N=128, K=64)
    _case("half_env1_fp32", half="1", dtype=F32, f32_passes=3, M=64, N=136, K=100)
    _case("half_env0_fp32", half="0", dtype=F32, f32_passes=3, M=130, N=136, K=100)
    # ---- BK = 32: tiles * split_k * batch >= 600, both operands k-slow
    for s in (599, 600):
        _case("bk32_%d_workgroups" % s, M=128, N=128, K=64 * 600, split_k=s, **KSLOW)
    _case("bk32_25_tiles_24_slices", M=640, N=640, K=808, split_k=24, **KSLOW)
    _case("bk32_store_vec", M=3200, N=3072, K=72, a_mode=1, b_mode=1)              # 25 x 24 tiles, vector epilogue
    _case("bk32_batch", M=128, N=128, K=64, batch=600, batch_stride_a=128 * 64, batch_stride_b=128 * 64, batch_stride_c=128 * 128, **KSLOW)
    _case("bk32_not_k_contiguous_B", M=640, N=640, K=808, split_k=24, a_mode=1, b_mode=0, accumulate=2)
    _case("bk32_b_seg_64", M=640, N=640, K=64 * 24, split_k=24, b_seg_len=64, b_seg_stride=64 * 640, **KSLOW)
    _case("b_seg_not_32", M=640, N=640, K=48 * 24, split_k=24, b_seg_len=48, b_seg_stride=48 * 640, **KSLOW)
    _case("bk32_env0", env={"NS_GEMM_BK32": "0"}, M=640, N=640, K=808, split_k=24, **KSLOW)
    _case("bk32_env1", env={"NS_GEMM_BK32": "1"}, M=136, N=136, K=100, **KSLOW)
    _case("bk32_env1_staged", env={"NS_GEMM_BK32": "1", "NS_GEMM_DMA": "0"}, M=136, N=136, K=100, **KSLOW)
    _case("bk32_env1_b_seg_64", env={"NS_GEMM_BK32": "1"}, M=136, N=136, K=128, b_seg_len=64, b_seg_stride=64 * 136, **KSLOW)
    _case("bk32_env1_not_k_slow", env={"NS_GEMM_BK32": "1"}, M=136, N=136, K=72, a_mode=0, b_mode=1, accumulate=2)
    # ---- the direct-to-LDS loop: both operands k-slow, 31-bit byte offsets
    _case("dma_plain", M=136, N=136, K=100, **KSLOW)
    _case("dma_store_vec", M=136, N=136, K=100, a_mode=1, b_mode=1)
    _case("dma_env0", env={"NS_GEMM_DMA": "0"}, M=136, N=136, K=100, **KSLOW)
    _case("dma_env0_bk32", env={"NS_GEMM_DMA": "0"}, M=640, N=640, K=808, split_k=24, **KSLOW)
    _case("dma_A_below_2_31", M=136, N=136, K=1025, lda=1048568, **KSLOW)
    _case("dma_A_over_2_31", M=136, N=136, K=1025, lda=1048576, **KSLOW)
    _case("dma_B_over_2_31", M=136, N=136, K=1025, ldb=1048576, **KSLOW)
    _case("dma_b_seg", M=136, N=136, K=128, b_seg_len=64, b_seg_stride=64 * 136, **KSLOW)
    _case("dma_b_seg_negative_stride", M=136, N=136, K=128, b_seg_len=64, b_seg_stride=-64 * 136, **KSLOW)
    _case("dma_b_seg_over_2_31", M=136, N=136, K=128, b_seg_len=64, b_seg_stride=1 << 30, **KSLOW)
    _case("dma_negative_lda", M=136, N=136, K=100, lda=-136, **KSLOW)
    for a, b in ((0, 0), (0, 1), (1, 0)):
        _case("dma_not_modes_%d%d" % (a, b), M=136, N=136, K=72, a_mode=a, b_mode=b, accumulate=2)
    _case("modes_2_0", M=136, N=136, K=72, a_mode=2, b_mode=0, accumulate=2)       # the ladder's last rung takes what is left
    _case("modes_0_2", M=136, N=136, K=72, a_mode=0, b_mode=2, accumulate=2)
    # ---- fp32 operands
    for passes in (0, 1, 3):
        _case("f32_passes%d" % passes, dtype=F32, f32_passes=passes, M=136, N=136, K=100, **KSLOW)
        _case("f32_passes%d_store" % passes, dtype=F32, f32_passes=passes, M=136, N=136, K=100, a_mode=1, b_mode=0)
        _case("f32_passes%d_half" % passes, dtype=F32, f32_passes=passes, M=130, N=136, K=100, b_mode=1)
    for N in (1024, 1025, 1040):
        for passes in (1, 3):
            _case("skinny_f32_N%d_passes%d" % (N, passes), dtype=F32, f32_passes=passes, M=20, N=N, K=104)
    _case("skinny_f32_passes0", dtype=F32, f32_passes=0, M=20, N=72, K=104)
    for M in (32, 33):
        _case("skinny_f32_M%d" % M, dtype=F32, f32_passes=3, M=M, N=72, K=104)
    _case("skinny_f32_K_not_8", dtype=F32, f32_passes=3, M=20, N=72, K=100)
    _case("f32_K_not_4", dtype=F32, f32_passes=3, M=136, N=136, K=98)
    _case("f32_lda_not_4", dtype=F32, f32_passes=3, M=136, N=136, K=100, lda=102)
    _case("f32_b_seg_not_32", dtype=F32, f32_passes=3, M=136, N=136, K=96, b_seg_len=16, b_seg_stride=16 * 136, b_mode=1)
    _case("f32_split_k", dtype=F32, f32_passes=1, M=80, N=256, K=388, split_k=3, **KSLOW)
    # ---- one misalignment at a time: the generic kernel
    _case("generic_lda_not_8", lda=76)
    _case("generic_ldb_not_8", ldb=76)
    _case("generic_odd_A", A=A0 + 2)
    _case("generic_B_not_16", B=B0 + 8)
    _case("generic_K_not_8", K=67, lda=72, ldb=72)
    _case("generic_M_not_8_k_slow", M=130, a_mode=1, lda=136)
    _case("generic_batch_stride_a_not_8", batch=2, batch_stride_a=136 * 72 + 4, batch_stride_b=0, batch_stride_c=136 * 136)
    _case("generic_batch_stride_b_not_8", batch=2, batch_stride_a=0, batch_stride_b=136 * 72 + 4, batch_stride_c=136 * 136)
    _case("generic_b_seg_stride_not_8", K=128, b_seg_len=64, b_seg_stride=64 * 136 + 4, b_mode=1)
    _case("generic_split_k_batch", M=70, N=67, K=45, split_k=2, accumulate=2, batch=3, batch_stride_a=70 * 45, batch_stride_b=67 * 45,
          batch_stride_c=70 * 67)
    _case("generic_f32_stats", dtype=F32, M=70, N=67, K=45, **STATS)
    # ---- the vector epilogue: each operand misaligned in turn (M = 136 with k-slow A: no half tiles)
    V = dict(M=136, N=136, K=72, a_mode=1)
    ZST = dict(stat_z=X[5], ld_stat_z=136, stat_mean=X[6], stat_istd=X[7], **STATS)
    _case("vec_all_aligned", addend=X[8], ld_add=136, gate=X[9], ld_gate=136, bias=X[10], **dict(V, **ZST))
    _case("vec_C_not_16", **dict(V, C=C0 + 8))
    _case("vec_C_bf16_8_is_enough", **dict(V, C=C0 + 8, c_dtype=BF16))
    _case("vec_C_bf16_not_8", **dict(V, C=C0 + 4, c_dtype=BF16))
    _case("vec_ldc_not_4", **dict(V, ldc=138))
    _case("vec_N_not_4", **dict(V, N=134, ldc=136))
    _case("vec_addend_not_16", **dict(V, addend=X[8] + 8, ld_add=136))
    _case("vec_addend_bf16_8_is_enough", **dict(V, addend=X[8] + 8, ld_add=136, addend_dtype=BF16))
    _case("vec_ld_add_not_4", **dict(V, addend=X[8], ld_add=138))
    _case("vec_gate_not_8", **dict(V, gate=X[9] + 4, ld_gate=136))
    _case("vec_gate_f32_not_16", dtype=F32, f32_passes=3, **dict(V, K=100, gate=X[9] + 8, ld_gate=136))
    _case("vec_stat_z_not_16", **dict(V, **dict(ZST, stat_z=X[5] + 8)))
    _case("vec_stat_mean_not_16", **dict(V, **dict(ZST, stat_mean=X[6] + 4)))
    _case("vec_stat_part_not_16", **dict(V, **dict(STATS, stat_part=X[2] + 4)))
    _case("vec_bias_not_16", **dict(V, bias=X[10] + 4))
    _case("vec_accumulate_1", **dict(V, accumulate=1))
    _case("vec_accumulate_2", **dict(V, accumulate=2))
    _case("x256_C_not_16", **dict(X256, C=C0 + 8))
    _case("x256_gate_not_8", **dict(X256, gate=X[9] + 4, ld_gate=6144))
    _case("x256_accumulate_2", **dict(X256, accumulate=2))                      # the 256-tile kernel does not look at it
    _case("x256_env_no256", env={"NS_GEMM_NO256": "1"}, **X256)
    # ---- batch and split-K
    _case("batch_3", M=130, N=136, K=72, batch=3, batch_stride_a=130 * 72, batch_stride_b=136 * 72, batch_stride_c=130 * 136)
    _case("split_k_atomic", M=136, N=264, K=520, split_k=3, **KSLOW)
    _case("split_k_fixed_order", M=136, N=264, K=520, split_k=3, splitk_work=X[8], splitk_count=X[9], **KSLOW)
    _case("split_k_0_reads_as_1", M=136, N=264, K=520, split_k=0, **KSLOW)
    _case("batch_0_reads_as_1", M=136, N=264, K=520, batch=0, **KSLOW)
    # ---- every argument check, in the order ns_gemm makes them
    _case("err_null_params")
    CASES[-1]["p"] = None
    _case("err_col_sumsq_alone", col_sumsq=X[1])
    _case("err_col_sum_without_scratch", col_sum=X[0])
    _case("err_stat_z_with_atomic", accumulate=2, **ZST)
    _case("err_bn_without_sums", bn_mean_out=X[8], bn_istd_out=X[9], bn_training=1, bn_count=10.0)
    _case("err_bn_without_count", bn_mean_out=X[8], bn_istd_out=X[9], bn_training=1, **STATS)
    _case("err_bn_empty", N=0, bn_mean_out=X[8], bn_istd_out=X[9], bn_training=1, bn_count=10.0, **STATS)
    _case("bn_accepted", bn_mean_out=X[8], bn_istd_out=X[9], bn_training=1, bn_count=10.0, **STATS)
    _case("err_negative_K", K=-1)
    _case("empty_M", M=0)
    _case("empty_N_with_null_operands", N=0, A=None, B=None, C=None)
    _case("K_0", K=0)
    _case("err_null_A", A=None)
    _case("err_null_C", C=None)
    _case("err_dtype", dtype=2)
    _case("err_c_dtype", c_dtype=7)
    _case("err_work_without_counters", split_k=2, accumulate=2, splitk_work=X[8])
    _case("err_fixed_order_with_batch", split_k=2, accumulate=2, splitk_work=X[8], splitk_count=X[9], batch=2)
    _case("err_scratch_beyond_2GB", M=4096, N=4096, K=4096, split_k=32, splitk_work=X[8], splitk_count=X[9], **KSLOW)
    _case("err_accumulate_3", accumulate=3)
    _case("err_accumulate_bf16_C", accumulate=1, c_dtype=BF16)
    _case("err_split_k_store", split_k=2)
    _case("err_split_k_activation", split_k=2, accumulate=2, act=1)
    _case("err_K_not_b_seg_multiple", K=72, b_seg_len=64)
    _case("err_b_seg_negative", K=72, b_seg_len=-8)
    _case("err_f32_passes_2", dtype=F32, f32_passes=2)
    _case("bf16_ignores_f32_passes", f32_passes=2)
    _case("alpha_0_reads_as_1", alpha=0.0)
    _case("err_batch_with_bias", batch=2, bias=X[10])
    _case("err_batch_65536", batch=65536)


_cases()


if __name__ == "__main__":
    args = sys.argv[1:]
    lib, func = None, "ns_gemm_plan"
    while args and args[0].startswith("--"):
        if args[0] == "--lib":
            lib = ctypes.CDLL(args[1])
            lib.ns_last_error.restype = ctypes.c_char_p
        else:
            assert args[0] == "--func", args[0]
            func = args[1]
        args = args[2:]
    by_id = {c["id"]: c for c in CASES}
    json.dump({i: plan_case(by_id[i], lib, func) for i in args}, sys.stdout)
