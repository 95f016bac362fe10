"""ns_gemm_group's host side (include/nspeech_hip.h): the item table's layout, the size of the kernel's argument block,
and ns_gemm_group_plan - classification, workgroup counts, order, the cut into launches and every refusal.  The plan is
pure host code that never dereferences an operand, so made-up (aligned) addresses serve and no device is needed."""
import ctypes
import re

import pytest

from nspeech_amd import _lib

BF16, F32 = _lib.NS_BF16, _lib.NS_F32
BAD_ARG = -1
MB = 1 << 20


def _max_items():
    src = open(_lib.HEADER_PATH).read()
    return int(re.search(r"NS_GEMM_GROUP_MAX\s*=\s*(\d+)", src).group(1))


def _product(slot, M, N, K, dtype=BF16, split_k=1, det=False, **kw):
    """A weight-gradient product as the models issue it: both operands k-slow, atomic fp32 accumulation.  slot picks
    disjoint made-up addresses."""
    p = _lib.struct("ns_gemm_params")
    base = 0x10000000 + slot * 64 * MB
    p.dtype, p.M, p.N, p.K = dtype, M, N, K
    p.A, p.lda, p.a_mode = base, M, 1
    p.B, p.ldb, p.b_mode = base + 16 * MB, N, 1
    p.C, p.ldc, p.c_dtype = base + 32 * MB, N, F32
    p.accumulate, p.split_k, p.alpha, p.f32_passes = 2, split_k, 1.0, 1
    if det:
        p.splitk_work, p.splitk_count = base + 40 * MB, base + 60 * MB
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _sum(slot, rows, C, dtype=BF16, ld=None, work=True, **kw):
    p = _lib.struct("ns_colsum_params")
    base = 0x10000000 + slot * 64 * MB
    p.x, p.dtype, p.ld, p.rows, p.C = base, dtype, ld or (C + 3) // 4 * 4, rows, C
    p.out = base + 32 * MB
    if work:
        p.work = base + 40 * MB if work is True else work
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _plan(products, sums):
    lib = _lib.lib()
    n = len(products) + len(sums)
    E = _lib.STRUCTS["ns_gemm_group_plan_entry"]
    entries = (E * max(n, 1))()
    for e in entries:
        e.index = -77                                   # what a refused call must leave behind
    ap = (_lib.STRUCTS["ns_gemm_params"] * len(products))(*products) if products else None
    asum = (_lib.STRUCTS["ns_colsum_params"] * len(sums))(*sums) if sums else None
    nl = ctypes.c_int(-5)
    rc = lib.ns_gemm_group_plan(ap, len(products), asum, len(sums), entries, ctypes.byref(nl))
    return rc, list(entries)[:n], nl.value


def test_item_layout_follows_the_header():
    it = _lib.STRUCTS["ns_gemm_group_item"]
    names = [f[0] for f in it._fields_]
    assert names == ["A", "B", "C", "work", "count", "lda", "ldb", "ldc", "b_seg_stride", "M", "N", "K", "b_seg_len",
                     "split_k", "dtype", "kind", "wg0", "nwg", "reserved"]
    assert ctypes.sizeof(it) == 112
    assert (it.A.offset, it.work.offset, it.lda.offset, it.M.offset, it.split_k.offset, it.wg0.offset, it.nwg.offset) == \
        (0, 24, 40, 72, 88, 100, 104)
    e = _lib.STRUCTS["ns_gemm_group_plan_entry"]
    assert [f[0] for f in e._fields_] == ["index", "kind", "launch", "wg0", "nwg", "k_extent"] and ctypes.sizeof(e) == 24
    for f in ("ns_gemm_group", "ns_gemm_group_plan", "ns_gemm_group_arg_bytes"):
        assert f in _lib.FUNCS and hasattr(_lib.lib(), f)
    assert _lib.lib().ns_version() >= 102


def test_argument_block_fits_4096_bytes():
    lib = _lib.lib()
    lib.ns_gemm_group_arg_bytes.restype = ctypes.c_size_t
    n = _max_items()
    item = ctypes.sizeof(_lib.STRUCTS["ns_gemm_group_item"])
    # the prefix table (one int per item) and the items, nothing else
    assert lib.ns_gemm_group_arg_bytes() == n * (4 + item) <= 4096
    assert n == 32 and 4096 // (4 + item) == 35           # what 4096 bytes allow; 32 leaves room


def _tiles(M, N):
    return ((M + 127) // 128) * ((N + 127) // 128)


def test_plan_of_a_mixed_list():
    products = [
        _product(0, 136, 264, 520, split_k=3, det=True),            # bf16, K per workgroup 3 tiles of 64 = 192
        _product(1, 80, 256, 388, dtype=F32, split_k=3, det=True),  # fp32, 13 tiles of 32 over 3 slices: 5 x 32 = 160
        _product(2, 1536, 4096, 6432, split_k=1),                   # whole K per workgroup
        _product(3, 256, 0, 100),                                   # empty output: accepted, no workgroups
        _product(4, 80, 136, 300, split_k=2, lda=16),               # overlapping im2col view (lda < M)
    ]
    sums = [_sum(5, 520, 264), _sum(6, 300, 100, dtype=F32, ld=104, work=False)]
    rc, entries, launches = _plan(products, sums)
    assert rc == 0, _lib.lib().ns_last_error()
    assert launches == 1
    by_index = {e.index: e for e in entries}
    assert sorted(by_index) == list(range(7))
    assert [by_index[i].kind for i in range(7)] == [0, 1, 0, 0, 0, 2, 2]
    want = {0: _tiles(136, 264) * 3, 1: _tiles(80, 256) * 3, 2: _tiles(1536, 4096), 3: 0, 4: _tiles(80, 136) * 2,
            5: ((520 + 127) // 128) * ((264 // 4 + 15) // 16),       # row blocks of <= 128 rows x blocks of 16 column quads
            6: ((300 + 127) // 128) * ((100 // 4 + 15) // 16)}
    assert {i: by_index[i].nwg for i in range(7)} == want
    assert {i: by_index[i].k_extent for i in range(7)} == {0: 192, 1: 160, 2: 6432, 3: 0, 4: 192, 5: 104, 6: 100}
    # order: descending K extent per workgroup, ties in caller order
    assert [e.index for e in entries] == [2, 0, 4, 1, 5, 6, 3]
    # every item starts at a multiple of 8, right behind the one before
    wg = 0
    for e in entries:
        assert e.wg0 % 8 == 0 and e.wg0 == wg and e.launch == 0
        wg = (wg + e.nwg + 7) // 8 * 8


def test_a_long_list_is_split():
    n = _max_items()
    products = [_product(i, 136, 136, 64 * (n + 8 - i)) for i in range(n + 5)]
    rc, entries, launches = _plan(products, [])
    assert rc == 0 and launches == 2
    assert [e.index for e in entries] == list(range(n + 5))
    assert [e.launch for e in entries] == [0] * n + [1] * 5
    assert entries[n].wg0 == 0 and entries[n - 1].wg0 == 8 * (n - 1)       # the second launch counts from 0 again


REFUSED = {
    "a_mode_0": lambda: ([_product(0, 136, 136, 520, a_mode=0, lda=520)], []),
    "b_mode_0": lambda: ([_product(0, 136, 136, 520, b_mode=0, ldb=520)], []),
    "skinny": lambda: ([_product(0, 16, 136, 520, a_mode=0, lda=520, b_mode=0, ldb=520)], []),
    "generic_M_not_8": lambda: ([_product(0, 130, 136, 520, lda=136)], []),
    "generic_unaligned_A": lambda: ([_product(0, 136, 136, 520, A=0x10000002)], []),
    "bk32": lambda: ([_product(0, 640, 640, 64 * 48, split_k=24)], []),
    "f32_exact": lambda: ([_product(0, 136, 136, 520, dtype=F32, f32_passes=0)], []),
    "f32_three_passes": lambda: ([_product(0, 136, 136, 520, dtype=F32, f32_passes=3)], []),
    "store": lambda: ([_product(0, 136, 136, 520, accumulate=0)], []),                      # vector epilogue / half tiles
    "store_256_tile": lambda: ([_product(0, 4096, 4096, 512, accumulate=0, a_mode=0, lda=512, b_mode=0, ldb=512)], []),
    "plain_accumulate": lambda: ([_product(0, 136, 136, 520, accumulate=1)], []),
    "batch": lambda: ([_product(0, 136, 136, 520, batch=2)], []),
    "bias": lambda: ([_product(0, 136, 136, 520, bias=0x20000000)], []),
    "activation": lambda: ([_product(0, 136, 136, 520, act=2)], []),
    "gate": lambda: ([_product(0, 136, 136, 520, gate=0x20000000, ld_gate=136)], []),
    "addend": lambda: ([_product(0, 136, 136, 520, addend=0x20000000, ld_add=136)], []),
    "row_mask": lambda: ([_product(0, 136, 136, 520, row_period=30, row_lo=2, row_hi=27)], []),
    "statistics": lambda: ([_product(0, 136, 136, 520, col_sum=0x20000000, stat_part=0x21000000)], []),
    "presplit": lambda: ([_product(0, 136, 136, 520, A_lo=0x20000000, B_lo=0x21000000)], []),
    "alpha": lambda: ([_product(0, 136, 136, 520, alpha=1.5)], []),
    "bf16_C": lambda: ([_product(0, 136, 136, 520, c_dtype=BF16)], []),
    "null_operand": lambda: ([_product(0, 136, 136, 520, B=None)], []),
    "refused_among_good": lambda: ([_product(0, 136, 136, 520), _product(1, 136, 136, 520, accumulate=1)], [_sum(2, 520, 264)]),
    "overlapping_C": lambda: ([_product(0, 136, 136, 520), _product(1, 136, 136, 520, C=0x10000000 + 32 * MB + 135 * 136 * 4)], []),
    "C_over_sum_out": lambda: ([_product(0, 136, 136, 520)], [_sum(1, 520, 264, out=0x10000000 + 32 * MB + 64)]),
    "shared_scratch": lambda: ([_product(0, 136, 136, 520, split_k=2, det=True),
                                _product(1, 136, 136, 520, split_k=2, det=True, splitk_work=0x10000000 + 40 * MB + 4096)], []),
    "shared_counters": lambda: ([_product(0, 136, 264, 520, split_k=2, det=True),
                                 _product(1, 136, 136, 520, split_k=2, det=True, splitk_count=0x10000000 + 60 * MB + 4)], []),
    "shared_sum_work": lambda: ([], [_sum(0, 520, 264), _sum(1, 520, 264, work=0x10000000 + 40 * MB + 512)]),
    "scratch_over_sum_work": lambda: ([_product(0, 136, 136, 520, split_k=2, det=True, splitk_work=0x10000000 + 64 * MB + 40 * MB)],
                                      [_sum(1, 520, 264)]),
    "sum_rows_unaligned": lambda: ([], [_sum(0, 520, 264, ld=266)]),
    "sum_ragged_without_padding": lambda: ([], [_sum(0, 300, 101, dtype=F32, ld=101)]),
    "sum_null": lambda: ([], [_sum(0, 520, 264, out=None)]),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusals_plan_nothing(case):
    products, sums = REFUSED[case]()
    rc, entries, launches = _plan(products, sums)
    assert rc == BAD_ARG, case
    assert launches == 0 and all(e.index == -77 for e in entries)
    assert _lib.lib().ns_last_error()
    # and the launching entry point refuses the same list before it touches a device
    lib = _lib.lib()
    ap = (_lib.STRUCTS["ns_gemm_params"] * len(products))(*products) if products else None
    asum = (_lib.STRUCTS["ns_colsum_params"] * len(sums))(*sums) if sums else None
    assert lib.ns_gemm_group(ap, len(products), asum, len(sums), None) == BAD_ARG


def test_null_and_empty_lists():
    lib = _lib.lib()
    nl = ctypes.c_int(-5)
    assert lib.ns_gemm_group_plan(None, 0, None, 0, None, ctypes.byref(nl)) == BAD_ARG and nl.value == 0
    assert lib.ns_gemm_group_plan(None, 2, None, 0, None, None) == BAD_ARG
    assert lib.ns_gemm_group(None, 0, None, 0, None) == BAD_ARG
    assert lib.ns_gemm_group(None, 0, None, 3, None) == BAD_ARG


def test_single_launch_entry_points_classify_as_before():
    """The classification that ns_gemm_group asks is the one ns_gemm dispatches by: a refused product is still a valid
    ns_gemm call (its checks pass up to the launch, which a host without a device cannot make - so only the argument
    errors are compared here)."""
    lib = _lib.lib()
    p = _product(0, 136, 136, 520, c_dtype=BF16)
    assert lib.ns_gemm(ctypes.byref(p), None) == BAD_ARG and b"accumulate needs fp32 C" in lib.ns_last_error()
