"""ns_gemm_plan (include/nspeech_hip.h): what ns_gemm would launch, asked without a device.  ns_gemm and the query share
one function up to the launch (csrc/gemm.hip: gemm_prepare), so what is pinned here is what runs.

 - every entry of FORMS in test_gemm_epilogue_gpu.py selects the kernel that test asserts after its launch;
 - the plans of the case list in gemm_plan_cases.py - both sides of every threshold of the choice, every argument check,
   every environment switch - are those of the commit before the kernel-form table, tests/golden/gemm_plan.json (its
   header says how they were recorded);
 - the models' own copies of the 256-tile thresholds agree with the library;
 - ns_gemm_group_plan accepts exactly the products that the query puts on one of the group's two forms.
NS_GEMM_HALF is read once per process: its cases run in a child process each, everything else here needs it unset."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

import gemm_plan_cases as G
from nspeech_amd import _lib
from test_gemm_epilogue_gpu import FORMS

BF16, F32 = _lib.NS_BF16, _lib.NS_F32
GROUP_FORMS = ("gemm_mfma_kernel<1, 1, false, 64, 128>", "gemm_mfma_f32_kernel<1, 1, 1, false, 128>")
PINNED = json.load(open(G.GOLDEN))["plans"]


@pytest.fixture(autouse=True)
def default_half_tiles():
    assert "NS_GEMM_HALF" not in os.environ, "these tests pin the default half-tile rule: unset NS_GEMM_HALF"


def test_abi():
    info = _lib.STRUCTS["ns_gemm_plan_info"]
    assert [f[0] for f in info._fields_] == ["kernel", "loop", "grid_x", "grid_y", "grid_z", "block", "lds_bytes", "stat_slots"]
    assert ctypes.sizeof(info) == 40
    assert "ns_gemm_plan" in _lib.FUNCS and hasattr(_lib.lib(), "ns_gemm_plan")
    assert _lib.lib().ns_version() >= 103
    assert _lib.lib().ns_gemm_plan(ctypes.byref(G.product()), None) == -1           # a null `out` is an argument error


# ------------------------------------------------------------------ the forms of the epilogue test
def _form_block(f):
    """The block test_gemm_epilogue_gpu._run_case hands to ns_gemm for form f under its plainest option set (the
    split-K set for the BK = 32 form, which is a launch of 600 workgroups): the same offsets, leading dimensions and
    alignment, over base addresses aligned as a device allocation is."""
    esz = 2 if f.dtype == torch.bfloat16 else 4
    aligned = f.kernel != "gemm_generic_kernel"
    pad, off = (8, 8) if aligned else (3, 3)
    lda = (f.K if f.a_mode == 0 else f.M) + pad
    ldb = (f.K if f.b_mode == 0 else f.N) + pad
    cpad = 8 if f.vec else 3
    ldc, c_off = f.N + cpad, (2 * (f.N + cpad) + 4 if f.vec else 1)
    kw = dict(A=G.A0 + off * esz, lda=lda, B=G.B0 + 2 * off * esz, ldb=ldb, C=G.C0 + c_off * 4, ldc=ldc, f32_passes=f.passes)
    if "presplit" in f.caps:
        kw.update(A_lo=G.X[3] + off * esz, B_lo=G.X[4] + 2 * off * esz)
    if "bk32" in f.caps:
        v = 1                                                   # _split_opt(24, ...): bias, fp32 addend, gate, mask
        kw.update(split_k=24, accumulate=2, alpha=1.5, bias=G.X[5] + v * 4, addend=G.X[6] + 2 * v * 4, ld_add=f.N + 4 * v,
                  gate=G.X[7] + 3 * v * esz, ld_gate=f.N + 5, row_period=30, row_lo=2, row_hi=27, row_shift=2)
    return G.product(dtype=BF16 if esz == 2 else F32, M=f.M, N=f.N, K=f.K, a_mode=f.a_mode, b_mode=f.b_mode, **kw)


@pytest.mark.parametrize("form", FORMS, ids=[f.id for f in FORMS])
def test_every_form_of_the_epilogue_test_is_planned_on_its_kernel(form):
    got = G.plan(_form_block(form))
    assert got[6] == 0, got
    assert got[0] == form.kernel


# ------------------------------------------------------------------ the plans of the commit before the table
def test_the_fixture_covers_the_case_list():
    assert sorted(PINNED) == sorted(c["id"] for c in G.CASES)


@pytest.mark.parametrize("case", [c for c in G.CASES if c["half"] is None], ids=lambda c: c["id"])
def test_plan_is_the_parents(case):
    assert G.plan_case(case) == PINNED[case["id"]]


@pytest.mark.parametrize("half", ["0", "1", "300"])
def test_plan_is_the_parents_under_ns_gemm_half(half):
    ids = [c["id"] for c in G.CASES if c["half"] == half]
    assert ids
    r = subprocess.run([sys.executable, G.__file__] + ids, env=dict(os.environ, NS_GEMM_HALF=half), check=True,
                       capture_output=True, text=True)
    got = json.loads(r.stdout)
    assert got == {i: PINNED[i] for i in ids}


def test_a_query_leaves_the_last_launch_alone():
    lib = _lib.lib()
    lib.ns_gemm_last_kernel.restype = lib.ns_gemm_last_loop.restype = ctypes.c_char_p
    before = (lib.ns_gemm_last_kernel(), lib.ns_gemm_last_loop())
    assert G.plan(G.product(**G.KSLOW))[:2] == ["gemm_mfma_kernel<1, 1, false, 64, 128>", "dma"]
    assert (lib.ns_gemm_last_kernel(), lib.ns_gemm_last_loop()) == before


# ------------------------------------------------------------------ the models' copies of the 256-tile thresholds
ROWS = (768, 1023, 1024, 1025, 1280, 1536, 2048, 4096)
COUTS = tuple(128 * n for n in (8, 16, 31, 32, 37, 38, 46, 47, 48, 49, 64, 94, 95, 96, 97, 190, 191, 192))


def test_the_grid_straddles_both_thresholds():
    tiles = lambda r, c: ((r + 255) // 256) * ((c + 255) // 256)      # noqa: E731
    assert {95, 96} <= {tiles(r, c) for r in ROWS for c in COUTS if r >= 1024}
    assert any(tiles(r, c) >= 96 for r in ROWS for c in COUTS if r < 1024)


@pytest.mark.parametrize("rows", ROWS)
def test_x256_fits_is_the_librarys_rule(rows):
    from nspeech_amd.models.tacotron2 import Tacotron2
    for cout in COUTS:
        kernel = G.plan(G.product(M=rows, N=cout, K=512))[0]
        assert Tacotron2._x256_fits(None, rows, cout) == (kernel == "gemm_x256_kernel<1>"), (rows, cout, kernel)


@pytest.mark.parametrize("rows", ROWS)
def test_x256_split_ok_is_the_librarys_rule(rows):
    """the shape conditions of _x256_split_ok (a mixed-precision model with a pre-split shadow of the weights), over
    pre-split operands: where it says no, the library refuses the call"""
    from types import SimpleNamespace
    from nspeech_amd.models.tacotron2 import Tacotron2
    model = SimpleNamespace(mode="mixed", tsh={"postT_0_hi": object()})
    for cout in COUTS + (128 * 48 + 64,):                       # and one that is no multiple of 128
        for k, cin in ((5, 512), (5, 24), (1, 96)):             # k * cin: 2560, 120 (not a multiple of 64), 96 (neither)
            K = k * cin
            got = G.plan(G.product(M=rows, N=cout, K=K, f32_passes=3, **G.LO))
            want = Tacotron2._x256_split_ok(model, "post0", rows, cin, cout, k)
            assert want == (got[0] == "gemm_x256_kernel<3>"), (rows, cout, K, got)
            assert want or got[6] == -1


# ------------------------------------------------------------------ the grouped launch asks the same question
def _group_accepts(p):
    arr = (_lib.STRUCTS["ns_gemm_params"] * 1)(p)
    return _lib.lib().ns_gemm_group_plan(arr, 1, None, 0, None, None) == 0


def _group_candidates():
    """the pinned products that meet every condition of ns_gemm_group but the kernel form"""
    out = []
    for c in G.CASES:
        f = c["p"]
        if f is None or c["env"] or c["half"] or PINNED[c["id"]][6] != 0 or PINNED[c["id"]][0] is None:
            continue
        if f.get("accumulate") != 2 or f.get("batch", 1) > 1 or f.get("alpha", 1.0) != 1.0:
            continue
        if any(k in f for k in ("bias", "gate", "addend", "col_sum", "stat_z", "A_lo", "B_lo", "row_period", "act", "c_dtype")):
            continue
        out.append(c)
    return out


def test_the_candidates_fall_on_both_sides():
    names = [PINNED[c["id"]][0] for c in _group_candidates()]
    assert all(names.count(n) >= 2 for n in GROUP_FORMS) and sum(n not in GROUP_FORMS for n in names) >= 8


@pytest.mark.parametrize("case", _group_candidates(), ids=lambda c: c["id"])
def test_group_accepts_exactly_its_two_forms(case):
    f = case["p"]
    named = G.plan_case(case)[0] in GROUP_FORMS
    # (the form's name says "1, 1" for whatever the mode ladder's last rung took; the group wants the modes themselves)
    assert _group_accepts(G.product(**f)) == (named and f.get("a_mode") == 1 and f.get("b_mode") == 1)
