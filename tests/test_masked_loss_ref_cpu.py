"""tests/masked_loss_ref.py is the yardstick of tests/test_masked_loss_contract_gpu.py: here its vectorised statement of
ns_l1_loss_masked's contract is held to a naive triple loop, its own outputs pass its own comparison, and each deliberate
mutant - a kernel with one defect - is shown to fail at least one named case."""
import numpy as np
import pytest

import masked_loss_ref as R

SMALL = [n for n in R.case_names() if "rows" not in n]


@pytest.mark.parametrize("name", [n for n in SMALL if "1025" not in n or n in ("wide-1025-bf16", "wide-1025-ld1025")])
def test_reference_equals_the_triple_loop(name):
    c = R.build(name)
    e, n = R.expect(c), R.naive(c)
    assert np.array_equal(e["acc"], n["acc"])                 # multiples of 1/4: exact in any order
    if c["ddt"]:
        assert R.bits_equal(e["dpred"], n["dpred"]).all()
        assert (e["dpred"][:R.MARGIN] == R.SENT).all() and (e["dpred"][-R.MARGIN:] == R.SENT).all()
    else:
        assert e["dpred"] is None and n["dpred"] is None


def test_random_case_equals_the_triple_loop_within_float64():
    c = R.build("narrow-16-random")
    e, n = R.expect(c), R.naive(c)
    assert np.allclose(e["acc"], n["acc"], rtol=1e-13, atol=0)
    assert R.bits_equal(e["dpred"], n["dpred"]).all()


@pytest.mark.parametrize("name", R.case_names() + R.case_names(random=True) + R.probe_names())
def test_the_contract_passes_its_own_comparison(name):
    c = R.build(name)
    acc, dpred = R.mutant_outputs(c, None)
    assert not R.check(c, acc, dpred), R.check(c, acc, dpred)
    if "-probe-" in name:
        n, t, _ = (int(x[1:]) for x in name.split("-probe-")[1].split("-"))
        live = t < R.frames_of(c["lengths"], c["p"]["N"], c["p"]["T"])[n]
        assert R.expect(c)["acc"][0] == (1.0 if live else 0.0)


def test_what_the_cases_cover():
    cs = {n: R.build(n) for n in SMALL}
    ps = [c["p"] for c in cs.values()]
    assert {p["F"] for p in ps} == {1025, 257, 256, 80, 78, 16}
    assert any(p["ldp"] % 4 for p in ps) and any(c["ddt"] and c["p"]["ldd"] % 4 for c in cs.values())
    assert {c["ddt"] for c in cs.values()} == {"f32", "bf16", None}
    assert {0, 205} <= {p["n_prio"] for p in ps} and any(p["n_prio"] == p["F"] for p in ps)
    assert any(c["lengths"] is None for c in cs.values())
    flat = [x for c in cs.values() if c["lengths"] for x in c["lengths"]]
    assert 0 in flat and min(flat) < 0 and max(flat) > 20 and 1 in flat
    assert cs["taco1-mel"]["p"]["P"] == 25 and cs["taco1-mel"]["p"]["padl"] == 5
    big = R.build("wide-256-rows4250")["p"]
    assert big["N"] * big["T"] > 4 * 1024
    big = R.build("narrow-80-rows6800")["p"]
    assert big["N"] * big["T"] * big["F"] // 4 > 512 * 256


# each mutant and a case that must reject it (found among all cases below as well)
NAMED = {"off_by_one": "wide-1025-bf16", "stale_rows": "narrow-80", "no_clamp": "narrow-16-clamps", "prio_all": "wide-256",
         "sign0": "narrow-78"}


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_each_mutant_fails_its_named_case(mut):
    c = R.build(NAMED[mut])
    acc, dpred = R.mutant_outputs(c, mut)
    bad = R.check(c, acc, dpred)
    print(mut, NAMED[mut], bad)
    assert bad


def test_mutants_against_every_case():
    """Which cases see which mutant: every gradient case sees sign0 and stale_rows (when a row is padded), the sums alone
    see off_by_one and no_clamp."""
    seen = {m: [] for m in R.MUTANTS}
    for name in SMALL + R.probe_names():
        c = R.build(name)
        for m in R.MUTANTS:
            if R.check(c, *R.mutant_outputs(c, m)):
                seen[m].append(name)
    for m, names in seen.items():
        print(m, len(names))
        assert names, m
    assert "wide-1025-nograd" in seen["off_by_one"] and "narrow-80-nograd" in seen["off_by_one"]       # by the sums alone
    assert "wide-256-clamps" in seen["no_clamp"]
    assert "narrow-80-probe-n1-t12-f0" in seen["off_by_one"]           # the first padded frame of a row
