"""The case table of tests/spectral_fixtures.py against the launch rules of csrc/lk_spectral.hip (asked through
``lk_spectral_variant``, host code), and the derived bound against fp32 restatements and mutants - all without a device."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import spectral_fixtures as sf  # noqa: E402


@pytest.fixture(scope="module")
def K():
    from laplace_amd._lib import LIB_PATH, HipKernels

    if not os.path.exists(LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return HipKernels()


def _variant(K, c):
    return K.spectral_variant(sf.form_of(c), c["N"], c["C"], c["DP"], c["G"], not c["unaligned"])


def test_the_table_reaches_every_launch_form(K):
    seen, tiles_per, edges = set(), set(), {"P": set(), "N": set(), "G": set()}
    for c in sf.CASES:
        v = _variant(K, c)
        assert v is not None, sf.case_id(c)
        P = sf.n_params(c)
        ntj = -(-P // sf.TILE_J)
        assert v["ll"] == (c["loader"] == "ll") and v["grid"] == (c["epi"] == "grid")
        assert v["pairs"] == (c["epi"] == "cov" and c["C"] > 10)
        assert v["gc"] == (5 if v["ct"] == 10 else 64 // v["ct"])
        seen.add((c["loader"], c["epi"], v["ct"], v["pairs"]))
        tiles_per.add((c["loader"], c["epi"], -(-ntj // v["split"])))
        edges["P"].add((c["loader"], P % sf.TILE_J if P > sf.TILE_J else P))
        edges["N"].add((c["loader"], c["N"] % sf.TILE_N if c["N"] < sf.BIG_N else 0))
        if v["grid"]:
            edges["G"].add((v["ct"], c["G"] - v["gc"] if abs(c["G"] - v["gc"]) <= 1 else c["G"]))
    for loader in ("ll", "r"):
        for epi in ("cov", "grid"):
            for ct in (1, 2, 5, 10):
                assert (loader, epi, ct, False) in seen, (loader, epi, ct)
            assert (loader, epi, 1) in tiles_per and (loader, epi, 2) in tiles_per  # one tile per workgroup, and a range of two
        assert (loader, "cov", 10, True) in seen
        assert {(loader, 1), (loader, 31), (loader, 1)} <= edges["N"] and (loader, 1) in edges["P"]
    assert {("r", p) for p in (1, 127, 128, 129 - 128, 257 - 256)} <= edges["P"]
    assert {c["G"] for c in sf.CASES if c["epi"] == "grid" and c["C"] == 1} >= {1, 63, 64, 65, 100, 130}
    assert {(1, -1), (1, 0), (1, 1), (1, 100), (1, 130), (10, -1), (10, 0), (10, 1), (10, 100)} <= edges["G"]
    assert any(c["unaligned"] for c in sf.CASES if c["loader"] == "ll") and any(c["unaligned"] for c in sf.CASES if c["loader"] == "r")
    assert {c["DP"] for c in sf.CASES if c["loader"] == "ll"} >= {1, 31, 33}
    assert {c["C"] for c in sf.CASES} >= {1, 2, 3, 10, 11, 21}


def test_the_variant_refuses_what_the_entry_points_refuse(K):
    assert K.spectral_variant(sf.QUAD_LL, 4, 2, 896) is not None and K.spectral_variant(sf.QUAD_LL, 4, 2, 897) is None
    assert K.spectral_variant(sf.QUAD_R, 4, 2, 32768) is not None and K.spectral_variant(sf.QUAD_R, 4, 2, 32769) is None
    assert K.spectral_variant(sf.QUAD_LL | sf.BIAS, 4, 64, 511) is not None and K.spectral_variant(sf.QUAD_LL | sf.BIAS, 4, 64, 512) is None
    assert K.spectral_variant(sf.QUAD_R | sf.BIAS, 4, 2, 16) is None and K.spectral_variant(8, 4, 2, 16) is None
    assert K.spectral_variant(sf.GRID_R, 0, 2, 16) is None and K.spectral_variant(sf.GRID_R, 1, 0, 16) is None


SMALL = [i for i, c in enumerate(sf.CASES) if c["N"] <= 33 and c["C"] <= 11 and c["G"] <= 33]


def test_two_restatements_stay_inside_the_bound():
    worst = 0.0
    for i in SMALL:
        for block in (128, 16):
            r = sf.ratio(sf.restate(i, block), i)
            assert r <= 1.0, (sf.case_id(sf.CASES[i]), block, r)
            worst = max(worst, r)
    print(f"worst |err| / bound of the fp32 restatements: {worst:.3f}")
    assert worst > 0.0  # (the restatements do round)


def test_exact_cases_are_exact_in_any_order():
    for i, c in enumerate(sf.CASES):
        if c["exact"]:
            want = sf.reference(i)[0]
            for block in (128, 16):
                assert torch.equal(sf.restate(i, block).double(), want), sf.case_id(c)


@pytest.mark.parametrize("mutant", sf.MUTANTS)
def test_mutants_leave_the_bound(mutant):
    def applies(c):
        if c["exact"]:
            return False
        if mutant in ("hfac_dropped", "delta_before_hfac"):
            return c["hfac"] != 1.0
        if mutant == "grid_not_squared":
            return c["epi"] == "grid"
        if mutant == "bias_dropped":
            return c["loader"] == "ll" and c["bias"] == 1
        return c["loader"] == "ll" and c["DP"] > 1

    def blind(c):
        """hfac only scales lam: where the prior precision exceeds hfac lam_max by 2^24 the weights are the same fp32 numbers with
        and without it.  That holds for the single-prior rows at delta = 1e4 (lam <= 10, hfac <= 7) and for no other row."""
        return mutant == "hfac_dropped" and c["G"] == 1 and c["delta"] == max(sf.DELTAS)

    hit = [i for i in SMALL if applies(sf.CASES[i]) and not blind(sf.CASES[i])]
    assert len(hit) >= 4
    missed = [sf.case_id(sf.CASES[i]) for i in hit if sf.ratio(sf.restate(i, 128, mutant), i) <= 1.0]
    assert not missed, missed


def test_the_grid_loop_fixture_separates_its_two_best_points():
    """(asserted inside the fixture, in fp64 on the CPU; here: that it runs, and what it hands the device test)"""
    case = sf.grid_loop_case()
    two = torch.sort(case["losses"]).values[:2]
    assert 0 < case["tol"] < 1e-4 and float(two[1] - two[0]) > 2 * case["tol"]
    assert case["argmin"] == int(case["losses"].argmin()) and len(case["grid"]) == len(case["losses"])
