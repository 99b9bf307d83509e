"""The fixture table of the pooling kernels (tests/pool_fixtures.py) does what tests/test_gpu_pool.py relies on - on the CPU:

* through ``lk_pool_variant`` (pure host code of csrc/lk_pool.hip) the table reaches every path: 16-byte and scalar loads,
  selection and summing, the seeds in one slice and split over grid.y, and a seed loop that ends one short of, at, and one past
  the seeds per pass;
* the emulation (tests/emulated_pool_kernels.py: the window walked tap by tap with a strict ``>``) meets every assertion of the
  device test against the float64 references, and a MUTANT that breaks ties towards the last maximum fails the post-ReLU cases:
  the references can tell the tie rule;
* the end-to-end fixtures keep the gaps that make a comparison of two separately executed passes meaningful: a max pool decides
  like a ReLU mask, so in the float64 forward the two largest distinct values of every window, and every ReLU pre-activation and
  zero, are further apart than 1e-3 of the map's maximum (exact ties are served by the tie rule).
"""
import os

import pytest
import torch

from tests import pool_fixtures as pf
from tests.emulated_pool_kernels import EmulatedPoolKernels


@pytest.fixture(scope="module")
def variant():
    from laplace_amd._lib import LIB_PATH, HipKernels

    if not os.path.exists(LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    K = HipKernels()
    return lambda c, aligned=None: K.pool_variant(pf.kernel_kind(K, c), c["S"], c["B"], c["H"], c["W"], c["C"], c["k"], c["s"],
                                                  c["p"], not c["off"] if aligned is None else aligned)


def test_the_table_reaches_every_path(variant):
    plans = [variant(c) for c in pf.CASES]
    assert all(p is not None for p in plans)
    assert {p["seeds_per_pass"] for p in plans} == {pf.SEEDS_PER_PASS}
    for kind in ("max", "avg"):
        mine = [(c, p) for c, p in zip(pf.CASES, plans) if c["kind"] == kind]
        seen = {(p["vec"], p["summing"]) for _, p in mine}
        assert seen == {(v, s) for v in (False, True) for s in (False, True)}, (kind, seen)
        assert {p["seed_split"] for _, p in mine} == {False, True}, kind
    for c, p in zip(pf.CASES, plans):
        assert p["summing"] == (not pf.selection(c)) and p["vec"] == (c["C"] % 4 == 0 and not c["off"]), pf.case_id(c)
    # the seeds a lane loops over: the slice, and the last slice's remainder
    loops = set()
    for c, p in zip(pf.CASES, plans):
        loops |= {min(p["seeds_per_slice"], c["S"]), c["S"] - (-(-c["S"] // p["seeds_per_slice"]) - 1) * p["seeds_per_slice"]}
    assert {pf.SEEDS_PER_PASS - 1, pf.SEEDS_PER_PASS, pf.SEEDS_PER_PASS + 1} <= loops, sorted(loops)
    split_with_remainder = [c for c, p in zip(pf.CASES, plans) if p["seed_split"] and p["seeds_per_slice"] > pf.SEEDS_PER_PASS]
    assert split_with_remainder, "no case splits the seeds AND loops more than one pass in a slice"
    # an unaligned base turns the 16-byte path off for a channel count that would take it
    c = next(c for c in pf.CASES if c["off"] and c["C"] % 4 == 0)
    assert variant(c, True)["vec"] and not variant(c, False)["vec"]


def test_the_table_holds_what_the_device_test_lists():
    geos = {(c["k"], c["s"], c["p"], (c["H"], c["W"])) for c in pf.CASES}
    pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)  # noqa: E731
    assert {tuple(pair(v) for v in g) for g in pf.GEOMETRIES} <= geos
    for kind in ("max", "avg"):
        mine = [c for c in pf.CASES if c["kind"] == kind]
        assert {c["C"] for c in mine} >= {4, 6, 8, 12, 68} and {c["B"] for c in mine} >= {1, 3}, kind
        assert {c["S"] for c in mine} >= {1, 2, 9, 17} and {c["off"] for c in mine} == {0, 1}, kind
    for g in geos:
        assert {c["inp"] for c in pf.CASES if c["kind"] == "max" and (c["k"], c["s"], c["p"], (c["H"], c["W"])) == g} \
            >= ({"rand", "relu", "neg", "const"} if g[3][0] < 32 else {"relu"})
    avg = [c for c in pf.CASES if c["kind"] == "avg"]
    assert {c["cip"] for c in avg if c["p"] != (0, 0)} == {False, True} and any(c["div"] for c in avg)


def _run(K, c):
    """the assertions of tests/test_gpu_pool.py on a kernel object -> list of failures"""
    gen = torch.Generator().manual_seed(11 + pf.CASES.index(c))
    x = pf.make_input(c, gen)
    kind, (OH, OW), bad = pf.kernel_kind(K, c), pf.out_hw(c), []
    y, arg = K.pool_forward(x, kind, c["k"], c["s"], c["p"], c["cip"], c["div"])
    ref = pf.forward_reference(c, x)
    if c["kind"] == "max":
        if not torch.equal(y.double(), ref["y"]):
            bad.append("y")
        if not torch.equal(pf.codes_to_flat_index(c, arg), ref["idx"]):
            bad.append("arg")
    elif not bool(((y.double() - ref["y"]).abs() <= ref["bound"]).all()):
        bad.append("y")
    g = torch.randn(c["S"], c["B"], OH, OW, c["C"], generator=gen)
    amax = torch.zeros(1)
    dx = K.pool_vjp(g.reshape(c["S"] * c["B"], OH, OW, c["C"]), arg, c["S"], (c["H"], c["W"]), kind, c["k"], c["s"], c["p"],
                    c["cip"], c["div"], amax=amax).reshape(c["S"], c["B"], c["H"], c["W"], c["C"])
    # (a wrong argmax also moves the cotangent: the VJP is checked against the REFERENCE's indices)
    want, bound = pf.vjp_reference(c, g, ref.get("idx"))
    if bound is None:
        if not torch.equal(dx, want.float()):
            bad.append("dx")
    elif not bool(((dx.double() - want).abs() <= bound).all()):
        bad.append("dx")
    if not torch.equal(amax.view(torch.int32), dx.abs().max().reshape(1).view(torch.int32)):
        bad.append("amax")
    return bad


@pytest.mark.parametrize("c", pf.CASES, ids=pf.case_id)
def test_the_emulation_meets_the_references(c):
    assert _run(EmulatedPoolKernels(), c) == []


def test_a_last_maximum_mutant_fails_the_post_relu_cases():
    mutant = EmulatedPoolKernels()
    mutant.last_wins = True
    # (a window of zeros is where the two rules part: one in 16 of the four-tap windows, none of the 64-tap ones)
    relu = [c for c in pf.CASES if c["kind"] == "max" and c["inp"] == "relu" and c["k"][0] * c["k"][1] <= 4]
    assert len(relu) >= 4
    caught = [c for c in relu if {"arg", "dx"} <= set(_run(mutant, c))]
    assert len(caught) == len(relu), [pf.case_id(c) for c in relu if c not in caught]
    # (the maximum itself is the same either way; with distinct values the mutant is indistinguishable)
    rand = next(c for c in pf.CASES if c["kind"] == "max" and c["inp"] == "rand")
    assert _run(mutant, rand) == []


@pytest.mark.parametrize("name", sorted(pf.E2E))
def test_the_end_to_end_fixtures_keep_their_decisions_clear_of_near_ties(name):
    gaps, seen = pf.e2e_gaps(name)
    net, act = pf.E2E[name][:2]
    assert seen["window"] >= 1000, seen  # (the probes looked at the pools ...)
    assert (seen["relu"] >= 9000) == (act == "relu"), seen  # (... and at every ReLU of a ReLU network)
    assert gaps["window"] > pf.GAP, f"two distinct values of a pooling window lie {gaps['window']:.2e} of the map's maximum apart"
    assert gaps["relu"] > pf.GAP, f"a ReLU pre-activation lies {gaps['relu']:.2e} of the map's maximum from zero"
