"""The case table and the criteria of the gate kernels' device test (tests/gate_fixtures.py), checked on the CPU: through
lk_gate_variant (host code) the table reaches every path of csrc/lk_gate.hip and every refusal of its shape guards; the rule in
torch (`torch_math`, which the emulation runs) meets the criteria on every case; every mutant of it fails at least one case."""
import pytest
import torch

from tests import gate_fixtures as gf

RUN = [c for c in gf.CASES if not c["wide"]]


@pytest.fixture(scope="module")
def K():
    import os

    from laplace_amd._lib import LIB_PATH, HipKernels

    if not os.path.exists(LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return HipKernels()


def _variant(K, c):
    return K.gate_variant(c["kind"] == "vjp", c["S"], c["B"], c["P"], c["C"], aligned=not c["off"])


def test_the_cases_are_small_and_distinct():
    assert len({gf.case_id(c) for c in gf.CASES}) == len(gf.CASES)
    for c in RUN:
        assert c["S"] * c["B"] * c["P"] * c["C"] <= 4 << 20 and c["P"] <= 4096, gf.case_id(c)
    assert {c["P"] for c in RUN} >= {1, 2, 3, 16, 49, 64, 128, 129, 512, 513, 1024}
    assert {c["C"] for c in RUN} >= {1, 3, 4, 8, 32, 36, 64, 260}
    assert {c["B"] for c in RUN} >= {0, 1, 2, 5} and {c["S"] for c in RUN} >= {1, 3, 9}
    for kind in ("reduce", "vjp"):
        assert {(c["split"], c["off"]) for c in RUN if c["kind"] == kind} == {(a, b) for a in (False, True) for b in (0, 1)}
    assert {(c["r"], c["amax"], c["split"]) for c in RUN if c["kind"] == "vjp"} == {(a, b, s) for a in (False, True) for b in (False, True)
                                                                                 for s in (False, True)}


def test_the_table_reaches_every_path(K):
    plans = {gf.case_id(c): _variant(K, c) for c in gf.CASES}
    assert all(p is not None for p in plans.values())
    for kind in ("reduce", "vjp"):
        mine = [(c, plans[gf.case_id(c)]) for c in gf.CASES if c["kind"] == kind]
        run = [(c, p) for c, p in mine if not c["wide"]]
        # vector and scalar path, each with an fp32 and a split cotangent; every lane count from 1 to 64
        assert {(p["vec"], c["split"]) for c, p in run} == {(v, s) for v in (False, True) for s in (False, True)}
        assert {p["lanes"] for c, p in run} >= {1, 2, 4, 8, 16, 32, 64}
        # channel vectors that do not fill the lanes (36 channels: nine vectors on 16 lanes), a second channel tile (260)
        assert any(p["vec"] and c["C"] == 36 and p["lanes"] == 16 for c, p in run)
        assert any(c["C"] == 260 and c["B"] > 0 for c, p in run)
        # a unit count at the grid's limit with units left over: the grid strides
        assert any(p["blocks"] == gf.MAX_BLOCKS for c, p in run) and any(0 < p["blocks"] < gf.MAX_BLOCKS for c, p in run)
        assert any(p["blocks"] == 0 and c["B"] == 0 for c, p in run)
        # 64-bit indexing: by shape only
        assert any(p["wide_index"] for c, p in mine) and not any(p["wide_index"] for c, p in run)
        assert all(c["wide"] == p["wide_index"] for c, p in mine)
    red = [(c, plans[gf.case_id(c)]) for c in RUN if c["kind"] == "reduce"]
    # x resident and re-read, on both paths, at the limit and one position past it; the seeds over grid.y and in one slice
    for vec, lim in ((True, 512), (False, 128)):
        at = [p for c, p in red if p["vec"] == vec and c["C"] == 32 and c["P"] == lim]
        past = [p for c, p in red if p["vec"] == vec and c["C"] == 32 and c["P"] == lim + 1]
        assert at and past and all(p["resident"] for p in at) and not any(p["resident"] for p in past)
    assert {(p["resident"], c["split"]) for c, p in red} == {(r, s) for r in (False, True) for s in (False, True)}
    assert {p["seed_split"] for c, p in red if c["S"] > 1 and c["B"] > 0} == {False, True}
    assert all(p["resident"] == (c["P"] <= (256 // p["lanes"]) * gf.RESIDENT_POSITIONS) for c, p in red)
    vjp = [(c, plans[gf.case_id(c)]) for c in RUN if c["kind"] == "vjp"]
    assert not any(p["resident"] or p["seed_split"] for c, p in vjp)
    # positions past one chunk of the VJP: more workgroups than maps x channel tiles
    assert any(c["P"] > (256 // p["lanes"]) * gf.VJP_POSITIONS and p["blocks"] > c["S"] * c["B"] for c, p in vjp)


REFUSED = [dict(S=0), dict(B=-1), dict(P=0), dict(P=1 << 30), dict(C=0), dict(C=1 << 30), dict(S=1 << 10, B=1 << 10, P=1 << 10, C=1 << 10),
           dict(S=1 << 40, B=1, P=1, C=1)]
ACCEPTED = [dict(S=1), dict(B=0), dict(P=1), dict(P=(1 << 30) - 1, S=1, B=1, C=1), dict(C=1), dict(C=(1 << 30) - 1, S=1, B=1, P=1),
            dict(S=(1 << 10) - 1, B=1 << 10, P=1 << 10, C=1 << 10), dict(S=(1 << 40) - 1, B=1, P=1, C=1)]


@pytest.mark.parametrize("vjp", (False, True))
def test_the_variant_query_refuses_what_the_guards_refuse(K, vjp):
    base = dict(S=3, B=2, P=16, C=32)
    for edit in REFUSED:
        assert K.gate_variant(vjp, **{**base, **edit}) is None, edit
    for edit in ACCEPTED:
        assert K.gate_variant(vjp, **{**base, **edit}) is not None, edit
    assert K.lib.lk_gate_variant(2, 3, 2, 16, 32, 1) == -1 and K.lib.lk_gate_variant(-1, 3, 2, 16, 32, 1) == -1


@pytest.fixture(scope="module")
def worked():
    """per runnable case ``(inputs, fp64 reference)``, computed once"""
    out = {}
    for i, c in enumerate(gf.CASES):
        if not c["wide"]:
            inp = gf.make_inputs(c, torch.Generator().manual_seed(100 + i))
            out[gf.case_id(c)] = (inp, gf.reference(c, inp))
    return out


@pytest.mark.parametrize("c", RUN, ids=gf.case_id)
def test_the_rule_in_torch_meets_the_criteria(c, worked):
    inp, ref = worked[gf.case_id(c)]
    assert gf.violations(c, gf.torch_math(c, inp), ref, inp) == []
    if c["split"]:  # (the reference of a split case is the reconstruction of its planes)
        assert torch.equal(inp["g_split"].float().reshape(inp["g"].shape), inp["g"])


@pytest.mark.parametrize("mutant", gf.MUTANTS)
def test_every_mutant_fails_a_case(mutant, worked):
    caught = [gf.case_id(c) for c in RUN if gf.violations(c, gf.torch_math(c, worked[gf.case_id(c)][0], mutant), worked[gf.case_id(c)][1],
                                                          worked[gf.case_id(c)][0])]
    assert caught, f"no case notices the mutant {mutant}"
