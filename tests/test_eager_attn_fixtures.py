"""CPU proofs about tests/eager_attn_fixtures.py, on which the device tests of csrc/lk_softmax.hip and csrc/lk_matmul.hip rest:
the case tables reach every launch path of both entry points (asked of the library's host-only ``*_variant`` queries), the
acceptance criteria hold for an fp32 evaluation of the kernels' rules in forward, reversed and pairwise order, and they reject
wrong kernels (softmax without the ``- sum g y`` term, the dot taken without ``y``, log-softmax with ``y`` for ``exp(y)``, ``da``
with ``b`` untransposed, ``db`` from the wrong seed).  The recorded ``expf`` constant is re-measured."""
import pytest
import torch

from tests import eager_attn_fixtures as ef

SMX = [i for i, c in enumerate(ef.SOFTMAX_CASES) if not c["wide"]]
MM = [i for i, c in enumerate(ef.MATMUL_CASES) if not c["wide"]]
# (the ordered evaluations keep every product of a dot in memory: the cases they can afford)
MM_SMALL = [i for i in MM if ef.MATMUL_CASES[i]["S"] * ef.MATMUL_CASES[i]["NB"] * ef.MATMUL_CASES[i]["M"] * ef.MATMUL_CASES[i]["K"]
            * ef.MATMUL_CASES[i]["N"] <= 1 << 24]


@pytest.fixture(scope="module")
def K():
    from laplace_amd._lib import HipKernels

    return HipKernels()


def test_the_softmax_table_reaches_every_launch_path(K):
    plans = [K.softmax_vjp_variant(c["S"], c["R"], c["L"], c["log"], not c["off"]) for c in ef.SOFTMAX_CASES]
    assert all(p is not None for p in plans)
    # the eight kernel instances: 16- / 4-byte accesses x softmax / log x resident / re-read per seed
    assert {(p["vec"], p["log"], p["resident"]) for p in plans} == {(v, lg, r) for v in (0, 1) for lg in (0, 1) for r in (0, 1)}
    assert {p["lanes_per_row"] for p in plans} == {1, 2, 4, 8, 16, 32, 64}
    assert {p["seed_split"] for p in plans} == {False, True} and {p["wide_index"] for p in plans} == {False, True}
    for c, p in zip(ef.SOFTMAX_CASES, plans):
        assert p["wide_index"] == c["wide"] and p["vec"] == (c["L"] % 4 == 0 and not c["off"])
        nvec = c["L"] // 4 if p["vec"] else c["L"]
        assert p["resident"] == (nvec <= 8 * p["lanes_per_row"])
    # one either side of the resident limit on both paths; a grid that strides; rows either side of a workgroup's
    by = {(c["L"], c["off"], c["log"]): p for c, p in zip(ef.SOFTMAX_CASES, plans) if c["kind"] == "random"}
    assert by[(2048, 0, False)]["resident"] and not by[(2052, 0, False)]["resident"]
    assert by[(511, 0, False)]["resident"] and not by[(513, 0, False)]["resident"]
    assert by[(512, 1, False)]["resident"] and not by[(516, 1, False)]["resident"]
    assert any(p["blocks"] == ef.SMX_MAX_BLOCKS and c["R"] > ef.SMX_MAX_BLOCKS * (256 // p["lanes_per_row"])
               for c, p in zip(ef.SOFTMAX_CASES, plans) if not c["wide"])
    rows = {(c["R"], 256 // p["lanes_per_row"]) for c, p in zip(ef.SOFTMAX_CASES, plans)}
    assert {(15, 16), (17, 16), (3, 4), (5, 4), (255, 256), (257, 256)} <= rows and any(c["R"] == 0 for c in ef.SOFTMAX_CASES)
    assert {c["S"] for c in ef.SOFTMAX_CASES} >= {1, 2, 9} and {c["kind"] for c in ef.SOFTMAX_CASES} == {"random", "masked", "saturated"}
    assert {c["L"] for c in ef.SOFTMAX_CASES} >= {1, 3, 4, 5, 63, 64, 65, 255, 256, 257}


def test_the_matmul_table_reaches_every_launch_path(K):
    plans = [K.matmul_vjp_variant(c["S"], c["NB"], c["M"], c["K"], c["N"], ef.matmul_wants(c)) for c in ef.MATMUL_CASES]
    assert all(p is not None for p in plans)
    # the four kernel instances (da / db x panel resident / restaged), each also with the other output null
    assert {(p["da"], p["resident_da"]) for p in plans if p["da"]} == {(True, True), (True, False)}
    assert {(p["db"], p["resident_db"]) for p in plans if p["db"]} == {(True, True), (True, False)}
    assert {(p["da"], p["db"]) for p in plans} == {(True, True), (True, False), (False, True)}
    assert {p["seed_split"] for p in plans} == {False, True} and {p["wide_index"] for p in plans} == {False, True}
    for c, p in zip(ef.MATMUL_CASES, plans):
        assert p["resident_da"] == (p["da"] and c["N"] <= ef.MM_RES_DEPTH) and p["resident_db"] == (p["db"] and c["M"] <= ef.MM_RES_DEPTH)
        assert p["wide_index"] == c["wide"]
    for dim in ("M", "K", "N"):  # every tile edge and the resident limit on each side
        assert {c[dim] for c in ef.MATMUL_CASES} >= {1, 2, 31, 32, 33, 63, 64, 65, 129}, dim
    assert {c["NB"] for c in ef.MATMUL_CASES} >= {0, 1, 3} and {c["S"] for c in ef.MATMUL_CASES} >= {1, 2, 5}
    assert any(c["N"] == 128 and c["M"] == 128 for c in ef.MATMUL_CASES)  # (the last resident depth)


def test_the_recorded_expf_constant_is_what_the_cpu_measures():
    ys = [ef.softmax_case_inputs(i)[1] for i in SMX if ef.SOFTMAX_CASES[i]["log"]]
    measured = ef.measured_exp_error(ys)
    print(f"measured exp error: {measured:.4f} u")
    assert 0.5 * ef.MEASURED_EXP_ERROR <= measured <= ef.MEASURED_EXP_ERROR and ef.C_EXP == 2 * ef.MEASURED_EXP_ERROR


@pytest.mark.parametrize("i", SMX, ids=lambda i: ef.softmax_case_id(ef.SOFTMAX_CASES[i]))
def test_the_softmax_criterion_accepts_every_order_and_rejects_the_mutants(i):
    c = ef.SOFTMAX_CASES[i]
    g, y = ef.softmax_case_inputs(i)
    ref = ef.softmax_reference(g, y, c["log"])
    orders = ef.ORDERS if c["L"] <= 260 else ("pairwise",)  # (a Python loop per element of a long row is not worth its time)
    for order in orders:
        dx = ef.softmax_math(g, y, c["log"], order)
        assert ef.softmax_violations(c, dx, ref) == [], order
        if c["kind"] != "random" and not c["log"]:  # exact zeros where the probability is zero
            assert bool((dx[:, y == 0] == 0).all()) and bool((y == 0).any())
    if c["kind"] == "saturated":
        assert bool(((y == 1).sum(-1) == 1).all()) and bool(((y == 0).sum(-1) == c["L"] - 1).all())
    if c["R"] == 0:
        return
    for mutant in ef.SOFTMAX_MUTANTS:
        applies = (mutant == "log-y-for-exp") == c["log"] and c["kind"] != "saturated" and c["L"] > 1
        if applies:
            assert ef.softmax_violations(c, ef.softmax_math(g, y, c["log"], "forward", mutant), ref), mutant


@pytest.mark.parametrize("i", MM_SMALL, ids=lambda i: ef.matmul_case_id(ef.MATMUL_CASES[i]))
def test_the_matmul_criteria_accept_every_order_and_reject_the_mutants(i):
    c = ef.MATMUL_CASES[i]
    want = ef.matmul_wants(c)
    for ints in (False, True):
        g, a, b = ef.matmul_case_inputs(i, ints)
        ref = ef.matmul_reference(g, a, b)
        for order in ef.ORDERS if c["M"] * c["N"] <= 64 * 65 else ("pairwise",):
            da, db = ef.matmul_math(g, a, b, want, order)
            assert ef.matmul_violations(c, da, db, ref, ints) == [], (order, ints)
        if c["NB"] == 0:
            continue
        if want[0] and c["K"] == c["N"] > 1:
            assert ef.matmul_violations(c, *ef.matmul_math(g, a, b, want, None, "b-untransposed"), ref, ints), "b-untransposed"
        if want[1] and c["S"] > 1:
            assert ef.matmul_violations(c, *ef.matmul_math(g, a, b, want, None, "wrong-seed"), ref, ints), "wrong-seed"


def test_the_mutants_meet_cases_that_show_them():
    assert sum(c["K"] == c["N"] > 1 and c["want"] != "db" and c["NB"] > 0 for c in ef.MATMUL_CASES) >= 2
    assert sum(c["S"] > 1 and c["want"] != "da" and c["NB"] > 0 for c in ef.MATMUL_CASES) >= 10
    assert sum(c["log"] and c["L"] > 1 for c in ef.SOFTMAX_CASES) >= 10


def test_the_emulations_state_the_rules():
    from tests.emulated_matmul_kernels import EmulatedEagerAttnKernels

    E = EmulatedEagerAttnKernels()
    i = next(i for i in SMX if ef.SOFTMAX_CASES[i]["L"] == 65 and not ef.SOFTMAX_CASES[i]["log"])
    c = ef.SOFTMAX_CASES[i]
    g, y = ef.softmax_case_inputs(i)
    dx = E.softmax_vjp(g.reshape(c["S"] * c["R"], c["L"]), y, c["S"])
    assert dx.shape == (c["S"] * c["R"], c["L"]) and ef.softmax_violations(c, dx, ef.softmax_reference(g, y, False)) == []
    E.softmax_mutant = "no-sum"
    assert ef.softmax_violations(c, E.softmax_vjp(g.reshape(c["S"] * c["R"], c["L"]), y, c["S"]), ef.softmax_reference(g, y, False))
    j = next(j for j in MM if ef.MATMUL_CASES[j]["M"] == 33)
    c = ef.MATMUL_CASES[j]
    g, a, b = ef.matmul_case_inputs(j)
    da, db = E.matmul_vjp(g.reshape(c["S"] * c["NB"], c["M"], c["N"]), a, b, c["S"])
    assert da.shape == (c["S"] * c["NB"], c["M"], c["K"]) and db.shape == (c["S"] * c["NB"], c["K"], c["N"])
    assert ef.matmul_violations(c, da, db, ef.matmul_reference(g, a, b)) == []
    assert E.seen[-1] == ("matmul_vjp", c["S"], c["NB"], c["M"], c["K"], c["N"], (True, True))
    assert E.matmul_vjp_variant(2, 3, 4, 5, 6)["da"] and E.softmax_vjp_variant(2, 3, 64)["vec"]
