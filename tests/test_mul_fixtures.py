"""tests/mul_fixtures.py checked on the CPU: the table of kernel cases reaches every value of every field lk_mul_variant packs (asked of
the library's own host-only query), torch fp32 math on the table passes the criteria of tests/test_gpu_mul.py, and four wrong kernels
fail them: the gate of the wrong sample, a dropped tail of a row, the two outputs swapped and a row sum accumulated in fp16."""
import pytest
import torch

from tests import mul_fixtures as mf

RUN = [c for c in mf.CASES if not c["wide"]]


@pytest.fixture(scope="module")
def K():
    import os

    from laplace_amd._lib import LIB_PATH, HipKernels

    if not os.path.exists(LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return HipKernels()


def _variant(K, c):
    return K.mul_variant(c["S"], c["R"], c["L"], c["row"], mf.wants(c), not c["off"])


def test_the_table_reaches_every_value_of_every_field(K):
    seen = [(_variant(K, c), c) for c in mf.CASES]
    assert all(v is not None for v, _ in seen)
    for v, c in seen:  # what the variant reports is what was asked
        assert v["row"] == c["row"] and (v["da"], v["db"]) == mf.wants(c), mf.case_id(c)
        assert v["vec"] == (not c["off"] and c["L"] % 4 == 0), mf.case_id(c)
        assert v["wide_index"] == c["wide"] == (c["S"] * c["R"] * c["L"] >= 1 << 31), mf.case_id(c)
        nvec = c["L"] // 4 if v["vec"] else c["L"]
        if c["row"]:
            assert v["lanes_per_row"] == min(64, 1 << (nvec - 1).bit_length()), mf.case_id(c)
            assert v["resident"] == (nvec <= mf.RESIDENT_VECTORS), mf.case_id(c)
        else:
            assert v["lanes_per_row"] == 1 and v["resident"], mf.case_id(c)
    run = [(v, c) for v, c in seen if not c["wide"] and c["R"] > 0]
    for row in (True, False):
        for vec in (True, False):
            sub = [(v, c) for v, c in run if v["row"] == row and v["vec"] == vec]
            assert {(v["da"], v["db"]) for v, _ in sub} == {(True, True), (True, False), (False, True)}, (row, vec)
            assert {v["seed_split"] for v, _ in sub} == {True, False}, (row, vec)
            # one workgroup, several, and a grid that strides
            assert {min(v["blocks"], 2) if v["blocks"] < mf.MAX_BLOCKS else "full" for v, _ in sub} == {1, 2, "full"}, (row, vec)
            if row:
                assert {v["resident"] for v, _ in sub} == {True, False}, vec
                past = min(c["L"] // (4 if vec else 1) for v, c in sub if not v["resident"])
                assert past == mf.RESIDENT_VECTORS + 1, vec  # (one vector past the limit)
                assert any(v["resident"] and c["L"] // (4 if vec else 1) > 64 for v, c in sub), vec  # more than one vector per lane
    assert {v["lanes_per_row"] for v, c in run if c["row"]} == {1, 2, 4, 8, 16, 32, 64}
    # the grid strides by one row / one vector only: the last stride holds a single live group
    for v, c in run:
        if v["blocks"] == mf.MAX_BLOCKS:
            units = c["R"] if c["row"] else c["R"] * c["L"] // (4 if v["vec"] else 1)
            per = 256 // v["lanes_per_row"] if c["row"] else 256
            assert mf.MAX_BLOCKS * per < units <= mf.MAX_BLOCKS * per + per, mf.case_id(c)
    assert {(c["row"], v["vec"]) for v, c in seen if c["wide"]} >= {(True, True), (False, True), (True, False)}
    # the L and R and S of the list; an unaligned base on a multiple of four; no rows; rows that do not fill a workgroup
    assert {c["L"] for c in RUN if c["row"]} >= {1, 3, 4, 49, 64, 256, 260} and {c["L"] for c in RUN if not c["row"]} >= {1, 3, 4, 49, 64, 260}
    assert max(c["L"] for c in RUN) == 4096 and {c["R"] for c in RUN} >= {0, 1, 5} and {c["S"] for c in RUN} == {1, 3, 9}
    assert any(c["off"] and c["L"] % 4 == 0 and c["row"] for c in RUN) and any(c["off"] and c["L"] % 4 == 0 and not c["row"] for c in RUN)
    assert any(c["row"] and c["R"] % (256 // v["lanes_per_row"]) for v, c in run if v["blocks"] < mf.MAX_BLOCKS and c["R"] > 5)
    assert len({mf.case_id(c) for c in mf.CASES}) == len(mf.CASES)


def test_the_variant_refuses_what_the_entry_point_refuses(K):
    v = K.mul_variant
    assert v(0, 4, 8, 1) is None and v(1, -1, 8, 1) is None and v(1, 4, 0, 1) is None and v(1, 4, 1 << 30, 1) is None
    assert v(1, 4, 8, 2) is None and v(1, 4, 8, -1) is None and v(1, 4, 8, 1, (False, False)) is None
    assert v(1 << 10, 1 << 20, 1 << 10, 0) is None and v((1 << 10) - 1, 1 << 20, 1 << 10, 0)["wide_index"]
    assert v(1, 0, 8, 1) == {"row": True, "vec": True, "lanes_per_row": 2, "resident": True, "seed_split": False, "wide_index": False,
                             "da": True, "db": True, "blocks": 0}
    # the gates of SEResNetSmall and the gated feed-forward of ViTSwiGLU at S = 9, B = 128
    assert v(9, 128 * 32, 32 * 32, 1) == {"row": True, "vec": True, "lanes_per_row": 64, "resident": True, "seed_split": False,
                                          "wide_index": False, "da": True, "db": True, "blocks": 1024}
    assert v(9, 128 * 128, 8 * 8, 1)["lanes_per_row"] == 16
    assert v(9, 128, 64 * 512, 0) == {"row": False, "vec": True, "lanes_per_row": 1, "resident": True, "seed_split": False,
                                      "wide_index": False, "da": True, "db": True, "blocks": 2048}


def _inputs(c):
    return mf.make_inputs(c, torch.Generator().manual_seed(7 + mf.CASES.index(c)))


@pytest.mark.parametrize("c", RUN, ids=mf.case_id)
def test_the_data_are_full_mantissa_and_torch_math_passes_the_criteria(c):
    g, a, b = _inputs(c)
    for t in (g, a, b):
        assert t.dtype == torch.float32 and bool(torch.isfinite(t).all())
        if t.numel():
            assert 2.0 ** -10 <= float(t.abs().min()) and float(t.abs().max()) < 2.0 ** 10
        if t.numel() >= 64:
            assert bool((t < 0).any()) and bool((t > 0).any())
            assert bool((t.view(torch.int32) & 1).bool().any())  # (the last mantissa bit is in use)
    ref = mf.vjp_reference(g, a, b, c["row"])
    assert ref["da"].dtype == torch.float64 and tuple(ref["da"].shape) == (c["S"], c["R"], c["L"])
    assert tuple(ref["db"].shape) == ((c["S"], c["R"]) if c["row"] else (c["S"], c["R"], c["L"]))
    if g.numel():
        assert float(ref["da"].abs().min()) >= 2.0 ** -20  # (no product underflows)
    da, db = mf.torch_math(g, a, b, c["row"], mf.wants(c))
    assert mf.violations(c, da, db, ref) == []
    # the reference itself, rounded once, is inside the bound
    want_da, want_db = mf.wants(c)
    assert mf.violations(c, ref["da"].float() if want_da else None, ref["db"].float() if want_db else None, ref) == []


def test_the_criteria_notice_a_missing_or_an_unasked_output():
    c = next(c for c in RUN if c["want"] == "da" and c["R"])
    g, a, b = _inputs(c)
    ref = mf.vjp_reference(g, a, b, c["row"])
    da, db = mf.torch_math(g, a, b, c["row"])
    assert mf.violations(c, da, db, ref) and mf.violations(c, None, None, ref) and not mf.violations(c, da, None, ref)


def test_the_mutants_fail_the_criteria_of_the_table():
    failed = {m: set() for m in mf.MUTANTS}
    for c in RUN:
        g, a, b = _inputs(c)
        ref = mf.vjp_reference(g, a, b, c["row"])
        for m in failed:
            if mf.violations(c, *mf.torch_math(g, a, b, c["row"], mf.wants(c), m), ref):
                failed[m].add(mf.case_id(c))
    live = [c for c in RUN if c["R"] > 0]
    ids = lambda cases: {mf.case_id(c) for c in cases}  # noqa: E731
    # the gate of another sample: wherever there is more than one seed and more than one row, and da is asked for
    assert failed["wrong-sample"] == ids(c for c in live if c["S"] > 1 and c["R"] > 1 and mf.wants(c)[0]) != set()
    # the tail of a row: every L that is no multiple of four - by the NaN it leaves in an element-wise output; a row sum ALONE
    # shows it where the dropped products are not lost in the bound of a long row (L = 49 is caught, one element of 513 need not be)
    ragged = ids(c for c in live if c["L"] % 4)
    assert failed["dropped-tail"] <= ragged and ragged - failed["dropped-tail"] <= ids(c for c in live if c["row"] and c["want"] == "db")
    assert ids(c for c in live if c["row"] and c["want"] == "db" and c["L"] == 49) <= failed["dropped-tail"]
    # the outputs swapped: every full-form case
    assert failed["swapped"] == ids(c for c in live if not c["row"]) != set()
    # the fp16 accumulator: every row sum
    assert failed["fp16-sum"] == ids(c for c in live if c["row"] and mf.wants(c)[1]) != set()


def test_the_emulation_states_the_rule_and_its_mutants():
    from tests.emulated_mul_kernels import EmulatedMulKernels

    K = EmulatedMulKernels()
    for c in (next(c for c in RUN if c["row"] and c["L"] == 49 and c["want"] == "both"),
              next(c for c in RUN if not c["row"] and c["L"] == 49 and c["want"] == "db")):
        g, a, b = _inputs(c)
        ref = mf.vjp_reference(g, a, b, c["row"])
        S, R, L = g.shape
        da, db = K.mul_vjp(g.reshape(S * R, L), a, b, S, c["row"], mf.wants(c))
        assert (da is None) == (c["want"] == "db") and tuple(db.shape) == ((S * R,) if c["row"] else (S * R, L))
        assert mf.violations(c, da, db, ref) == []
        assert K.seen[-1] == ("mul_vjp", "row" if c["row"] else "full", S, R, L, mf.wants(c))
        K.mutant = "dropped-tail"
        assert mf.violations(c, *K.mul_vjp(g.reshape(S * R, L), a, b, S, c["row"], mf.wants(c)), ref)
        K.mutant = None
    assert K.mul_variant(3, 5, 49, True, aligned=False)["lanes_per_row"] == 64
