"""tests/slice_fixtures.py checked on the CPU: the table of kernel cases reaches every path lk_slice_vjp_f32 can take (asked of the
library's own host-only ``lk_slice_variant``), and the reference of tests/test_gpu_slice.py tells three wrong kernels from the right
one: one that drops the zero fill, one that ignores ``c0`` and one that sums in the reverse order."""
import pytest
import torch

from tests import slice_fixtures as sf

RUN = [c for c in sf.CASES if not c["wide"]]
SMALL = [c for c in RUN if c["R"] <= 1024]


@pytest.fixture(scope="module")
def K():
    import os

    from laplace_amd._lib import LIB_PATH, HipKernels

    if not os.path.exists(LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return HipKernels()


def _variant(K, c, aligned=None):
    return K.slice_variant(sf.split_mask(c), [p[0] for p in c["pieces"]], [p[1] for p in c["pieces"]], c["R"], c["Ct"],
                           not c["off"] if aligned is None else aligned)


def _fours(c):
    return c["Ct"] % 4 == 0 and all(c0 % 4 == 0 and cs % 4 == 0 for c0, cs, _ in c["pieces"])


def _covered(c):
    return {col for c0, cs, _ in c["pieces"] for col in range(c0, c0 + cs)}


def test_the_table_reaches_every_path(K):
    seen = [(_variant(K, c), c) for c in sf.CASES]
    assert all(v is not None for v, _ in seen)
    for v, c in seen:  # what the variant reports is what was asked, and the vector path is exactly "multiples of four and aligned"
        assert v["npieces"] == len(c["pieces"]) and v["split_mask"] == sf.split_mask(c), sf.case_id(c)
        assert v["vec"] == (not c["off"] and _fours(c)), sf.case_id(c)
        assert v["wide_index"] == c["wide"], sf.case_id(c)
    run = [(v, c) for v, c in seen if not c["wide"] and c["R"] > 0]
    for vec in (True, False):
        sub = [(v, c) for v, c in run if v["vec"] == vec]
        assert {1, 2, 3, 8} <= {v["npieces"] for v, _ in sub}, vec  # one piece and eight
        assert {v["split_mask"] for v, _ in sub if v["npieces"] == 3} >= set(range(8)), vec  # every mix in a row of three
        assert any(len(_covered(c)) < c["Ct"] for _, c in sub), vec  # columns no piece covers
        assert any(sum(cs for _, cs, _ in c["pieces"]) > len(_covered(c)) for _, c in sub), vec  # overlap
        assert any(len(set(c["pieces"])) < len(c["pieces"]) for _, c in sub) or not vec  # (a piece listed twice: vector path)
        # one workgroup, several, and a grid that strides (more lanes than 2048 workgroups of 256 hold)
        blocks = {min(v["blocks"], 2) if v["blocks"] < 2048 else "full" for v, _ in sub}
        assert blocks == {1, 2, "full"}, (vec, blocks)
    strided = [(v, c) for v, c in run if v["blocks"] == 2048]
    assert len(strided) >= 2 and all(c["R"] * (c["Ct"] // 4 if v["vec"] else c["Ct"]) > sf.GRID_LANES for v, c in strided)
    assert all(c["R"] * (c["Ct"] // 4 if v["vec"] else c["Ct"]) <= sf.GRID_LANES + c["Ct"] for v, c in strided)  # (just past it)
    # the 64-bit lane index on both paths, by shape only
    assert {v["vec"] for v, c in seen if c["wide"]} == {True, False}
    # an unaligned base sends a shape of multiples of four to the scalar path
    assert any(c["off"] and _fours(c) for c in RUN)
    assert any(c["R"] == 0 for c in RUN) and any(c["cancel"] for c in RUN)
    # the smallest shapes
    tiny = [c for c in RUN if len(c["pieces"]) == 1]
    assert {c["R"] for c in tiny} >= {1, 3} and {c["Ct"] for c in tiny} >= {5, 8, 12}
    assert {c["pieces"][0][0] for c in tiny} >= {0, 1, 4}
    assert any(c["pieces"][0][:2] == (0, c["Ct"]) for c in tiny)  # (a full-width part alone)
    assert len({sf.case_id(c) for c in sf.CASES}) == len(sf.CASES)


def test_the_variant_refuses_what_the_entry_point_refuses(K):
    v = K.slice_variant
    assert v(0, [], [], 8, 8) is None and v(0, [0] * 9, [8] * 9, 8, 8) is None
    assert v(2, [0], [8], 8, 8) is None  # (a mask bit beyond the pieces)
    assert v(0, [4], [5], 8, 8) is None and v(0, [0], [0], 8, 8) is None and v(0, [-1], [4], 8, 8) is None
    assert v(0, [0], [8], -1, 8) is None and v(0, [0], [8], 1 << 37, 8) is None and v(0, [0], [1], 1, 1 << 30) is None
    assert v(0, [0], [8], (1 << 37) - 1, 8)["wide_index"]  # (2^38 lanes)
    # the largest chunk of CSPNetSmall at S = 9, B = 128: both halves and a full-width part
    assert v(5, [0, 0, 32], [64, 32, 32], 9 * 128 * 32 * 32, 64) == {"vec": True, "npieces": 3, "split_mask": 5,
                                                                      "wide_index": False, "blocks": 2048}


@pytest.mark.parametrize("c", SMALL, ids=sf.case_id)
def test_the_data_are_finite_and_the_reference_is_the_sum_of_the_covering_pieces(c):
    gen = torch.Generator().manual_seed(5 + sf.CASES.index(c))
    pieces = sf.make_pieces(c, gen)
    R, Ct = c["R"], c["Ct"]
    exact, bound = torch.zeros(R, Ct, dtype=torch.float64), torch.zeros(R, Ct, dtype=torch.float64)
    for p, c0, cs in pieces:
        v = sf.piece_value(p)
        assert v.dtype == torch.float32 and tuple(v.shape) == (R, cs) and bool(torch.isfinite(v).all())
        if not c["cancel"]:
            assert v.numel() == 0 or bool((v != v.round()).any())
            assert v.numel() == 0 or float(v.abs()[v != 0].min()) > 2.0 ** -100  # (nothing near the subnormals)
        exact[:, c0:c0 + cs] += v.double()
        bound[:, c0:c0 + cs] += v.abs().double()
    want = sf.vjp_reference(pieces, R, Ct)
    assert tuple(want.shape) == (R, Ct) and want.dtype == torch.float32
    if R:
        assert float((want.double() - exact).abs().max()) <= len(pieces) * 2.0 ** -23 * float(bound.max())
        free = sorted(set(range(Ct)) - _covered(c))
        assert bool((want[:, free] == 0).all()) and not bool(torch.signbit(want[:, free]).any())  # (+0.0 where no piece reaches)
    if c["cancel"] and R:
        first = c["pieces"][1][0]
        assert bool((want[:, first:first + 4] == 1.0).all())


def test_a_single_piece_keeps_a_negative_zero():
    p = torch.tensor([[-0.0, 1.5, -0.0]])
    want = sf.vjp_reference([(p, 1, 3)], 1, 5)
    assert torch.signbit(want).tolist() == [[False, True, False, True, False]]
    two = sf.vjp_reference([(p, 1, 3), (torch.zeros(1, 3), 1, 3)], 1, 5)
    assert not bool(torch.signbit(two).any())  # (-0.0 + 0.0 = +0.0: a sum, unlike a single piece, does not keep it)


def test_split_values_are_formed_as_split_tensor_float_forms_them():
    from laplace_amd._lib import SplitTensor

    c = next(c for c in SMALL if sf.split_mask(c) == 7 and len(c["pieces"]) == 3)
    for p, _, _ in sf.make_pieces(c, torch.Generator().manual_seed(1)):
        st = SplitTensor(torch.stack([p[0], p[1]]), torch.tensor([p[2]], dtype=torch.int32))
        assert torch.equal(st.float(), sf.piece_value(p)) and torch.equal(sf.piece_value(st), sf.piece_value(p))


def test_the_mutants_fail_the_check_of_the_table():
    """a kernel that leaves uncovered columns as they were, one that ignores c0 and one that sums in the reverse order:
    ``torch.equal`` with the reference tells all three"""
    failed = {"no-zero-fill": [], "ignore-c0": [], "reversed": []}
    for c in SMALL:
        gen = torch.Generator().manual_seed(5 + sf.CASES.index(c))
        pieces = sf.make_pieces(c, gen)
        want = sf.vjp_reference(pieces, c["R"], c["Ct"])
        for mutant in failed:
            if not torch.equal(sf.vjp_reference(pieces, c["R"], c["Ct"], mutant), want):
                failed[mutant].append(sf.case_id(c))
    live = [c for c in SMALL if c["R"] > 0]
    # every case with rows and an uncovered column catches the first; every case with rows and a piece off column 0 the second;
    # the cancellation rows the third (and nothing with fewer than three pieces over one column: a sum of two commutes)
    assert set(failed["no-zero-fill"]) == {sf.case_id(c) for c in live if len(_covered(c)) < c["Ct"]} != set()
    assert set(failed["ignore-c0"]) == {sf.case_id(c) for c in live if any(c0 for c0, _, _ in c["pieces"])} != set()
    cancel = {sf.case_id(c) for c in live if c["cancel"]}
    assert len(cancel) >= 2 and cancel <= set(failed["reversed"])
    deep = {sf.case_id(c) for c in live
            if max(sum(c0 <= col < c0 + cs for c0, cs, _ in c["pieces"]) for col in range(c["Ct"])) >= 3}
    assert set(failed["reversed"]) <= deep


def test_the_emulation_states_the_reference_and_its_mutants():
    from laplace_amd._lib import SplitTensor
    from tests.emulated_slice_kernels import EmulatedSliceKernels

    c = next(c for c in SMALL if c["cancel"] and sf.split_mask(c))
    pieces = sf.make_pieces(c, torch.Generator().manual_seed(2))
    ops = [(p if torch.is_tensor(p) else SplitTensor(torch.stack([p[0], p[1]]), torch.tensor([p[2]], dtype=torch.int32)), c0, cs)
           for p, c0, cs in pieces]
    K = EmulatedSliceKernels()
    word = torch.zeros(1)
    want = sf.vjp_reference(pieces, c["R"], c["Ct"])
    assert torch.equal(K.slice_vjp(ops, c["R"], c["Ct"], amax=word), want) and float(word) == float(want.abs().max())
    K.mutant = "reversed"
    assert not torch.equal(K.slice_vjp(ops, c["R"], c["Ct"]), want)
    src = torch.arange(15.0).reshape(3, 5)
    assert torch.equal(K.slice_forward(src, 3, 5, 1, 3), src[:, 1:4]) and K.slice_forward(src, 3, 5, 1, 3).is_contiguous()
    assert K.slice_variant(0, [0], [4], 3, 4) == {"vec": True, "npieces": 1, "split_mask": 0, "wide_index": False, "blocks": 1}
