"""The case table and the references of the static separable resampling rule hold what they claim (CPU): every operation of the
table IS separable (the condition the rule stands on), the transposed tap lists are exactly the transposes of the axis matrices,
the fp32 tables are torch's own fp32 operator, the table reaches every path of csrc/lk_resample.hip, three mutants of the emulation
fail the stated reference, and the end-to-end fixtures keep their ReLUs clear of a near tie."""
import pytest
import torch

from laplace_amd._lib import HipKernels
from tests import resample_fixtures as rf
from tests.emulated_resample_kernels import EmulatedResampleKernels

SMALL = [c for c in rf.runnable() if c["H"] * c["W"] <= 256]
IDS = [rf.case_id(c) for c in SMALL]


def test_the_table_names_its_cases_once():
    ids = [rf.case_id(c) for c in rf.CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("c", SMALL, ids=IDS)
def test_every_operation_is_separable_in_fp64(c):
    """the CONDITION of the rule, not a measurement: ``Mh (x) Mw`` equals the dense operator built from the full ``H W`` basis of
    torch's operation to 1e-12 (nearest-exact included: a mode that failed this would have to be refused by name)"""
    t = rf.tables(c, torch.float64)
    D = rf.dense_operator(c, torch.float64)
    assert (torch.kron(t.Mh, t.Mw) - D).abs().max().item() <= 1e-12


@pytest.mark.parametrize("c", rf.runnable(), ids=[rf.case_id(c) for c in rf.runnable()])
def test_the_tap_lists_are_the_transposes_with_ascending_indices_inside_the_cap(c):
    t = rf.tables(c)
    OH, OW = rf.out_extent(c)
    for M, axis, OL in ((t.Mh, t.csr_h, OH), (t.Mw, t.csr_w, OW)):
        ptr, idx, w = axis
        assert ptr.dtype == idx.dtype == torch.int32 and w.dtype == torch.float32
        assert torch.equal(rf.dense_transposed(axis, OL), M.t().double())  # (exactly: no tap lost, none invented)
        assert int(ptr[0]) == 0 and int(ptr[-1]) == idx.numel() == w.numel() == int((M != 0).sum())
        for l in range(min(M.shape[1], 64)):
            own = idx[int(ptr[l]):int(ptr[l + 1])]
            assert bool((own[1:] > own[:-1]).all())
    assert max(t.taps) <= rf.CAP and t.taps == (int(rf.tap_counts(t.csr_h).max()), int(rf.tap_counts(t.csr_w).max()))
    K = EmulatedResampleKernels()
    K.resample_pack(*t.csr_h, c["H"], OH), K.resample_pack(*t.csr_w, c["W"], OW)  # (the wrapper's validation passes)


@pytest.mark.parametrize("c", SMALL, ids=IDS)
def test_the_fp32_tables_are_torchs_fp32_operator_on_the_basis(c):
    """each axis matrix against torch's fp32 operator on the FULL ``H W`` basis (another derivation than the per-axis one the tables
    come from): bit-equal where the other axis holds a weight of exactly 1 to read it through; where it holds none (area, the
    antialias filters) the operator's entry is a rounded product of two weights, and is held to that one rounding, ``2^-23``"""
    t = rf.tables(c)
    H, W = c["H"], c["W"]
    OH, OW = rf.out_extent(c)
    D = rf.dense_operator(c, torch.float32).reshape(OH, OW, H, W)
    if c["k"] == 1:
        assert torch.equal(D[0, :, 0, :], t.Mw) and torch.equal(t.Mh, torch.ones(1, 1))
        return
    for M, other, pick in ((t.Mh, t.Mw, lambda o, l: D[:, o, :, l]), (t.Mw, t.Mh, lambda o, l: D[o, :, l, :])):
        ones = (other == 1).nonzero()
        if ones.numel():
            assert any(torch.equal(pick(int(o), int(l)), M) for o, l in ones.tolist())
        else:
            o, l = (int(v) for v in (other == other.max()).nonzero()[0])
            want = M.double() * float(other[o, l])
            assert bool(((pick(o, l).double() - want).abs() <= 2.0 ** -23 * want.abs()).all())


def test_the_table_reaches_every_path_of_the_kernel():
    """paths that small shapes cannot reach on a device (the 64-bit lane index) are reached through the variant function alone"""
    K = HipKernels()
    seen = []
    for c in rf.CASES:
        OH, OW = rf.out_extent(c)
        taps = (1, 1) if c["huge"] else rf.tables(c).taps
        v = K.resample_variant(c["P"], OH, OW, c["H"], c["W"], *taps, aligned=c["off"] % 4 == 0)
        assert v is not None, rf.case_id(c)
        assert v["vec"] == (c["W"] % 4 == 0 and c["off"] % 4 == 0)
        assert v["taps_in_registers"] == (max(taps) <= 4)
        seen.append((v, c["huge"]))
    for key in ("vec", "taps_in_registers", "plane_split", "grid_stride", "packed_slices", "wide_index"):
        assert {v[key] for v, _ in seen} == {False, True}, key
    on_device = [v for v, huge in seen if not huge]
    for key in ("vec", "taps_in_registers", "plane_split", "grid_stride", "packed_slices"):
        assert {v[key] for v in on_device} == {False, True}, key
    assert not any(v["wide_index"] for v in on_device) and all(v["wide_index"] for v, huge in seen if huge)
    assert any(v["vec"] and not v["taps_in_registers"] for v in on_device) and any(not v["vec"] and not v["taps_in_registers"] for v in on_device)
    assert all(v["blocks"] <= 2048 for v, _ in seen)
    # the cap itself, and what the entry point refuses
    assert K.resample_variant(1, 4, 4, 2, 2, rf.CAP, rf.CAP) is not None
    assert K.resample_variant(1, 4, 4, 2, 2, rf.CAP + 1, 1) is None and K.resample_variant(1, 4, 4, 2, 2, 1, rf.CAP + 1) is None
    assert K.resample_variant(0, 4, 4, 2, 2, 1, 1) is None and K.resample_variant(1, 1 << 30, 1, 1, 1, 1, 1) is None
    assert K.resample_variant(1 << 20, 1 << 10, 1 << 10, 2, 2, 1, 1) is None  # P * OH * OW = 2^40
    over = rf.tables(rf.OVER_CAP)
    assert max(over.taps) == rf.CAP + 1


def _run(K, c, t, g):
    OH, OW = rf.out_extent(c)
    return K.resample_vjp(g, K.resample_pack(*t.csr_h, c["H"], OH), K.resample_pack(*t.csr_w, c["W"], OW))


def _holds(dx, ref, bound, untapped):
    ok = bool(((dx.double() - ref).abs() <= bound).all()) and not bool(torch.isnan(dx).any())
    zeros = dx[untapped.expand_as(dx)]
    return ok and bool((zeros == 0).all()) and not bool(torch.signbit(zeros).any())


@pytest.mark.parametrize("c", SMALL, ids=IDS)
def test_the_emulation_meets_the_reference_and_writes_every_element(c):
    t, gen = rf.tables(c), torch.Generator().manual_seed(1)
    g = rf.make_g(c, gen)
    OH, OW = rf.out_extent(c)
    K = EmulatedResampleKernels()
    dx = _run(K, c, t, g)
    ref, bound, untapped = rf.vjp_reference(g, t.csr_h, t.csr_w)
    assert _holds(dx, ref, bound, untapped)
    # ... and the reference is the VJP of torch's operation: one autograd pass
    x = torch.zeros(c["P"], 1, *((c["W"],) if c["k"] == 1 else (c["H"], c["W"])), dtype=torch.float64, requires_grad=True)
    y = rf.apply(c, x)
    y.backward(g.double().reshape(y.shape))
    assert (x.grad.reshape(ref.shape) - ref).abs().max().item() <= 1e-6 * max(ref.abs().max().item(), 1.0)


def test_three_mutants_fail_the_stated_reference():
    gen = torch.Generator().manual_seed(2)
    # a dropped clamped edge tap: bilinear x2 and the replicate pad read their border input through more than one output
    for c in (rf.CASES[1], next(c for c in rf.CASES if c["kw"].get("mode") == "replicate")):
        t, g = rf.tables(c), rf.make_g(c, gen)
        ref, bound, untapped = rf.vjp_reference(g, t.csr_h, t.csr_w)
        K = EmulatedResampleKernels()
        assert _holds(_run(K, c, t, g), ref, bound, untapped)
        K.mutant = "drop-edge"
        assert not _holds(_run(K, c, t, g), ref, bound, untapped)
    # align_corners swapped: the tables of the other convention
    c = rf.CASES[1]
    assert c["kw"]["align_corners"] is False
    t, g = rf.tables(c), rf.make_g(c, gen)
    ref, bound, untapped = rf.vjp_reference(g, t.csr_h, t.csr_w)
    assert not _holds(_run(EmulatedResampleKernels(), c, rf.tables(c, align_corners=True), g), ref, bound, untapped)
    # a skipped zero write for an untapped input: the cropped border keeps the NaN the output was filled with
    c = next(c for c in rf.CASES if c["op"] == "pad" and min(c["kw"]["pad"]) < 0)
    t, g = rf.tables(c), rf.make_g(c, gen)
    ref, bound, untapped = rf.vjp_reference(g, t.csr_h, t.csr_w)
    assert bool(untapped.any())
    K = EmulatedResampleKernels()
    assert _holds(_run(K, c, t, g), ref, bound, untapped)
    K.mutant = "no-zero"
    assert not _holds(_run(K, c, t, g), ref, bound, untapped)


def test_the_wrapper_validates_the_tables_once():
    from laplace_amd._lib import LaplaceHipError

    K = EmulatedResampleKernels()
    c = rf.CASES[1]
    ptr, idx, w = rf.tables(c).csr_w
    OW = rf.out_extent(c)[1]
    K.resample_pack(ptr, idx, w, c["W"], OW)
    bad = idx.clone()
    bad[0] = OW
    with pytest.raises(LaplaceHipError, match="idx must lie in"):
        K.resample_pack(ptr, bad, w, c["W"], OW)
    bad = idx.clone()
    bad[:2] = bad[:2].flip(0)
    with pytest.raises(LaplaceHipError, match="ascend"):
        K.resample_pack(ptr, bad, w, c["W"], OW)
    bad = ptr.clone()
    bad[-1] -= 1
    with pytest.raises(LaplaceHipError, match="ptr must rise"):
        K.resample_pack(bad, idx, w, c["W"], OW)
    with pytest.raises(LaplaceHipError, match="are no tap lists"):
        K.resample_pack(ptr[:-1], idx, w, c["W"], OW)
    over = rf.tables(rf.OVER_CAP)
    with pytest.raises(LaplaceHipError, match="exceed LK_RESAMPLE_MAX_TAPS"):
        K.resample_pack(*over.csr_w, rf.OVER_CAP["W"], rf.out_extent(rf.OVER_CAP)[1])
    at_cap = next(c for c in rf.CASES if c["kw"].get("scale_factor") == rf.CAP and c["k"] == 1)
    assert K.resample_pack(*rf.tables(at_cap).csr_w, at_cap["W"], rf.out_extent(at_cap)[1])[5] == rf.CAP


@pytest.mark.parametrize("name", sorted(rf.FIXTURES))
def test_the_end_to_end_fixtures_keep_their_relus_clear_of_near_ties(name):
    fixture = rf.FIXTURES[name]()
    gap = rf.relu_gap(fixture)
    assert gap > rf.GAP, f"a ReLU pre-activation lies {gap:.2e} of the map's maximum from zero"
    assert sum(isinstance(m, torch.nn.ReLU) for m in fixture[0].modules()) >= 3
    again = rf.FIXTURES[name]()
    assert torch.equal(again[2], fixture[2]) and all(torch.equal(a, b) for a, b in zip(again[0].state_dict().values(), fixture[0].state_dict().values()))
