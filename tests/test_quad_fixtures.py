"""The table of tests/quad_fixtures.py reaches EVERY instantiation of the weight-sharing predictive kernels, and its inputs
leave room under the tolerance (CPU only: ``lk_quadform_shared_variant`` is a pure host function of the built library, the
kernels are stood in for by tests/emulated_kernels.py).

A threshold that moves in a launcher (6144 / 10240 eigenvalue floats, ``L == 16``, ``L % 4``, the alignment test, the
class tiles, the splits) moves the query's answer with it — both call the same helpers of csrc/lk_quadtile.h — and fails
here instead of silently un-covering a kernel in tests/test_gpu_quadform_instances.py."""
import itertools
import os

import pytest
import torch

from tests import quad_fixtures as qf
from tests.emulated_kernels import EmulatedKernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def K():
    from laplace_amd._lib import LIB_PATH, HipKernels

    if not os.path.exists(LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return HipKernels()


def shapes(row):
    """(B, L, aligned16) of every launch shape of a row"""
    return [(B, L, True) for B in row["Bs"] for L in row["Ls"]] + [(B, L, False) for B in row["Bs"] for L in row.get("offset_Ls", ())]


def queried(K, family):
    for row in qf.CASES[family]:
        for B, L, aligned in shapes(row):
            var = K.quadform_shared_variant(qf.row_form(row), B, row["C"], row["Do"], row["Dk"], L, aligned)
            assert var is not None, (qf.row_id(row), B, L)
            yield row, B, L, var


def test_query_refuses_what_the_forms_do_not_serve(K):
    q = K.quadform_shared_variant
    assert q(qf.QF_KRON, 3, 10, 33, 135, 9) == {"ct": 10, "arith": 0, "split": 4}
    assert q(qf.QF_KRON, 3, 10, 33, 135, 16, aligned16=False)["arith"] == 0
    assert q(qf.QF_KRON, 3, 11, 33, 135, 9) is None and q(qf.QF_DIAG_GGN, 3, 11, 33, 135, 9) is None
    assert q(qf.QF_GRID, 3, 11, 33, 135, 9)["ct"] == 10  # (blocks of outputs: any C)
    assert q(qf.QF_PLANES, 3, 10, 33, 135, 16) is None and q(qf.QF_PLANES, 3, 10, 32, 135, 24) is None
    assert q(qf.QF_KRON, 0, 1, 1, 1, 1) is None and q(qf.QF_KRON, 1, 1, 1, 1, 0) is None and q(6, 1, 1, 1, 1, 1) is None
    assert q(-1, 1, 1, 1, 1, 1) is None
    # the thresholds of the planes form, on both sides (eigenvalue floats Do + Dk: 6144 two per CU, 10240 in LDS)
    assert q(qf.QF_PLANES, 3, 10, 32, 6112, 32) == {"ct": 10, "split": 48, "occ": 2, "sub": False, "w_in_lds": True}
    assert q(qf.QF_PLANES, 3, 10, 32, 6113, 32)["occ"] == 1
    assert q(qf.QF_PLANES, 3, 10, 32, 10208, 32)["w_in_lds"] and not q(qf.QF_PLANES, 3, 10, 32, 10209, 32)["w_in_lds"]
    assert q(qf.QF_PLANES, 3, 10, 32, 6112, 16)["sub"] and not q(qf.QF_PLANES, 3, 10, 32, 6113, 16)["sub"]


@pytest.mark.parametrize("family", ["planes", "fp32", "diag_ggn", "grid"])
def test_every_row_selects_the_variant_its_name_promises(K, family):
    n = 0
    for row, B, L, var in queried(K, family):
        what = (qf.row_id(row), B, L, var)
        tiles = qf.GRID_CLASS_TILES if family == "grid" else qf.CLASS_TILES
        assert var["ct"] == qf.class_tile(min(row["C"], tiles[-1]), tiles), what
        if family == "planes":
            assert {k: var[k] for k in ("occ", "sub", "w_in_lds")} == qf.planes_expectation(row), what
        else:
            assert var["arith"] == row["arith"], what
        nt = qf.ntiles(row["Do"], row["Dk"])
        assert 1 <= var["split"] <= (B if family == "diag_ggn" else nt), what
        if row.get("stream"):
            assert max(qf.planes_chunk_counts(row["Do"], row["Dk"], L, var["split"])) >= 2 * (L // 16) and L > 16, what
        if row.get("multitile"):
            assert nt > var["split"], what
        if row.get("manysamples"):
            assert B > var["split"], what
        n += 1
    assert n >= len(qf.CASES[family])


def test_the_table_reaches_every_planes_instantiation(K):
    got = {(var["ct"], var["occ"], var["sub"], var["w_in_lds"]) for _, _, _, var in queried(K, "planes")}
    want = {(ct, *v) for ct in qf.CLASS_TILES for v in ((2, False, True), (2, True, True), (1, False, True), (1, False, False))}
    assert got == want, (sorted(want - got), sorted(got - want))


def test_the_table_reaches_every_fp32_instantiation(K):
    got = {(var["ct"], var["arith"], row["route"]) for row, _, _, var in queried(K, "fp32")}
    want = set(itertools.product(qf.CLASS_TILES, (0, 1), ("kron", "kron-seedmajor", "diag")))
    assert got == want, (sorted(want - got), sorted(got - want))
    # ARITH 0 is reached both ways: positions that are no whole float4s, and a misaligned operand
    ways = {(L % 4 == 0, aligned) for row in qf.CASES["fp32"] if row["arith"] == 0 for _, L, aligned in shapes(row)}
    assert ways == {(False, True), (True, False)}


def test_the_table_reaches_every_diag_ggn_instantiation(K):
    got = {(var["ct"], var["arith"]) for _, _, _, var in queried(K, "diag_ggn")}
    assert got == set(itertools.product(qf.CLASS_TILES, (0, 1)))


def test_the_table_reaches_every_grid_instantiation(K):
    got = {(var["ct"], row["mode"], var["arith"]) for row, _, _, var in queried(K, "grid")}
    assert got == set(itertools.product(qf.GRID_CLASS_TILES, (0, 1, 2), (0, 1)))
    assert {row["seed_major"] for row in qf.CASES["grid"]} == {False, True}
    assert any(row["C"] > 10 and row["C"] % 10 for row in qf.CASES["grid"])  # a short second block of outputs


def test_the_table_holds_the_structural_cases(K):
    """by property, from the split the query returns: the ring's prologue / tail on both sides of its depth, chunk streams
    across tiles, walks over several tiles, several samples per workgroup"""
    seen = {2: set(), 4: set(), 6: set()}
    stream = False
    for row, B, L, var in queried(K, "planes"):
        NS = qf.planes_ring_depth(var)
        for Q in qf.planes_chunk_counts(row["Do"], row["Dk"], L, var["split"]):
            assert Q >= 1  # (split <= ntiles: no workgroup is idle, so Q < NS - 1 does not exist for the two-stage ring)
            seen[NS].add("below" if Q < NS - 1 else "at" if Q == NS - 1 else "above" if Q > NS else "between")
        my_tiles = -(-qf.ntiles(row["Do"], row["Dk"]) // var["split"])
        stream |= my_tiles >= 2 and L > 16
    assert seen[2] >= {"at", "above"} and "below" not in seen[2], seen
    assert seen[4] >= {"below", "at", "above"} and seen[6] >= {"below", "at", "above"}, seen
    assert stream
    assert any(qf.ntiles(r["Do"], r["Dk"]) > v["split"] for r, _, _, v in queried(K, "fp32"))
    assert {v["arith"] for r, _, _, v in queried(K, "fp32") if qf.ntiles(r["Do"], r["Dk"]) > v["split"]} == {0, 1}
    assert any(qf.ntiles(r["Do"], r["Dk"]) > v["split"] for r, _, _, v in queried(K, "grid"))
    assert {v["arith"] for r, B, _, v in queried(K, "diag_ggn") if B > v["split"]} == {0, 1}
    # the XCD remap of the quadratic-form kernels (gridDim % (8 split) == 0) is on in some launches and off in others
    remap = {(B * v["split"]) % (8 * v["split"]) == 0 for _, B, _, v in queried(K, "planes")}
    assert remap == {False, True}


def test_linear_grid_rows_walk_the_grid_in_pieces_and_raise_the_lds_limit():
    """lk_quadform_linear_grid_f32 stages v^2 [4][Di] and S [4][GS][Do] floats: GS = what fits in 64 KiB beside v^2 (restated
    here from the launcher's comment; there is one instantiation per mode and no query for it)"""
    G = qf.DELTAS.numel()
    kinds = set()
    for row in qf.CASES["linear_grid"]:
        fixed, per_g = 16 * row["Dk"], 16 * row["Do"]
        GS = min(G, max(1, (65536 - fixed) // per_g)) if fixed < 65536 else 1
        kinds.add((row["mode"], row["bias"], "pieces" if 1 < GS < G else "bigLDS" if fixed + GS * per_g > 65536 else "whole"))
    assert kinds == set(itertools.product((0, 1, 2), (False, True), ("pieces", "bigLDS")))


def test_reference_pair_sums_are_all_large():
    """correlated, differently scaled outputs: every off-diagonal entry is of the size of the diagonal ones it couples"""
    ops = qf.operands(10, 3, 32, 160, 32, seed=7, spectrum="kfac")
    want = qf.reference_fvar(ops.u, ops.v, qf.kron_weights(ops.l1, ops.l2, ops.delta))
    d = torch.diagonal(want, dim1=1, dim2=2)
    ratio = want / torch.sqrt(d[:, :, None] * d[:, None, :])
    assert ratio.min().item() > 0.1  # (0.36 in expectation: 0.6^2 of shared variance)
    assert torch.unique(torch.triu(want[0]).flatten()).numel() == 55 + 1  # every pair sum is its own number
    # ... so a swapped pair index, or one off-diagonal entry dropped, is far outside the tolerance
    swapped = want.clone()
    swapped[:, 0, 1], swapped[:, 0, 2] = want[:, 0, 2], want[:, 0, 1]
    assert qf.tolerance_ratio(swapped, want, 2) > 1e3 and qf.tolerance_ratio(want, want, 2) == 0.0
    smallest = want.clone()
    smallest[0, 0, 1] *= 1 + 3e-4  # (the smallest sample's smallest coupling: element-wise, not against the batch's maximum)
    assert qf.tolerance_ratio(smallest, want, 2) > 1.0


# ---- the inputs leave room: the emulated kernels (same operand splits, fp32 sums) against the fp64 reference -----------------
def _emulated(row, B, L, spectrum):
    """the row's operands; of a many-sample row of a per-sample output every 8th sample (the same five decades of
    magnitudes: what the device walks in full takes the CPU a minute)"""
    ops = qf.operands(row["C"], B, row["Do"], row["Dk"], L, qf.row_seed(row), spectrum)
    if B > 48 and row["family"] != "diag_ggn":
        ops.u, ops.v = ops.u[:, ::8].contiguous(), ops.v[::8].contiguous()
    return ops


def _sample_chunks(ops, nb=48):
    B = ops.v.shape[0]
    for n0 in range(0, B, nb):
        d = dict(vars(ops))
        d["u"], d["v"] = ops.u[:, n0:n0 + nb].contiguous(), ops.v[n0:n0 + nb].contiguous()
        yield n0, type(ops)(**d)


FAMILY_VARIANTS = sorted({(f, r["variant"]) for f, rows in qf.CASES.items() for r in rows})


@pytest.mark.parametrize("family,variant", FAMILY_VARIANTS, ids=[f"{f}-{v}" for f, v in FAMILY_VARIANTS])
def test_inputs_leave_room_under_the_tolerance(family, variant):
    """every row (at its first batch size and longest map, both spectra) through the CPU emulation of its kernel"""
    E = EmulatedKernels()
    worst = 0.0
    for row in (r for r in qf.CASES[family] if r["variant"] == variant):
        B, L = row["Bs"][0], row["Ls"][-1]
        for spectrum in qf.SPECTRA:
            if family == "linear_grid":
                from tests.test_prior_grid import GridKernels

                ops = qf.linear_operands(row["C"], B, row["Do"], row["Dk"], qf.row_seed(row), spectrum)
                got = qf.run_linear_grid(GridKernels(), ops, row["mode"], row["bias"], qf.DELTAS)
                W = qf.grid_weights(row["mode"], ops.l1, ops.l2, qf.DELTAS)
                want = qf.reference_linear_grid_var(ops.u, ops.v, W, *((ops.ub, ops.wb, qf.DELTAS) if row["bias"] else ()))
                worst = max(worst, qf.tolerance_ratio(got, want, 1))
                continue
            ops = _emulated(row, B, L, spectrum)
            if family == "planes":
                want = qf.reference_fvar(ops.u, ops.v, qf.kron_weights(ops.l1, ops.l2, ops.delta))
                for per_image in (True, False):
                    got = torch.cat([qf.run_planes(E, part, per_image) for _, part in _sample_chunks(ops)])
                    worst = max(worst, qf.tolerance_ratio(got, want, 2))
            elif family == "fp32":
                w = ops.var_w.double() if row["route"] == "diag" else qf.kron_weights(ops.l1, ops.l2, ops.delta)
                want = qf.reference_fvar(ops.u, ops.v, w)
                got = torch.cat([qf.run_fp32(E, part, row["route"]) for _, part in _sample_chunks(ops)])
                worst = max(worst, qf.tolerance_ratio(got, want, 2))
            elif family == "diag_ggn":
                want = qf.reference_diag_ggn(ops.u, ops.v)
                h = torch.zeros(row["Do"] * row["Dk"])
                for _, part in _sample_chunks(ops):
                    qf.run_diag_ggn(E, part, 1.0, h)
                worst = max(worst, qf.tolerance_ratio(h, want, 1))
            else:
                from tests.test_prior_grid import GridKernels

                want = qf.reference_grid_var(ops.u, ops.v, qf.grid_weights(row["mode"], ops.l1, ops.l2, qf.DELTAS))
                got = torch.cat([qf.run_grid(GridKernels(), part, row["mode"], row["seed_major"], qf.DELTAS)
                                 for _, part in _sample_chunks(ops)], dim=1)
                worst = max(worst, qf.tolerance_ratio(got, want, 1))
    print(f"{family}-{variant}: worst |err| / tolerance of the emulation = {worst:.3g}")
    assert worst <= 1.0, worst
