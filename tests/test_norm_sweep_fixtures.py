"""The shape table of tests/test_gpu_norm_sweep.py, checked WITHOUT a device:

* through ``lk_norm_sweep_variant`` (pure host code of csrc/lk_normvjp.hip) the table reaches every kernel, load width, on-chip /
  two-pass path, lane count and seed-split decision that the function returns over a wide scan of shapes, for both layouts;
* the error bounds of the kernel test hold for an fp32 mean-shifted two-pass forward, for torch's own ``layer_norm`` and for the
  fp32 VJP formula, and a forward with ``var = E[x^2] - mu^2`` FAILS them at N = 3 and 4 with mean 100 - the mutant the bound
  exists to catch.
"""
import itertools
import os

import pytest
import torch

from tests import norm_sweep_fixtures as nf


@pytest.fixture(scope="module")
def variant():
    from laplace_amd._lib import LIB_PATH, HipKernels

    if not os.path.exists(LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    K = HipKernels()
    return lambda c, aligned=None: K.norm_sweep_variant(c["S"], c["B"], c["L"], c["Ch"], c["G"], c["layout"],
                                                        (c.get("off", 0) == 0) if aligned is None else aligned)


def test_constants_are_the_kernels():
    k = nf.kernel_constants()
    assert (k["NVJP_SC"], k["NVJP_NV"], k["NVJP_WIDE"], k["NVJP_TILE_LANES"]) == (nf.NVJP_SC, nf.NVJP_NV, nf.NVJP_WIDE,
                                                                                  nf.NVJP_TILE_LANES)


def _keys(v, S):
    path = (v["layout"], v["kernel"], v["vec"], v["two_pass"])
    return path + (v["lanes"],), (path + (v["seed_split"],) if S > 1 else None)


def test_table_reaches_every_variant_of_both_layouts(variant):
    """universe: every (layout, kernel, vec, two-pass, lanes) and every (layout, kernel, vec, two-pass, seed-split at S > 1) that
    a scan over S, B, G, Ch / G, L and the alignment returns; the table must return each of them too"""
    uni_lanes, uni_split = set(), set()
    cpgs = (1, 2, 3, 4, 5, 7, 8, 12, 15, 16, 17, 20, 32, 64, 100, 128, 512, 2048, 2052, 4096)
    Ls = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4100)
    for S, B, G, cpg, L, aligned, layout in itertools.product((1, 2, 9), (1, 128, 4096), (1, 2, 3, 4, 8, 32, 33, 64), cpgs, Ls,
                                                              (True, False), (0, 1)):
        v = variant(dict(S=S, B=B, L=L, Ch=cpg * G, G=G, layout=layout), aligned)
        assert v is not None
        a, b = _keys(v, S)
        uni_lanes.add(a)
        if b is not None:
            uni_split.add(b)
    got_lanes, got_split = set(), set()
    for c in nf.CASES:
        v = variant(c)
        assert v is not None, c
        a, b = _keys(v, c["S"])
        got_lanes.add(a)
        if b is not None:
            got_split.add(b)
    # every combination exists somewhere: both kernels in layout 1, the ROW kernel alone in layout 0
    assert {k[:4] for k in uni_lanes} == {(lay, ker, vec, tp) for lay in (0, 1) for ker in ((0,) if lay == 0 else (0, 1))
                                          for vec in (False, True) for tp in (False, True)}
    assert {k[4] for k in uni_lanes if k[1] == 0} == {1, 2, 4, 8, 16, 32, 64}
    assert not uni_lanes - got_lanes, f"variants the table does not reach: {sorted(uni_lanes - got_lanes)}"
    assert not uni_split - got_split, f"seed-split decisions the table does not reach: {sorted(uni_split - got_split)}"


def test_table_contains_what_the_kernel_test_must_cover(variant):
    Ns = {(c["layout"], c["Ch"] // c["G"] * c["L"]) for c in nf.CASES}
    for layout in (0, 1):
        assert {(layout, n) for n in (1, 3, 4)} <= Ns
        for n in (nf.ROW_LANES * nf.NVJP_NV, nf.ROW_LANES * nf.NVJP_NV * 4):  # the on-chip row limits of either load width
            assert {(layout, n + d) for d in (-1, 0, 1)} <= Ns or {(layout, n + 4 * d) for d in (-1, 0, 1)} <= Ns
        assert any(c["layout"] == layout and c["Ch"] == c["G"] and c["Ch"] > 1 for c in nf.CASES)  # Ch / G = 1
        assert any(c["layout"] == layout and c["G"] == 1 and c["Ch"] > 1 for c in nf.CASES)
        assert any(c["layout"] == layout and c["B"] * c["G"] == 1 for c in nf.CASES)
        assert {1, nf.NVJP_SC - 1, nf.NVJP_SC + 1, 9} <= {c["S"] for c in nf.CASES if c["layout"] == layout}
        assert any(c["layout"] == layout and c["off"] == 1 for c in nf.CASES)
        assert any(c["layout"] == layout and c["w"] == "none" for c in nf.CASES)
    gn = [c for c in nf.CASES if (c["Ch"], c["G"], c["L"], c["layout"]) == (64, 32, 16, 1)]
    assert gn and variant(gn[0])["kernel"] == 1 and variant(gn[0])["vec"], "GroupNorm(32, 64) at L = 16 reads whole channel vectors"
    for c in nf.CASES:
        if c["off"]:
            assert not variant(c)["vec"]
        assert c["S"] * c["B"] * c["L"] * c["Ch"] * 4 <= 64 << 20, c
    w, _ = nf.make_affine(dict(Ch=5, w="rand"), torch.Generator().manual_seed(0), "cpu")
    assert (w == 0).any() and (w < 0).any()


def test_refused_shapes_come_back_negative(variant):
    ok = dict(S=3, B=2, L=4, Ch=8, G=2, layout=0)
    assert variant(ok) is not None
    for bad in (dict(G=3), dict(G=0), dict(layout=2), dict(S=0), dict(L=0), dict(B=1 << 31), dict(Ch=1 << 30, G=1 << 29),
                dict(L=(1 << 30) - 1, Ch=6, G=2)):
        assert variant({**ok, **bad}) is None, bad


# ---- the bounds -----------------------------------------------------------------------------------------------------------------
BOUND_NS = (1, 3, 4, 257, 4096, 65536)


def _worst(got, want, bound):
    return ((got.double() - want).abs() / bound.clamp_min(1e-300)).max().item()


@pytest.fixture(scope="module")
def bound_rows():
    """per (N, mean): fp32 rows ``[rows, 1, N]`` laid out as layout 0 with Ch = G = 1, and their float64 forward"""
    out = {}
    gen = torch.Generator().manual_seed(20)
    for N, mean in itertools.product(BOUND_NS, (0.0, 100.0)):
        rows = max(4, min(256, 65536 // N))
        x = torch.randn(rows, 1, N, generator=gen) + mean
        c = dict(S=1, B=rows, L=N, Ch=1, G=1, layout=0)
        out[(N, mean)] = (x, c, nf.forward_reference(x, None, None, c, 1e-5))
    return out


@pytest.mark.parametrize("mean", (0.0, 100.0))
@pytest.mark.parametrize("N", BOUND_NS)
def test_two_pass_fp32_forwards_meet_the_bounds(bound_rows, N, mean):
    x, c, ref = bound_rows[(N, mean)]
    xr = nf.to_rows(x, 1, 0)
    xhat, rstd = nf.forward_two_pass_fp32(xr, 1e-5)
    r1, r2 = _worst(xhat, ref["xhat"], ref["b_xhat"]), _worst(rstd, ref["rstd"], ref["b_rstd"])
    r3 = _worst(torch.nn.functional.layer_norm(xr, (N,), None, None, 1e-5), ref["xhat"], ref["b_xhat"])
    print(f"N={N} mean={mean}: two-pass xhat {r1:.3f}, rstd {r2:.3f}; torch layer_norm xhat {r3:.3f} of the bound")
    assert max(r1, r2, r3) <= 1.0


@pytest.mark.parametrize("N", (3, 4))
def test_the_uncentred_variance_fails_the_bound_at_mean_100(bound_rows, N):
    x, c, ref = bound_rows[(N, 100.0)]
    xhat, _ = nf.forward_mutant_fp32(nf.to_rows(x, 1, 0), 1e-5)
    r = _worst(xhat, ref["xhat"], ref["b_xhat"])
    print(f"N={N}: E[x^2] - mu^2 reaches {r:.1f} times the xhat bound")
    assert r > 10.0


@pytest.mark.parametrize("mean", (0.0, 100.0))
@pytest.mark.parametrize("N", BOUND_NS)
def test_the_fp32_vjp_formula_meets_its_bound(bound_rows, N, mean):
    x, c, ref = bound_rows[(N, mean)]
    gen = torch.Generator().manual_seed(N)
    xhat, rstd = ref["xhat"].float().reshape(x.shape), ref["rstd"].float().reshape(-1, 1)
    g = torch.randn(2, *x.shape, generator=gen)
    want, bound = nf.vjp_reference(g, xhat, rstd, None, c)
    t = nf.to_rows(g, 1, 0)
    xr = nf.to_rows(xhat, 1, 0)
    got = rstd.reshape(1, -1, 1, 1) * (t - t.mean(-1, keepdim=True) - xr * (t * xr).mean(-1, keepdim=True))
    r = _worst(got, want, bound)
    print(f"N={N} mean={mean}: fp32 VJP {r:.3f} of the bound")
    assert r <= 1.0
