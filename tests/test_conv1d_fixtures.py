"""The test infrastructure of the 1-D convolutional networks checks itself on the CPU: the case table of tests/conv1d_fixtures.py
reaches every path ``lk_reduce_variant`` reports, the stated references tell the kernels' plausible mistakes apart (a last-maximum
kernel, an ``amax`` answered with the first maximum, a skipped zero fill), the end-to-end inputs keep the gap they promise and each
2-D twin is the same function."""
import pytest
import torch

from tests import conv1d_fixtures as cf


def _variant(c, vjp, even=False):
    from laplace_amd._lib import HipKernels

    return HipKernels().reduce_variant(vjp, c["S"], c["outer"], c["L"], c["inner"], even, cf.aligned(c))


def test_the_case_table_reaches_every_path():
    fwd = [_variant(c, False) for c in cf.CASES if c["outer"]]
    vjp = [_variant(c, True, even) for c in cf.CASES if c["outer"] for even in (False, True)]
    assert None not in fwd and None not in vjp
    # forward: the row path with every group size 1 .. 64, the column path with and without vectors
    assert {v["lanes"] for v in fwd if v["row"]} == {1, 2, 4, 8, 16, 32, 64}
    assert {(v["row"], v["vec"]) for v in fwd} == {(True, False), (False, False), (False, True)}
    # VJP: both layouts, both access widths, both modes; the seeds split over grid.y and not
    assert {(v["row"], v["vec"], v["even"]) for v in vjp} == {(r, w, e) for r in (True, False) for w in (True, False) for e in (True, False)}
    assert {v["seed_split"] for v in vjp} == {True, False}
    # an unaligned base drops the vectors of a shape that would take them
    for c in cf.CASES:
        if c["off"] % 4:
            al = dict(c, off=0)
            assert not _variant(c, True)["vec"] and (_variant(al, True)["vec"] or _variant(al, False)["vec"])
    # one lane past a full stride of the grid on each path: the grid is capped and the work exceeds one stride of it
    full = [c for c in cf.runnable() if c["outer"] > 2048]
    paths = set()
    for c in full:
        for v in (_variant(c, False), _variant(c, True)):
            if v["blocks"] == 2048:
                paths.add((v["vjp"], v["row"], v["vec"]))
    assert paths >= {(False, True, False), (False, False, False), (False, False, True), (True, True, False), (True, True, True),
                     (True, False, False), (True, False, True)}, paths
    # past 2^31 lanes: the 64-bit index, on the forward's column path and on the VJP's row and column paths (never run)
    wide = {(v["vjp"], v["row"]) for c in cf.CASES if c["huge"] for v in (_variant(c, False), _variant(c, True)) if v["wide_index"]}
    assert wide >= {(True, True), (True, False)}, wide
    assert all(c["outer"] * c["L"] * c["inner"] >= (1 << 31) for c in cf.CASES if c["huge"])
    assert not any(c["outer"] * c["L"] * c["inner"] * c["S"] >= (1 << 24) for c in cf.runnable())  # (seconds, not minutes)


def test_shapes_outside_the_contract_have_no_variant():
    from laplace_amd._lib import HipKernels

    K = HipKernels()
    assert K.reduce_variant(True, 1, 1, 1 << 30, 1) is None and K.reduce_variant(True, 1, 1, 1, 1 << 30) is None
    assert K.reduce_variant(True, 0, 1, 1, 1) is None and K.reduce_variant(True, 1, -1, 1, 1) is None
    assert K.reduce_variant(True, 2, 1 << 20, 1 << 19, 1) is None  # (S * outer * L * inner = 2^40)
    assert K.reduce_variant(False, 1, 1 << 16, 1, 1 << 15) is None  # (outer * inner = 2^31)
    assert K.reduce_variant(True, 1, 0, 1, 1) is not None


def test_the_fills_are_what_they_say():
    gen = torch.Generator().manual_seed(0)
    for c in cf.runnable():
        if not c["outer"]:
            continue
        x = cf.make_x(c, gen)
        y, idx, cnt = cf.forward_reference(x)
        L = c["L"]
        want = {"first": (0, 1), "last": (L - 1, 1), "twice": (L // 3, 2 if L // 3 != L - 1 else 1), "all": (0, L),
                "negzero": (L // 3, 2), "neginf": (0, L)}.get(c["fill"])
        if want is None:
            assert bool((cnt == 1).all()), cf.case_id(c)
        else:
            assert bool((idx == want[0]).all()) and bool((cnt == want[1]).all()), (cf.case_id(c), idx.unique(), cnt.unique())
        if c["fill"] == "negzero":  # (-0.0 comes first and 0.0 == -0.0: torch's max reports the first, as the reference)
            assert torch.equal(x.max(1).indices.int(), idx) and bool((x[:, L // 3] == 0).all()) and bool(torch.signbit(x[:, L // 3]).all())
    assert torch.max(torch.tensor([0.0, -0.0, 0.0]), 0).indices.item() == 0


def test_the_references_are_autograds_rules():
    gen = torch.Generator().manual_seed(1)
    for c in cf.runnable():
        if not c["outer"] or c["outer"] > 300 or c["fill"] == "neginf":
            continue
        x = cf.make_x(c, gen).double().requires_grad_(True)
        g = torch.randn(c["S"], c["outer"], c["inner"], generator=gen).double()
        for even, out in ((False, x.max(1).values), (True, x.amax(1))):
            want = torch.stack([torch.autograd.grad(out, x, g[s], retain_graph=True)[0] for s in range(c["S"])])
            got = cf.vjp_reference(g, x.detach().float(), even)
            assert torch.allclose(got, want, rtol=1e-12, atol=0), (cf.case_id(c), even)


def _first_index_cases():
    return [c for c in cf.runnable() if 0 < c["outer"] <= 300 and c["fill"] in ("twice", "all", "negzero", "neginf")]


def test_a_last_maximum_mutant_fails_the_first_index_cases():
    gen = torch.Generator().manual_seed(2)
    for c in _first_index_cases():
        if c["L"] == 1:
            continue
        x = cf.make_x(c, gen)
        assert not torch.equal(cf.forward_reference(x, "last")[1], cf.forward_reference(x)[1]), cf.case_id(c)
        g = torch.randn(c["S"], c["outer"], c["inner"], generator=gen) + 0.05
        assert not torch.equal(cf.vjp_reference(g, x, False, "last"), cf.vjp_reference(g, x, False)), cf.case_id(c)


def test_a_first_index_amax_mutant_fails_the_tie_cases():
    gen = torch.Generator().manual_seed(3)
    for c in _first_index_cases():
        if c["L"] == 1:
            continue
        x = cf.make_x(c, gen)
        g = torch.randn(c["S"], c["outer"], c["inner"], generator=gen) + 0.05
        bad, good = cf.vjp_reference(g, x, True, "first-for-amax"), cf.vjp_reference(g, x, True)
        assert bool(((bad - good).abs() > cf.even_bound(g, x)).any()), cf.case_id(c)


def test_a_mutant_that_skips_the_zero_fill_fails():
    gen = torch.Generator().manual_seed(4)
    for c in cf.runnable():
        if not 0 < c["outer"] <= 300 or c["L"] == 1 or c["fill"] in ("all", "neginf"):
            continue
        x = cf.make_x(c, gen)
        g = torch.randn(c["S"], c["outer"], c["inner"], generator=gen) + 0.05
        stale = torch.full((c["S"], c["outer"], c["L"], c["inner"]), float("nan"))
        for even in (False, True):
            bad, good = cf.vjp_reference(g, x, even, "no-fill", stale), cf.vjp_reference(g, x, even)
            if bool((good == 0).any()):  # (an even split over two maxima of two positions owes no zero)
                assert not torch.equal(bad, good), (cf.case_id(c), even)


def test_the_emulation_states_the_same_rules():
    from laplace_amd.sweep import reduce_forward_math, reduce_vjp_math
    from tests.emulated_reduce_kernels import EmulatedReduceKernels

    K, gen = EmulatedReduceKernels(), torch.Generator().manual_seed(5)
    for c in cf.runnable():
        if not c["outer"] or c["outer"] > 300:
            continue
        S, o, L, i = c["S"], c["outer"], c["L"], c["inner"]
        x = cf.make_x(c, gen)
        g = torch.randn(S, o, i, generator=gen)
        y, idx, cnt = K.maxred_forward(x, o, L, i)
        for a, b in zip((y, idx, cnt), reduce_forward_math(x)):
            assert torch.equal(a, b), cf.case_id(c)
        assert torch.equal(K.maxred_vjp(g, S, o, L, i, idx=idx), reduce_vjp_math(g, L, idx=idx))
        assert torch.allclose(K.maxred_vjp(g, S, o, L, i, x=x, y=y, cnt=cnt), reduce_vjp_math(g, L, x=x, y=y, cnt=cnt), rtol=1e-6, atol=0)


# ---- end-to-end fixtures ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=sorted(cf.FIXTURES))
def fixture(request):
    return request.param, cf.FIXTURES[request.param]()


def test_every_maximum_keeps_the_gap_in_float64(fixture):
    name, (m, twin, X, X2, y) = fixture
    gaps = cf._gaps(m, X)
    assert gaps and min(gaps) >= cf.GAP, (name, gaps)


def test_the_twin_is_the_same_function(fixture):
    from oracle import curvature_oracle as co

    name, (m, twin, X, X2, y) = fixture
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in twin.named_parameters()]
    assert [p.requires_grad for p in m.parameters()] == [p.requires_grad for p in twin.parameters()]
    assert [p.numel() for p in m.parameters()] == [p.numel() for p in twin.parameters()]
    assert any(isinstance(mod, torch.nn.Conv1d) for mod in m.modules())
    assert not any(isinstance(mod, torch.nn.Conv1d) for mod in twin.modules())
    J1, f1 = co.jacobians(m, X)
    J2, f2 = co.jacobians(twin, X2)
    assert (f1 - f2).abs().max() <= 1e-12 * f1.abs().max() and (J1 - J2).abs().max() <= 1e-12 * J1.abs().max()


def test_the_resnet_fixture_holds_what_it_promises():
    m = cf.resnet1d_fixture()[0]
    convs = [mod for mod in m.modules() if isinstance(mod, torch.nn.Conv1d)]
    assert any(c.stride[0] == 2 and c.dilation[0] == 2 for c in convs) and any(c.groups == c.in_channels > 1 for c in convs)
    assert any(isinstance(mod, torch.nn.MaxPool1d) for mod in m.modules())
