"""The fixture table of the depthwise-convolution kernels (tests/dwconv_fixtures.py) does what tests/test_gpu_dwconv.py relies on,
and the host rule of the NHWC sweep for depthwise layers - on the CPU:

* through ``lk_dwconv_variant`` (pure host code of csrc/lk_dwconv.hip) the table reaches every path: wide and scalar accesses,
  with and without stride, both tap classes, the seeds in one slice and split over grid.y, and a seed loop that ends one short
  of, at, and one past the seeds per pass;
* the emulation (tests/emulated_dwconv_kernels.py: the gather form, by index) meets every assertion of the device test against
  the float64 references (the scatter definition), and two MUTANTS fail the cases they should: a backward that correlates instead
  of transposing, and one that drops the divisibility test of a strided layer;
* ``SplitSweep`` admits the end-to-end fixtures, names the node and the cause for every variant it refuses (such a model still
  computes what the NCHW sweep computes), and registers the forward bound that spares the BatchNorm behind a depthwise layer its
  ``absmax`` pass;
* the ReLU / ReLU6 fixtures keep every pre-activation clear of a decision point in the float64 forward.
"""
import copy
import os

import pytest
import torch
from torch import nn

from tests import dwconv_fixtures as df
from tests.emulated_dwconv_kernels import EmulatedDwconvKernels


@pytest.fixture(scope="module")
def variant():
    from laplace_amd._lib import LIB_PATH, HipKernels

    if not os.path.exists(LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    K = HipKernels()
    return lambda c, aligned=None: K.dwconv_variant(c["S"], c["B"], c["H"], c["W"], c["C"], c["k"], c["s"], c["p"],
                                                    not c["off"] if aligned is None else aligned)


def test_the_table_reaches_every_path(variant):
    plans = [variant(c) for c in df.CASES]
    assert all(p is not None for p in plans)
    assert {p["seeds_per_pass"] for p in plans} == {df.SEEDS_PER_PASS}
    seen = {(p["vec"], p["strided"], p["tap_class"]) for p in plans}
    assert seen == {(v, s, t) for v in (False, True) for s in (False, True) for t in (0, 1)}, seen
    assert {(p["seed_split"], p["tap_class"]) for p in plans} >= {(False, 0), (False, 1), (True, 0), (True, 1)}
    for c, p in zip(df.CASES, plans):
        assert p["vec"] == (c["C"] % 4 == 0 and not c["off"]) and p["strided"] == df.strided(c), df.case_id(c)
        assert p["tap_class"] == int(df.taps(c) > 9), df.case_id(c)
    # the seeds a lane loops over: the slice, and the last slice's remainder
    loops = set()
    for c, p in zip(df.CASES, plans):
        loops |= {min(p["seeds_per_slice"], c["S"]), c["S"] - (-(-c["S"] // p["seeds_per_slice"]) - 1) * p["seeds_per_slice"]}
    assert {df.SEEDS_PER_PASS - 1, df.SEEDS_PER_PASS, df.SEEDS_PER_PASS + 1} <= loops, sorted(loops)
    split_with_passes = [c for c, p in zip(df.CASES, plans) if p["seed_split"] and p["seeds_per_slice"] > df.SEEDS_PER_PASS]
    assert split_with_passes, "no case splits the seeds AND loops more than one pass in a slice"
    # an unaligned base turns the wide path off for a channel count that would take it
    c = next(c for c in df.CASES if c["off"] and c["C"] % 4 == 0)
    assert variant(c, True)["vec"] and not variant(c, False)["vec"]


def test_the_table_holds_what_the_device_test_lists():
    geos = {(c["k"], c["s"], c["p"], (c["H"], c["W"])) for c in df.CASES}
    assert len(df.GEOMETRIES) == 12 and {tuple(df._pair(v) for v in g) for g in df.GEOMETRIES} <= geos
    for g in {tuple(df._pair(v) for v in g) for g in df.GEOMETRIES}:
        mine = [c for c in df.CASES if (c["k"], c["s"], c["p"], (c["H"], c["W"])) == g]
        assert {c["C"] for c in mine} >= {4, 6, 8, 12, 68} and {c["B"] for c in mine} == {1, 3}, g
        assert {c["off"] for c in mine} == {0, 1}, g
    assert {c["S"] for c in df.CASES} >= {1, 2, 9, 17, df.SEEDS_PER_PASS - 1, df.SEEDS_PER_PASS, df.SEEDS_PER_PASS + 1}
    for sub in ([c for c in df.CASES if df.strided(c)], [c for c in df.CASES if not df.strided(c)],
                [c for c in df.CASES if df.taps(c) > 9], [c for c in df.CASES if df.taps(c) <= 9]):
        assert {c["S"] for c in sub} >= {1, 2, 9, 17, df.SEEDS_PER_PASS - 1, df.SEEDS_PER_PASS, df.SEEDS_PER_PASS + 1}
    n_bias = sum(c["bias"] for c in df.CASES)
    assert abs(2 * n_bias - len(df.CASES)) <= 2, "bias on half of the forward cases"


def _run(K, c):
    """the assertions of tests/test_gpu_dwconv.py on a kernel object -> list of failures"""
    gen = torch.Generator().manual_seed(31 + df.CASES.index(c))
    x, w_tap, bias, g = df.make_inputs(c, gen)
    bad = []
    y = K.dwconv_forward(x, w_tap, bias, c["k"], c["s"], c["p"])
    ref, bound = df.forward_reference(c, x, w_tap, bias)
    if tuple(y.shape) != tuple(ref.shape) or not bool(((y.double() - ref).abs() <= bound).all()):
        bad.append("y")
    amax = torch.zeros(1)
    dx = K.dwconv_backward(g, w_tap, c["S"], (c["H"], c["W"]), c["k"], c["s"], c["p"], amax=amax)
    dx = dx.reshape(c["S"], c["B"], c["H"], c["W"], c["C"])
    want, bound = df.backward_reference(c, g.planes, g.sexp, w_tap)
    if not bool(((dx.double() - want).abs() <= bound).all()):
        bad.append("dx")
    if not torch.equal(amax.view(torch.int32), dx.abs().max().reshape(1).view(torch.int32)):
        bad.append("amax")
    return bad


@pytest.mark.parametrize("c", df.CASES, ids=df.case_id)
def test_the_emulation_meets_the_references(c):
    assert _run(EmulatedDwconvKernels(), c) == []


def test_a_correlating_mutant_fails_every_case_with_more_than_one_tap():
    mutant = EmulatedDwconvKernels()
    mutant.correlate = True
    for c in df.CASES:
        bad = _run(mutant, c)
        # (on a 1 x 1 map under a padded 3 x 3 window only the centre tap lies in the image, and the centre is its own mirror)
        centre_only = (c["H"], c["W"]) == (1, 1)
        assert ("dx" in bad) == (df.taps(c) > 1 and not centre_only), df.case_id(c)
        assert "y" not in bad, df.case_id(c)


def test_a_mutant_without_the_divisibility_test_fails_the_strided_cases_only():
    mutant = EmulatedDwconvKernels()
    mutant.floor_div = True
    for c in df.CASES:
        assert ("dx" in _run(mutant, c)) == df.strided(c), df.case_id(c)


# ---- the host rule, on the emulation -------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _depthwise_route(monkeypatch):
    """the route under test is opt-in (``SplitSweep.nhwc_depthwise`` is off by default: DESIGN.md section 3)"""
    from laplace_amd.sweep_nhwc import SplitSweep

    assert SplitSweep.nhwc_depthwise is False  # (the default stays off until both lines of tools/dwconv_bench.py gain)
    monkeypatch.setattr(SplitSweep, "nhwc_depthwise", True)


@pytest.fixture
def dw_kernels():
    from laplace_amd import _lib

    prev = _lib.set_kernels_for_testing(EmulatedDwconvKernels())
    yield
    _lib.set_kernels_for_testing(prev)


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300)).item()


@pytest.mark.parametrize("name", df.E2E)
def test_the_split_sweep_admits_the_end_to_end_fixtures(dw_kernels, name, monkeypatch):
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep_nhwc import SplitSweep

    m64, X, _ = df.e2e_fixture(name)
    model = copy.deepcopy(m64).float()
    sw = SplitSweep(model, df.e2e_taps(model), kernels=get_kernels)
    assert sw.split_reason is None and sw.split_ok
    assert set(df.depthwise_names(model)) <= sw.tap_names and len(df.depthwise_names(model)) in (2, 6)
    # the switch restores the route, and the reason, of a model with a grouped convolution
    monkeypatch.setattr(SplitSweep, "nhwc_depthwise", False)
    off = SplitSweep(model, df.e2e_taps(model), kernels=get_kernels)
    first = df.depthwise_names(model)[0]
    assert not off.split_ok
    assert off.split_reason == f"{first}: grouped convolution (foreign to the NHWC kernels; the NCHW sweep serves it)"


def _refused_model(grouped):
    return nn.Sequential(nn.Conv2d(3, 32, 3, padding=1), nn.Tanh(), grouped, nn.Tanh(), nn.Conv2d(grouped.out_channels, 32, 1),
                         nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(32, 3)).eval()


REFUSED = {  # cause -> (the grouped layer, what the reason must say)
    "channel multiplier": (lambda: nn.Conv2d(32, 64, 3, padding=1, groups=32), "channel multiplier 2"),
    "narrow groups": (lambda: nn.Conv2d(32, 32, 3, padding=1, groups=8), "narrow groups"),
    "window": (lambda: nn.Conv2d(32, 32, (5, 6), padding=2, groups=32), "kh kw > 25"),
    "dilation": (lambda: nn.Conv2d(32, 32, 3, padding=2, dilation=2, groups=32), "dilation (2, 2)"),
    "stride": (lambda: nn.Conv2d(32, 32, 3, stride=9, padding=1, groups=32), "stride (9, 9) above 8"),
    "padding": (lambda: nn.Conv2d(32, 32, 3, padding=3, groups=32), "padding (3, 3) not below the window"),
    "entry points": (lambda: nn.Conv2d(32, 32, 3, padding=1, groups=32), "kernels without the depthwise entry points"),
    "switch": (lambda: nn.Conv2d(32, 32, 3, padding=1, groups=32), "foreign to the NHWC kernels"),
}


@pytest.mark.parametrize("cause", sorted(REFUSED))
def test_a_refused_variant_names_the_node_and_the_cause_and_takes_the_nchw_sweep(cause, monkeypatch):
    from laplace_amd import HipGGN, _lib
    from laplace_amd.sweep_nhwc import SplitSweep
    from tests.emulated_gconv_kernels import EmulatedGConvKernels
    from tests.emulated_pool_kernels import EmulatedPoolKernels

    class WithoutDepthwise(EmulatedPoolKernels, EmulatedGConvKernels):
        pass

    make, says = REFUSED[cause]
    torch.manual_seed(5)
    model = _refused_model(make())
    X, y = torch.randn(4, 3, 8, 8), torch.randint(3, (4,))
    prev = _lib.set_kernels_for_testing(WithoutDepthwise() if cause == "entry points" else EmulatedDwconvKernels())
    if cause == "switch":
        monkeypatch.setattr(SplitSweep, "nhwc_depthwise", False)
    try:
        b = HipGGN(model, "classification")
        loss, h = b.diag(X, y)
        tape = b._tape()
        sweeps = [s for s in tape.sweeps.values() if s]
        assert sweeps and all(isinstance(s, SplitSweep) and not s.split_ok for s in sweeps)
        for s in sweeps:
            assert s.split_reason.startswith("2: grouped convolution (") and says in s.split_reason, s.split_reason
        nchw = HipGGN(model, "classification")
        nchw.use_split_sweep = False
        loss2, h2 = nchw.diag(X, y)
        assert _rel(h, h2) < 1e-6 and _rel(loss, loss2) < 1e-6
    finally:
        _lib.set_kernels_for_testing(prev)
    # (the same layer on the depthwise route, where the contract admits it, computes the same diagonal)
    if cause in ("entry points", "switch"):
        prev = _lib.set_kernels_for_testing(EmulatedDwconvKernels())
        monkeypatch.setattr(SplitSweep, "nhwc_depthwise", True)
        try:
            b = HipGGN(model, "classification")
            _, h3 = b.diag(X, y)
            sweep = b._tape().sweeps[frozenset({"gconv"})]
            assert sweep.split_ok, sweep.split_reason
            assert _rel(h3, h2) < 1e-4
        finally:
            _lib.set_kernels_for_testing(prev)


def test_a_depthwise_layer_off_the_feature_maps_or_alone_is_refused(dw_kernels):
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep_nhwc import SplitSweep

    # admitted depthwise layers do not count as convolutions: a graph still needs a dense one
    alone = nn.Sequential(nn.Conv2d(32, 32, 3, padding=1, groups=32), nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(32, 3)).eval()
    sw = SplitSweep(alone, {"0": alone[0], "3": alone[3]}, kernels=get_kernels)
    assert not sw.split_ok and sw.split_reason == "no convolution in the graph"


def test_the_forward_bound_spares_the_batchnorm_behind_a_depthwise_layer_its_absmax(dw_kernels, monkeypatch):
    """the ReLU fixture: every depthwise layer reads the output of a fused BatchNorm + ReLU launch, whose per-image maxima are
    known; with the bound ``max|x_n| * l1`` registered no feature map is measured in the forward.  Control: without the
    registration every BatchNorm behind a depthwise layer measures its input."""
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep_nhwc import SplitSweep

    m64, X, _ = df.e2e_fixture("v1-relu")
    model = copy.deepcopy(m64).float()
    sw = SplitSweep(model, df.e2e_taps(model), kernels=get_kernels)
    assert sw.split_ok, sw.split_reason
    K, maps = get_kernels(), []
    real = K.absmax
    monkeypatch.setattr(K, "absmax", lambda x, out=None: (maps.append(tuple(x.shape)) if x.dim() == 4 else None, real(x, out))[1],
                        raising=False)
    sw.forward(X.float())  # (fills the caches of the per-model constants)
    maps.clear()
    f = sw.forward(X.float())
    assert maps == [], maps
    # control: drop the depthwise registrations
    monkeypatch.setattr(SplitSweep, "_run_depthwise", _without_bound(SplitSweep._run_depthwise))
    f2 = sw.forward(X.float())
    assert len(maps) == len(df.depthwise_names(model)), maps
    assert _rel(f2, f) < 1e-5


def _without_bound(run):
    def wrapped(self, node, m, inp):
        out = run(self, node, m, inp)
        self._aux.pop(out.data_ptr(), None)
        return out

    return wrapped


@pytest.mark.parametrize("name", [n for n in df.E2E if n != "v1-tanh"])
def test_the_relu_fixtures_keep_their_decisions_clear_of_near_ties(name):
    gap, seen = df.e2e_gaps(name)
    assert seen >= 100000, seen  # (the probes looked at every ReLU / ReLU6 of the network)
    assert gap > df.GAP, f"a pre-activation lies {gap:.2e} of its map's maximum from a decision point"
    # the signed layers do decide: a fifth of the pre-activations of the fixture, at the least, are switched off or clamped
    m, X, _ = df.e2e_fixture(name)
    acts = []
    hooks = [mod.register_forward_hook(lambda mod_, i, o: acts.append(((o == 0) | (o == 6)).double().mean().item()))
             for mod in m.modules() if isinstance(mod, (nn.ReLU, nn.ReLU6))]
    with torch.no_grad():
        m(X)
    for h in hooks:
        h.remove()
    assert max(acts[:2]) > 0.2, acts
