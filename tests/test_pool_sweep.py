"""Max and average pooling in the NHWC split-fp16 reverse sweep (laplace_amd/sweep_nhwc.py) - host logic on the kernel emulation
with the pooling entry points (tests/emulated_pool_kernels.py), against float64 autograd and the oracle.

Before the rule existed every model here had ``split_reason == "... has no NHWC rule"`` and ran through the NCHW sweep; that route
is still what a model takes whose pooling the NHWC kernels do not serve, and what ``SplitSweep.nhwc_pool = False`` restores.
"""
import copy

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from laplace_amd import _lib
from laplace_amd._lib import get_kernels
from laplace_amd.sweep import AVGPOOL, MAXPOOL
from laplace_amd.sweep_nhwc import SplitSweep
from oracle import curvature_oracle as co
from tests.norm_sweep_fixtures import autograd_reference
from tests.pool_fixtures import PoolStack


@pytest.fixture(autouse=True)
def _emulated():
    from tests.emulated_pool_kernels import EmulatedPoolKernels

    prev = _lib.set_kernels_for_testing(EmulatedPoolKernels())
    yield
    _lib.set_kernels_for_testing(prev)


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-300)).item()


class ConvPoolConv(nn.Module):
    """conv - ReLU - pool - conv - tanh - global average - Linear (the pooled map feeds a 3 x 3 convolution)"""

    def __init__(self, pool):
        super().__init__()
        self.c1, self.pool, self.c2 = nn.Conv2d(3, 32, 3, 1, 1), pool, nn.Conv2d(32, 32, 3, 1, 1, bias=False)
        self.gap, self.fc = nn.AdaptiveAvgPool2d(1), nn.Linear(32, 4)

    def forward(self, x):
        h = self.pool(torch.relu(self.c1(x)))
        return self.fc(torch.flatten(self.gap(torch.tanh(self.c2(h))), 1))


class ConvAvgHead(nn.Module):
    """conv - pool - flatten - Linear: the pool reads a convolution's output directly and feeds the head"""

    def __init__(self, pool, cells):
        super().__init__()
        self.c1, self.pool, self.fc = nn.Conv2d(3, 32, 3, 1, 1), pool, nn.Linear(32 * cells, 4)

    def forward(self, x):
        return self.fc(torch.flatten(self.pool(self.c1(x)), 1))


class Functional(nn.Module):
    """the functional spellings, as the reference's examples/helper/wideresnet.py ends: ``F.avg_pool2d(out, 8)``"""

    def __init__(self):
        super().__init__()
        self.c1, self.c2, self.fc = nn.Conv2d(3, 32, 3, 1, 1), nn.Conv2d(32, 32, 3, 1, 1), nn.Linear(32, 4)

    def forward(self, x):
        h = F.max_pool2d(torch.relu(self.c1(x)), 3, stride=2, padding=1)
        h = F.avg_pool2d(torch.relu(self.c2(h)), 8)
        return self.fc(h.view(-1, 32))


MODELS = {
    "conv-relu-maxpool(3,2,1)-conv": lambda: (ConvPoolConv(nn.MaxPool2d(3, 2, 1)), 8),
    "conv-relu-maxpool(2)-conv on 7x7": lambda: (ConvPoolConv(nn.MaxPool2d(2)), 7),  # (the last row and column in no window)
    "conv-relu-avgpool(3,2,1,no pad count)-conv": lambda: (ConvPoolConv(nn.AvgPool2d(3, 2, 1, count_include_pad=False)), 8),
    "conv-avgpool(2)-head": lambda: (ConvAvgHead(nn.AvgPool2d(2), 16), 8),
    "conv-avgpool(3,1,1,divisor 4)-head": lambda: (ConvAvgHead(nn.AvgPool2d(3, 1, 1, divisor_override=4), 16), 4),
    "vgg": lambda: (PoolStack(4, cfg=(32, "M", 32, "M"), in_hw=8), 8),  # (pool - flatten - Linear)
    "vgg-tanh": lambda: (PoolStack(4, cfg=(32, "M", 64, 32, "M"), in_hw=8, act=nn.Tanh), 8),
    "functional": lambda: (Functional(), 16),
}


def _build(name, seed=0):
    torch.manual_seed(seed + len(name))
    model, hw = MODELS[name]()
    model = model.double().eval()
    X, y = torch.randn(3, 3, hw, hw, dtype=torch.float64), torch.randint(4, (3,))
    return model, X, y


def _taps(model):
    return {n: m for n, m in model.named_modules() if isinstance(m, (nn.Conv2d, nn.Linear))}


def _n_pools(sw):
    return sum(r.kind in (MAXPOOL, AVGPOOL) for r in sw.rule.values())


@pytest.mark.parametrize("name", sorted(MODELS))
def test_pooled_models_take_the_split_sweep_and_match_float64_autograd(name, monkeypatch):
    m64, X, y = _build(name)
    model = copy.deepcopy(m64).float()
    taps = _taps(model)
    K, calls = get_kernels(), []
    for what in ("pool_forward", "pool_vjp"):
        inner = getattr(K, what)
        monkeypatch.setattr(K, what, lambda *a, _i=inner, _w=what, **kw: (calls.append((_w, kw.get("amax") is not None)),
                                                                          _i(*a, **kw))[1], raising=False)
    sw = SplitSweep(model, taps, kernels=get_kernels)
    assert sw.split_ok, sw.split_reason
    seeds = torch.randn(3, 3, 4, dtype=torch.float64)
    f = sw.forward(X.float())
    grads = sw.backward(seeds.float())
    # one forward launch per pooling node, one VJP launch for ALL seeds per node, each with a max|dx| word
    assert sorted(calls) == [("pool_forward", False)] * _n_pools(sw) + [("pool_vjp", True)] * _n_pools(sw), calls
    f64, ins, want = autograd_reference(m64, _taps(m64), X, seeds)
    assert rel(f, f64.detach()) < 1e-5
    for n in taps:
        assert rel(sw.taps[n]["a"], ins[n]) < 1e-5, n
        assert grads[n].shape == want[n].shape, n
        assert rel(grads[n], want[n]) < 1e-4, (n, rel(grads[n], want[n]))


@pytest.mark.parametrize("name", ["conv-relu-maxpool(3,2,1)-conv", "conv-avgpool(2)-head", "vgg"])
def test_jacobians_and_kfac_factors_equal_the_oracle(name):
    from laplace_amd import HipGGN

    m64, X, y = _build(name)
    b = HipGGN(copy.deepcopy(m64).float(), "classification")
    Js, f = b.jacobians(X.float())
    loss, kron = b.kron(X.float(), y, N=3)
    sweep = b._tape().sweep
    assert isinstance(sweep, SplitSweep) and sweep.split_ok, getattr(sweep, "split_reason", None)
    Js_ref, f_ref = co.jacobians(m64, X)
    assert rel(f, f_ref) < 1e-5 and rel(Js, Js_ref) < 1e-4, rel(Js, Js_ref)
    loss_ref, kf_ref = co.kfac_ggn(m64, X, y, 3, "classification")
    assert rel(loss, loss_ref) < 1e-5
    for i, (F_, G_) in enumerate(zip(kron.kfacs, kf_ref)):
        for j, (a, ref) in enumerate(zip(F_, G_)):
            assert rel(a, ref) < 1e-4, (i, j, rel(a, ref))


def _refused(pool, kernels=get_kernels, name="conv-relu-maxpool(3,2,1)-conv", hw=12):
    torch.manual_seed(1)
    model = ConvPoolConv(pool).eval()
    taps = _taps(model)
    sw = SplitSweep(model, taps, kernels=kernels)
    # the NCHW route serves the model as before: against one autograd pass per seed
    x, seeds = torch.randn(2, 3, hw, hw), torch.randn(2, 2, 4)
    f = sw.forward(x)
    grads = sw.backward(seeds)
    f_ref, _, want = autograd_reference(model, taps, x, seeds)
    assert torch.allclose(f, f_ref, rtol=1e-4, atol=1e-6)
    for n in taps:
        assert torch.allclose(grads[n], want[n], rtol=1e-4, atol=1e-6), n
    return sw


@pytest.mark.parametrize("pool,fragment", [
    (nn.MaxPool2d(3, 2, 1, ceil_mode=True), "pool: pooling with ceil_mode=True"),
    (nn.AvgPool2d(3, 2, 1, ceil_mode=True), "pool: pooling with ceil_mode=True"),
    (nn.MaxPool2d(2, 2, 0, dilation=2), "pool: dilated pooling"),
    (nn.MaxPool2d(9, 1, 4), "pool: pooling window (9, 9)"),
    (nn.AvgPool2d((2, 9), 1, (1, 4)), "pool: pooling window (2, 9)"),
], ids=["max-ceil", "avg-ceil", "dilation", "9x9", "2x9"])
def test_pooling_outside_the_kernels_contract_names_the_node_and_keeps_the_nchw_route(pool, fragment):
    sw = _refused(pool)
    assert not sw.split_ok and fragment in sw.split_reason, sw.split_reason


@pytest.mark.parametrize("missing", ("pool_forward", "pool_vjp", "POOL_MAX", "POOL_AVG"))
def test_split_sweep_wants_both_pooling_entry_points(missing):
    def absent(self):
        raise AttributeError(missing)

    K = type("OneEntryPoint", (type(get_kernels()),), {missing: property(absent)})()
    assert not hasattr(K, missing)
    sw = _refused(nn.MaxPool2d(3, 2, 1), kernels=lambda: K)
    assert not sw.split_ok and sw.split_reason == "pool: kernels without the pooling entry points"


def test_the_stock_emulation_keeps_pooled_models_on_the_nchw_route():
    from tests.emulated_kernels import EmulatedKernels

    prev = _lib.set_kernels_for_testing(EmulatedKernels())
    try:
        sw = _refused(nn.MaxPool2d(3, 2, 1))
    finally:
        _lib.set_kernels_for_testing(prev)
    assert not sw.split_ok and "kernels without the pooling entry points" in sw.split_reason


def test_the_functional_spelling_is_named_by_its_node():
    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.c1, self.fc = nn.Conv2d(3, 32, 3, 1, 1), nn.Linear(32, 4)

        def forward(self, x):
            return self.fc(F.max_pool2d(self.c1(x), 4, ceil_mode=True).flatten(1))

    m = M().eval()
    sw = SplitSweep(m, _taps(m), kernels=get_kernels)
    assert not sw.split_ok and sw.split_reason == "max_pool2d: pooling with ceil_mode=True (the NHWC kernels take ceil_mode=False only)"


def test_pooling_in_the_head_region_is_refused():
    """a pool whose input is no feature map (a reshaped head tensor) has no NHWC memory to run on"""
    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.c1, self.gap, self.fc = nn.Conv2d(3, 32, 3, 1, 1), nn.AdaptiveAvgPool2d(1), nn.Linear(8, 4)

        def forward(self, x):
            h = torch.flatten(self.gap(self.c1(x)), 1).view(-1, 2, 4, 4)
            return self.fc(F.avg_pool2d(h, 2).flatten(1))

    m = M().eval()
    sw = SplitSweep(m, _taps(m), kernels=get_kernels)
    assert not sw.split_ok and "avg_pool2d: avg_pool2d outside the feature maps" in sw.split_reason, sw.split_reason


def test_the_switch_restores_the_reason_and_the_route_of_before(monkeypatch):
    monkeypatch.setattr(SplitSweep, "nhwc_pool", False)
    sw = _refused(nn.MaxPool2d(3, 2, 1))
    assert not sw.split_ok and sw.split_reason == "pool: MaxPool2d has no NHWC rule"
    sw = _refused(nn.AvgPool2d(2))
    assert not sw.split_ok and sw.split_reason == "pool: AvgPool2d has no NHWC rule"
    m = Functional().eval()
    sw = SplitSweep(m, _taps(m), kernels=get_kernels)
    assert not sw.split_ok and sw.split_reason == "max_pool2d has no NHWC rule"


def test_the_pooled_map_inherits_the_per_image_bound_of_its_input():
    """pooling cannot raise a map's maximum: behind a BatchNorm launch (which measures per-image maxima) the pooled map carries
    the same words, and registers no split copy; an average with a divisor of its own inherits nothing"""
    class M(nn.Module):
        def __init__(self, pool):
            super().__init__()
            self.c1, self.bn, self.pool = nn.Conv2d(3, 32, 3, 1, 1, bias=False), nn.BatchNorm2d(32), pool
            self.c2, self.gap, self.fc = nn.Conv2d(32, 32, 3, 1, 1), nn.AdaptiveAvgPool2d(1), nn.Linear(32, 4)

        def forward(self, x):
            h = self.pool(torch.relu(self.bn(self.c1(x))))
            return self.fc(torch.flatten(self.gap(self.c2(h)), 1))

    for pool, inherits in ((nn.MaxPool2d(3, 2, 1), True), (nn.AvgPool2d(2), True), (nn.AvgPool2d(2, divisor_override=1), False)):
        torch.manual_seed(4)
        m = M(pool).eval()
        sw = SplitSweep(m, _taps(m), kernels=get_kernels)
        assert sw.split_ok, sw.split_reason
        seen = {}
        inner = sw._run_pool

        def spy(node, r, args, kwargs, _inner=inner, _sw=sw, _seen=seen):
            out, keep = _inner(node, r, args, kwargs)
            _seen["in"], _seen["out"] = _sw._aux_get(args[0]), _sw._aux_get(out)
            return out, keep

        sw._run_pool = spy
        x = torch.randn(3, 3, 8, 8)
        f = sw.forward(x)
        assert torch.allclose(f, m(x), rtol=1e-4, atol=1e-5)
        assert seen["in"] is not None and seen["in"].get("bound") is not None
        if inherits:
            assert seen["out"]["bound"] is seen["in"]["bound"] and seen["out"]["split"] is None
        else:
            assert seen["out"] is None


def test_an_inference_only_forward_keeps_nothing_for_the_pools():
    m64, X, _ = _build("vgg")
    model = copy.deepcopy(m64).float()
    sw = SplitSweep(model, _taps(model), kernels=get_kernels)
    assert sw.split_ok, sw.split_reason
    f = sw.forward(X.float(), need_vjp=False)
    assert sw.saved == {} and rel(f, m64(X).detach()) < 1e-5
    sw.forward(X.float())
    assert sum(sw.rule[n].kind == MAXPOOL for n in sw.saved) == 2
