"""The CAT rule of both seed-batched reverse sweeps (laplace_amd/sweep.py, laplace_amd/sweep_nhwc.py) on the CPU: models that
concatenate go through ONE sweep for all seeds and match one autograd pass per seed; the curvature quantities built on it match
the fp64 oracle; what the rule does not serve is refused by name and the backend answers through the tape; the kernel branch of
the split sweep's rule runs on the emulation (tests/emulated_cat_kernels.py).

Before the rule existed every model here was refused whole ("no VJP rule for function cat") and took the autograd tape."""
import copy

import pytest
import torch
import torch.fx as fx
import torch.nn.functional as F
from torch import nn

from laplace_amd import _lib
from laplace_amd._lib import SplitTensor, get_kernels, is_channels_last
from laplace_amd.sweep import CAT, CONST, Rule, SeedBatchedSweep, SweepUnsupported, classify
from laplace_amd.sweep_nhwc import SplitSweep
from tests import cat_fixtures as cf
from tests.norm_sweep_fixtures import autograd_reference


def _taps(model):
    return {n: m for n, m in model.named_modules() if isinstance(m, (nn.Linear, nn.Conv2d))}


# ---- 1. the sweep against autograd ---------------------------------------------------------------------------------------------------
class Nested(nn.Module):
    """DenseNet-style nested binary concatenations: cat([cat([x, a]), b])"""

    def __init__(self):
        super().__init__()
        self.c0, self.c1, self.c2 = nn.Conv2d(3, 4, 3, 1, 1), nn.Conv2d(4, 2, 3, 1, 1), nn.Conv2d(6, 2, 1)
        self.bn = nn.BatchNorm2d(8)
        self.fc = nn.Linear(8, 3)

    def forward(self, x):
        x = self.c0(x)
        x = torch.cat([x, self.c1(torch.tanh(x))], 1)
        x = torch.cat([x, self.c2(torch.relu(x))], 1)
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(torch.tanh(self.bn(x)), 1), 1))


class Growing(nn.Module):
    """torchvision's dense block: every layer reads the concatenation of a growing list of features"""

    def __init__(self):
        super().__init__()
        self.c0 = nn.Conv2d(3, 4, 3, 1, 1)
        self.layers = nn.ModuleList(nn.Conv2d(4 + 2 * i, 2, 3, 1, 1) for i in range(3))
        self.pool, self.fc = nn.AvgPool2d(2), nn.Linear(10 * 4, 3)

    def forward(self, x):
        feats = [self.c0(x)]
        for layer in self.layers:
            feats.append(layer(torch.tanh(torch.cat(feats, 1))))
        return self.fc(self.pool(torch.cat(feats, dim=1)).flatten(1))


class Twice(nn.Module):
    """the same node listed twice (it receives two parts), as a tuple, along dim=-3"""

    def __init__(self):
        super().__init__()
        self.c0, self.c1, self.fc = nn.Conv2d(3, 4, 3, 1, 1), nn.Conv2d(12, 4, 1), nn.Linear(4, 3)

    def forward(self, x):
        a = self.c0(x)
        b = torch.sigmoid(a)
        return self.fc(self.c1(torch.cat((a, b, a), dim=-3)).mean((2, 3)))


class Head(nn.Module):
    """a concatenation of flattened features in the head, with a frozen buffer as a source, in the ``concat`` spelling; and a
    second one along the last dim of a 3-D value in the ``concatenate`` spelling"""

    def __init__(self):
        super().__init__()
        self.c0, self.l1, self.l2, self.fc = nn.Conv2d(3, 4, 3, 1, 1), nn.Linear(4, 5), nn.Linear(4, 2), nn.Linear(10, 3)
        self.register_buffer("extra", torch.linspace(-1, 1, 18).reshape(6, 3))

    def forward(self, x):
        h = torch.flatten(F.adaptive_avg_pool2d(torch.tanh(self.c0(x)), 1), 1)
        u = torch.concat([self.l1(h), self.extra, torch.tanh(self.l2(h))], -1)  # [B, 10]
        v = torch.concatenate([u.view(-1, 2, 5), u.view(-1, 2, 5)], axis=2)  # [B, 2, 10]
        return self.fc(v.mean(1))


MODELS = {"nested": Nested, "growing": Growing, "twice": Twice, "head": Head}


def _build(name):
    torch.manual_seed(3 + len(name))
    m = MODELS[name]().double().eval()
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.3), mod.running_var.uniform_(0.5, 2.0)
            mod.weight.requires_grad_(False), mod.bias.requires_grad_(False)
    return m, torch.randn(6, 3, 4, 4, dtype=torch.float64)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_sweep_matches_one_autograd_pass_per_seed(name):
    """fails without the rule: "no VJP rule for function cat" """
    m64, X = _build(name)
    taps = _taps(m64)
    sweep = SeedBatchedSweep(m64, taps, kernels=None)
    cats = [r for r in sweep.rule.values() if r.kind == CAT]
    assert len(cats) == {"nested": 2, "growing": 4, "twice": 1, "head": 2}[name]
    assert all(isinstance(r.src, tuple) and all(isinstance(a, fx.Node) for a in r.src) for r in cats)
    assert [r.args for r in cats] == {"nested": [(1,), (1,)], "growing": [(1,)] * 4, "twice": [(-3,)], "head": [(-1,), (2,)]}[name]
    if name == "twice":
        assert cats[0].src[0] is cats[0].src[2]
    if name == "head":
        assert sweep.rule[cats[0].src[1]].kind == CONST
    f = sweep.forward(X)
    dims = [sweep.saved[n] for n, r in sweep.rule.items() if r.kind == CAT]
    if name == "twice":
        assert dims == [(1, (4, 4, 4))]  # (the resolved dim and the sizes of the sources along it)
    if name == "head":
        assert dims == [(1, (5, 3, 2)), (2, (5, 5))]
    torch.manual_seed(0)
    seeds = torch.randn(4, *f.shape, dtype=torch.float64)
    grads = sweep.backward(seeds)
    f_ref, ins, want = autograd_reference(m64, taps, X, seeds)
    assert cf.rel(f, f_ref) < 1e-12
    for n in taps:
        assert cf.rel(sweep.taps[n]["a"], ins[n]) < 1e-10, n
        assert cf.rel(grads[n], want[n]) < 1e-10, n


def test_the_default_workload_is_served_by_both_sweeps():
    from laplace_amd.nets import DenseNetSmall
    from tests.emulated_cat_kernels import EmulatedCatKernels

    m = DenseNetSmall().eval()
    assert [m.layers[i][2].out_channels for i in (4, 9)] == [96, 96] and m.fc.in_features == 224
    assert all(mod.in_channels % 32 == 0 and mod.out_channels % 32 == 0 for mod in m.modules()
               if isinstance(mod, nn.Conv2d) and mod.in_channels != 3)
    assert [p.requires_grad for n, p in m.named_parameters() if ".bn" in n or n.startswith("bn")].count(True) == 0
    K = EmulatedCatKernels()
    sw = SplitSweep(m, _taps(m), kernels=lambda: K)
    assert sw.split_ok and sw.split_reason is None
    assert sum(r.kind == CAT for r in sw.rule.values()) == 12


# ---- 2. curvature against the oracle -------------------------------------------------------------------------------------------------
@pytest.fixture
def emulated():
    from tests.emulated_cat_kernels import EmulatedCatKernels

    K = EmulatedCatKernels()
    prev = _lib.set_kernels_for_testing(K)
    yield K
    _lib.set_kernels_for_testing(prev)


@pytest.mark.parametrize("lik", ["classification", "regression"])
def test_curvature_on_the_emulation_matches_the_oracle(lik, emulated):
    got = cf.run_curvature_checks("cpu", lik)
    assert any(s[0] == "vjp" for s in emulated.seen) and any(s[0] == "forward" for s in emulated.seen)
    # the NCHW sweep (rule 1 alone) gives the same numbers
    def off(b):
        b.use_split_sweep = False

    ref = cf.run_curvature_checks("cpu", lik, configure=off, want_split=False)
    for k in ("Js", "f", "h", "f_var"):
        assert cf.rel(got[k], ref[k]) < 1e-4, k


def test_the_switch_sends_the_model_to_the_nchw_sweep(emulated, monkeypatch):
    monkeypatch.setattr(SplitSweep, "nhwc_cat", False)
    cf.run_curvature_checks("cpu", "classification", want_split=False)
    m64, _ = cf.small_dense(3)
    sw = SplitSweep(m64.float(), _taps(m64), kernels=get_kernels)
    assert not sw.split_ok and sw.split_reason == "cat: cat has no NHWC rule"


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------------------
def _cat_node(args, kwargs=None, target=torch.cat):
    g = fx.Graph()
    x = g.placeholder("x")
    resolve = lambda a: x if a == "x" else a  # noqa: E731
    args = tuple([resolve(t) for t in a] if isinstance(a, list) else resolve(a) for a in args)
    return g.call_function(target, args, {k: resolve(v) for k, v in (kwargs or {}).items()}), x


@pytest.mark.parametrize("args,kwargs,fragment", [
    ((["x", "x"], 0), None, "along dim 0 (the batch dim"),
    ((["x", "x"],), None, "along dim 0 (the batch dim"),  # (torch's default)
    ((["x", 2.0], 1), None, "an entry of the list is not a traced tensor (float"),
    ((["x", torch.zeros(1)], 1), None, "an entry of the list is not a traced tensor (Tensor"),
    ((["x", "x"], "x"), None, "data-dependent dim"),
    ((["x", "x"],), {"dim": "x"}, "data-dependent dim"),
    ((["x", "x"], 1), {"out": "x"}, "out= argument"),
    (("x", 1), None, "non-empty list or tuple"),
    (([], 1), None, "non-empty list or tuple"),
], ids=["dim0", "default-dim", "python-constant", "tensor-literal", "node-dim", "node-dim-kw", "out", "not-a-list", "empty"])
def test_classify_refuses_by_name(args, kwargs, fragment):
    for target in (torch.cat, torch.concat, torch.concatenate):
        node, _ = _cat_node(args, kwargs, target)
        with pytest.raises(SweepUnsupported, match="(cat|concat|concatenate).*" + fragment.replace("(", r"\(")):
            classify(node, {})
    node, x = _cat_node((["x", "x"],), {"dim": -1})
    r = classify(node, {})
    assert isinstance(r, Rule) and r.kind == CAT and r.src == (x, x) and r.args == (-1,) and r.fn is torch.cat


class _Refused(nn.Module):
    def __init__(self, how):
        super().__init__()
        self.how = how
        self.c0, self.c1 = nn.Conv2d(3, 32, 3, 1, 1), nn.Conv2d({"mixed": 34, "batch-dim": 32}.get(how, 64), 32, 3, 1, 1)
        self.fc = nn.Linear(32, 3)
        self.register_buffer("buf", torch.zeros(2, 64, 4, 4))

    def forward(self, x):
        how = self.how
        a = self.c0(x)
        b = torch.tanh(a)
        if how == "batch-dim":  # dim -4 of a 4-D value is the batch dim: only the value tells
            c = torch.cat([a, b], -4).view(2, -1, 32, 4, 4).mean(0)
        elif how == "out":
            c = torch.cat([a, b], 1, out=self.buf)
        elif how == "height":
            c = torch.cat([a, b], 2).view(-1, 64, 4, 4)
        elif how == "mixed":
            t = torch.flatten(F.adaptive_avg_pool2d(a, 1), 1).view(-1, 2, 4, 4)
            c = torch.cat([a, t], 1)
        else:
            c = torch.cat([a, b], 1)
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(self.c1(c), 1), 1))


def _tape_answers(model, X, fragment):
    """the backend falls to the tape with the refusal as its reason, and gives the oracle's numbers"""
    from laplace_amd import HipGGN
    from oracle import curvature_oracle as co
    from tests.emulated_cat_kernels import EmulatedCatKernels

    prev = _lib.set_kernels_for_testing(EmulatedCatKernels())
    try:
        backend = HipGGN(model, "classification")
        Js, f = backend.jacobians(X)
        assert fragment in backend._tape().sweep_reason
    finally:
        _lib.set_kernels_for_testing(prev)
    Js64, f64 = co.jacobians(copy.deepcopy(model).double(), X.double())
    assert cf.rel(f, f64) < 1e-5 and cf.rel(Js, Js64) < 1e-4


def test_a_dim_that_resolves_to_the_batch_dim_is_refused_on_the_value_and_the_tape_answers():
    torch.manual_seed(1)
    model, X = _Refused("batch-dim").eval(), torch.randn(2, 3, 4, 4)
    sweep = SeedBatchedSweep(model, _taps(model), kernels=None)  # (-4 is a static dim: `classify` lets it through)
    with pytest.raises(SweepUnsupported, match=r"cat along dim -4 of a value with 4 dims \(the batch dim"):
        sweep.forward(X)
    _tape_answers(model, X, "the batch dim")


def test_an_out_argument_is_refused_at_construction():
    with pytest.raises(SweepUnsupported, match="cat with an out= argument"):
        SeedBatchedSweep(_Refused("out").eval(), {}, kernels=None)


def _nchw_route(model, kernels, hw=4):
    """a model the split sweep refuses: the reason, and the NCHW walk's numbers against one autograd pass per seed"""
    taps = _taps(model)
    sw = SplitSweep(model, taps, kernels=kernels)
    assert not sw.split_ok
    x, seeds = torch.randn(2, 3, hw, hw), torch.randn(2, 2, 3)
    f = sw.forward(x)
    grads = sw.backward(seeds)
    f_ref, _, want = autograd_reference(model, taps, x, seeds)
    assert torch.allclose(f, f_ref, rtol=1e-4, atol=1e-6)
    for n in taps:
        assert torch.allclose(grads[n], want[n], rtol=1e-4, atol=1e-6), n
    return sw.split_reason


def test_eligibility_refusals_name_their_node_and_keep_the_nchw_route(emulated):
    torch.manual_seed(2)
    assert _nchw_route(_Refused("height").eval(), get_kernels) == \
        "cat: cat of feature maps along dim 2 (the NHWC kernels concatenate channels: dim 1 of a 4-D map)"
    assert _nchw_route(_Refused("mixed").eval(), get_kernels) == "cat: cat of feature maps with tensors outside the feature maps"
    assert SplitSweep(_Refused("plain").eval(), _taps(_Refused("plain")), kernels=get_kernels).split_ok


@pytest.mark.parametrize("missing", ("cat_forward", "cat_vjp"))
def test_split_sweep_wants_both_entry_points(missing, emulated):
    def absent(self):
        raise AttributeError(missing)

    K = type("OneEntryPoint", (type(emulated),), {missing: property(absent)})()
    assert not hasattr(K, missing)
    assert _nchw_route(_Refused("plain").eval(), lambda: K) == "cat: kernels without the concatenation entry points"


def test_the_pooling_emulation_keeps_a_concatenating_model_on_the_nchw_route():
    from tests.emulated_pool_kernels import EmulatedPoolKernels

    K = EmulatedPoolKernels()
    assert "kernels without the concatenation entry points" in _nchw_route(_Refused("plain").eval(), lambda: K)


def test_a_head_concatenation_takes_the_parent_math_on_the_split_sweep(emulated):
    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.c0, self.l1, self.fc = nn.Conv2d(3, 32, 3, 1, 1), nn.Linear(32, 4), nn.Linear(36, 3)

        def forward(self, x):
            h = torch.flatten(F.adaptive_avg_pool2d(torch.relu(self.c0(x)), 1), 1)
            return self.fc(torch.cat([h, torch.tanh(self.l1(h))], -1))

    torch.manual_seed(5)
    m64 = M().double().eval()
    model = copy.deepcopy(m64).float()
    taps = _taps(model)
    sw = SplitSweep(model, taps, kernels=get_kernels)
    assert sw.split_ok, sw.split_reason
    X, seeds = torch.randn(3, 3, 4, 4, dtype=torch.float64), torch.randn(2, 3, 3, dtype=torch.float64)
    f = sw.forward(X.float())
    grads = sw.backward(seeds.float())
    assert not emulated.seen  # (no kernel of lk_cat.hip: plain tensors)
    f64, ins, want = autograd_reference(m64, _taps(m64), X, seeds)
    assert cf.rel(f, f64) < 1e-5
    for n in taps:
        assert cf.rel(grads[n], want[n]) < 1e-4, n


# ---- 4. the kernel branch of the split sweep's rule on the emulation ------------------------------------------------------------------
def test_the_small_densenet_runs_the_kernel_branch_and_matches_float64_autograd(emulated):
    m64, X, _ = cf.e2e_fixture("tanh")
    model = copy.deepcopy(m64).float()
    taps = cf.e2e_taps(model)
    sw = SplitSweep(model, taps, kernels=get_kernels)
    assert sw.split_ok, sw.split_reason
    outs = {}
    inner = sw._run_cat
    sw._run_cat = lambda node, r, ts, dim, _i=inner: outs.setdefault(node, (_i(node, r, ts, dim), ts))[0]
    seeds = torch.randn(3, 4, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    f = sw.forward(X.float())
    grads = sw.backward(seeds.float())
    # layouts: NHWC memory in (a view, no copy), ONE NHWC allocation out, returned as the NCHW-logical view
    for out, ts in outs.values():
        assert is_channels_last(out) and out.shape[1] == sum(t.shape[1] for t in ts)
    fwd = [s for s in emulated.seen if s[0] == "forward"]
    vjp = [s for s in emulated.seen if s[0] == "vjp"]
    assert fwd == [("forward", (64, 32)), ("forward", (96, 32))] * 2  # (one call per node: stem + layer, then + layer)
    # per node one launch per source, each with a max|.| word; the inner node's cotangent arrives as the outer one's fp32 slice
    # beside the split tensor of the layer that reads it
    assert vjp == [("vjp", ("split",), 0, 96, True), ("vjp", ("split",), 96, 32, True),
                   ("vjp", ("f32", "split"), 0, 64, True), ("vjp", ("f32", "split"), 64, 32, True)] * 2
    f64, ins, want = autograd_reference(m64, cf.e2e_taps(m64), X, seeds)
    assert cf.rel(f, f64) < 1e-5
    for n in taps:
        assert cf.rel(sw.taps[n]["a"], ins[n]) < 1e-5, n
        assert grads[n].shape == want[n].shape and cf.rel(grads[n], want[n]) < 1e-4, (n, cf.rel(grads[n], want[n]))


def test_the_concatenation_inherits_the_element_wise_maximum_of_its_sources_bounds(emulated):
    class M(nn.Module):
        def __init__(self, second_is_conv):
            super().__init__()
            self.second_is_conv = second_is_conv
            self.c1, self.b1 = nn.Conv2d(3, 32, 3, 1, 1, bias=False), nn.BatchNorm2d(32)
            self.c2, self.b2 = nn.Conv2d(32, 32, 3, 1, 1, bias=False), nn.BatchNorm2d(32)
            self.c3, self.fc = nn.Conv2d(64, 32, 3, 1, 1), nn.Linear(32, 3)

        def forward(self, x):
            a = torch.relu(self.b1(self.c1(x)))
            b = self.c2(a)
            if not self.second_is_conv:
                b = torch.relu(self.b2(b))
            return self.fc(torch.flatten(F.adaptive_avg_pool2d(self.c3(torch.cat([a, b], 1)), 1), 1))

    for second_is_conv in (False, True):
        torch.manual_seed(4)
        m = M(second_is_conv).eval()
        with torch.no_grad():
            m.b2.weight.mul_(3.0)  # (the second source is the larger one on some images)
        sw = SplitSweep(m, _taps(m), kernels=get_kernels)
        assert sw.split_ok, sw.split_reason
        seen = {}
        inner = sw._run_cat

        def spy(node, r, ts, dim, _inner=inner, _sw=sw, _seen=seen):
            out = _inner(node, r, ts, dim)
            _seen["in"], _seen["out"] = [_sw._aux_get(t) for t in ts], _sw._aux_get(out)
            return out

        sw._run_cat = spy
        x = torch.randn(3, 3, 8, 8)
        f = sw.forward(x)
        assert torch.allclose(f, m(x), rtol=1e-4, atol=1e-5)
        assert seen["in"][0] is not None and seen["in"][0].get("bound") is not None
        if second_is_conv:  # (a convolution's output carries no measured bound: nothing is inherited)
            assert seen["out"] is None
        else:
            want = torch.maximum(seen["in"][0]["bound"], seen["in"][1]["bound"])
            assert torch.equal(seen["out"]["bound"], want) and seen["out"]["split"] is None
            assert not torch.equal(want, seen["in"][0]["bound"]) and tuple(want.shape) == (3,)


def test_more_than_four_parts_are_folded_through_fp32(emulated):
    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.c0 = nn.Conv2d(3, 32, 3, 1, 1)
            self.bns = nn.ModuleList(nn.BatchNorm2d(64) for _ in range(6))
            self.convs = nn.ModuleList(nn.Conv2d(64, 32, 1, bias=False) for _ in range(6))
            self.fc = nn.Linear(32, 3)

        def forward(self, x):
            a = self.c0(x)
            c = torch.cat([a, torch.tanh(a)], 1)
            out = self.convs[0](torch.tanh(self.bns[0](c)))
            for bn, conv in zip(self.bns[1:], self.convs[1:]):
                out = out + conv(torch.tanh(bn(c)))
            return self.fc(torch.flatten(F.adaptive_avg_pool2d(out, 1), 1))

    torch.manual_seed(6)
    m64 = M().double().eval()
    for bn in m64.bns:
        bn.running_mean.normal_(0, 0.3), bn.running_var.uniform_(0.5, 2.0)
        bn.weight.requires_grad_(False), bn.bias.requires_grad_(False)
    model = copy.deepcopy(m64).float()
    taps = _taps(model)
    sw = SplitSweep(model, taps, kernels=get_kernels)
    assert sw.split_ok, sw.split_reason
    X, seeds = torch.randn(2, 3, 4, 4, dtype=torch.float64), torch.randn(2, 2, 3, dtype=torch.float64)
    f = sw.forward(X.float())
    grads = sw.backward(seeds.float())
    vjp = [s for s in emulated.seen if s[0] == "vjp"]
    # six consumers: three split parts as they are and the other three folded into one fp32 tensor, one launch per source
    assert vjp == [("vjp", ("split", "split", "split", "f32"), 0, 32, True), ("vjp", ("split", "split", "split", "f32"), 32, 32, True)]
    f64, _, want = autograd_reference(m64, _taps(m64), X, seeds)
    assert cf.rel(f, f64) < 1e-5
    for n in taps:
        assert cf.rel(grads[n], want[n]) < 1e-4, (n, cf.rel(grads[n], want[n]))


def test_an_inference_only_forward_keeps_nothing(emulated):
    m64, X, _ = cf.e2e_fixture("tanh")
    model = copy.deepcopy(m64).float()
    sw = SplitSweep(model, cf.e2e_taps(model), kernels=get_kernels)
    f = sw.forward(X.float(), need_vjp=False)
    assert sw.saved == {} and cf.rel(f, m64(X).detach()) < 1e-5
