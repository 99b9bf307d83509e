"""The per-node rule table of the sweeps (laplace_amd/sweep.py, `classify`): every spelling of an operation that the
whitelist admits gets the same record, so the spellings run the same arithmetic in `forward` and `backward` (bit for bit)
and agree with one autograd pass per seed; what has no rule is refused before `backward` can hand a gradient over."""
import functools

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from laplace_amd import sweep as sw_mod
from laplace_amd.sweep import SeedBatchedSweep, SweepUnsupported


def _iadd(a, b):
    a += b
    return a


# operation -> (kind, flavour, the spellings as callables of (the module spelling's module, input); the first is the reference)
_OPS = {
    "relu": (sw_mod.ACT, "relu", nn.ReLU(), [lambda m, x: m(x), lambda m, x: torch.relu(x), lambda m, x: F.relu(x),
                                             lambda m, x: x.relu()]),
    "tanh": (sw_mod.ACT, "tanh", nn.Tanh(), [lambda m, x: m(x), lambda m, x: torch.tanh(x), lambda m, x: x.tanh()]),
    "sigmoid": (sw_mod.ACT, "sigmoid", nn.Sigmoid(), [lambda m, x: m(x), lambda m, x: torch.sigmoid(x),
                                                      lambda m, x: x.sigmoid()]),
    "gelu": (sw_mod.ACT, "generic", nn.GELU(), [lambda m, x: m(x), lambda m, x: F.gelu(x)]),
    "flatten": (sw_mod.RESHAPE, None, nn.Flatten(), [lambda m, x: m(x), lambda m, x: torch.flatten(x, 1),
                                                     lambda m, x: x.flatten(1), lambda m, x: x.view(x.size(0), -1),
                                                     lambda m, x: x.reshape(x.size(0), -1)]),
    "adaptive_pool": (sw_mod.GPOOL, None, nn.AdaptiveAvgPool2d(2), [lambda m, x: m(x), lambda m, x: F.adaptive_avg_pool2d(x, 2)]),
    "avg_pool": (sw_mod.AVGPOOL, None, nn.AvgPool2d(2), [lambda m, x: m(x), lambda m, x: F.avg_pool2d(x, 2)]),
    "max_pool": (sw_mod.MAXPOOL, None, nn.MaxPool2d(2), [lambda m, x: m(x), lambda m, x: F.max_pool2d(x, 2)]),
    "mean": (sw_mod.MEAN, None, None, [lambda m, x: torch.mean(x, (2, 3)), lambda m, x: x.mean((2, 3))]),
    "add": (sw_mod.ADD, None, None, [lambda m, x: x[0] + x[1], lambda m, x: torch.add(x[0], x[1]), lambda m, x: _iadd(x[0], x[1])]),
}
_CASES = [(name, i) for name, op in _OPS.items() for i in range(len(op[3]))]


class Net(nn.Module):
    """conv 3 -> 8, activation, pool, flatten, Linear to 3 outputs: the operation under test replaces its stage (an add
    joins a second convolution's output with the activation, torchvision style, between activation and pool)"""

    def __init__(self, op, spelling, conv, conv2, fc):
        super().__init__()
        self.conv, self.conv2, self.fc = conv, conv2, fc
        self.stage = {"relu": "act", "tanh": "act", "sigmoid": "act", "gelu": "act", "flatten": "flat", "add": "add"}.get(op, "pool")
        self.mod, self.fn = _OPS[op][2], _OPS[op][3][spelling]

    def forward(self, x):
        h = self.fn(self.mod, self.conv(x)) if self.stage == "act" else torch.relu(self.conv(x))
        if self.stage == "add":
            h = self.fn(self.mod, (self.conv2(h), h))
        h = self.fn(self.mod, h) if self.stage == "pool" else F.max_pool2d(h, 2)
        h = self.fn(self.mod, h) if self.stage == "flat" else torch.flatten(h, 1)
        return self.fc(h)


@functools.lru_cache(None)
def _shared(op):
    """what the twins of an operation share: weights, input, seeds"""
    torch.manual_seed(len(op))
    return nn.Conv2d(3, 8, 3), nn.Conv2d(8, 8, 3, padding=1), nn.LazyLinear(3), torch.randn(2, 3, 8, 8), torch.randn(3, 2, 3)


@functools.lru_cache(None)
def _run(op, spelling):
    """one twin through the sweep (computed once: the module spelling is every other twin's reference)"""
    conv, conv2, fc, x, seeds = _shared(op)
    model = Net(op, spelling, conv, conv2, fc).eval()
    with torch.no_grad():
        model(x)  # (materialises the lazy Linear on the reference twin)
    taps = {"conv": conv, "fc": fc, **({"conv2": conv2} if op == "add" else {})}
    sw = SeedBatchedSweep(model, taps)
    f = sw.forward(x)
    return model, taps, sw, f, sw.backward(seeds), x, seeds


@pytest.mark.parametrize("op,spelling", _CASES, ids=[f"{n}-{i}" for n, i in _CASES])
def test_every_spelling_gets_the_same_rule_and_runs_the_same_arithmetic(op, spelling):
    kind, flavour = _OPS[op][:2]
    model, taps, sw, f, grads, x, seeds = _run(op, spelling)
    rules = [r for r in sw.rule.values() if r.kind == kind and r.flavour == flavour]
    assert len(rules) == 1, [(r.kind, r.flavour) for r in sw.rule.values()]
    _, _, sw0, f0, grads0, _, _ = _run(op, 0)
    assert torch.equal(f, f0)
    for n in taps:
        assert torch.equal(sw.taps[n]["a"], sw0.taps[n]["a"]), n
        assert torch.equal(grads[n], grads0[n]), n
    if spelling == 0:  # the reference twin against one autograd pass per seed
        outs = {}
        hooks = [m.register_forward_hook(lambda m_, i, o, n=n: outs.__setitem__(n, o)) for n, m in taps.items()]
        f_ref = model(x)
        for h in hooks:
            h.remove()
        assert torch.allclose(f, f_ref, rtol=1e-4, atol=1e-7)
        for s in range(seeds.shape[0]):
            want = torch.autograd.grad(f_ref, [outs[n] for n in taps], grad_outputs=seeds[s], retain_graph=True)
            for n, w in zip(taps, want):
                assert torch.allclose(grads[n][s], w, rtol=1e-4, atol=1e-7), n


class _Mul(nn.Module):
    def forward(self, x):
        return self.fc(x * 2.0)


class _AddAlpha(nn.Module):
    def forward(self, x):
        h = self.fc(x)
        return torch.add(h, h, alpha=2)


class _GetAttr(nn.Module):
    def forward(self, x):
        return self.fc(x) + self.fc.bias


class _TwoInputs(nn.Module):
    def forward(self, x, y):
        return self.fc(x) + self.fc(y)


class _ReturnIndices(nn.Module):
    def forward(self, x):
        return self.fc(F.max_pool2d(x.view(-1, 1, 2, 2), 1, return_indices=True)[0].flatten(1))


@pytest.mark.parametrize("cls", [_Mul, _AddAlpha, _GetAttr, _TwoInputs, _ReturnIndices])
def test_graphs_without_a_rule_are_refused_before_backward(cls):
    """statically refusable graphs raise at construction or in `forward`: `backward` (which hands gradients to `on_tap` as it
    goes) is never reached"""
    model = cls()
    model.fc = nn.Linear(4, 3)
    model(*[torch.randn(2, 4)] * (2 if cls is _TwoInputs else 1))  # (the model itself is fine)
    with pytest.raises(SweepUnsupported):
        SeedBatchedSweep(model.eval(), {"fc": model.fc}).forward(torch.randn(2, 4))


def test_adaptive_pooling_to_several_cells_keeps_the_nhwc_walk_off_in_either_spelling():
    """the NHWC walk's pooling rule serves pooling to ONE cell: a larger output size must turn the walk off on the graph
    alone, whichever way the pooling is written (the functional spelling used to get past the check)"""
    from laplace_amd import _lib
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep_nhwc import SplitSweep
    from tests.emulated_kernels import EmulatedKernels

    class M(nn.Module):
        def __init__(self, functional):
            super().__init__()
            self.c, self.pool, self.fc, self.functional = nn.Conv2d(32, 32, 3, 1, 1, bias=False), nn.AdaptiveAvgPool2d(2), nn.Linear(128, 3), functional

        def forward(self, x):
            h = torch.relu(self.c(x))
            return self.fc(torch.flatten(F.adaptive_avg_pool2d(h, 2) if self.functional else self.pool(h), 1))

    prev = _lib.set_kernels_for_testing(EmulatedKernels())
    try:
        for functional in (False, True):
            m = M(functional).eval()
            s = SplitSweep(m, {"c": m.c, "fc": m.fc}, kernels=get_kernels)
            assert not s.split_ok and "adaptive pooling to more than one cell" in s.split_reason
    finally:
        _lib.set_kernels_for_testing(prev)


# ---- the rule tables of the two reverse walks (``SeedBatchedSweep._VJP``; ``SplitSweep._NHWC_VJP`` and the head-region fallback) ----
# every kind constant of sweep.py (its public upper-case strings), and the two fx ops that are their own kind
KINDS = sorted(v for k, v in vars(sw_mod).items() if k.isupper() and not k.startswith("_") and isinstance(v, str)) + ["placeholder", "output"]


def test_every_kind_has_an_entry_in_the_parents_table():
    assert len(KINDS) == 28 and len(set(KINDS)) == 28  # (26 constants: a new one is found by name, not listed here)
    table = SeedBatchedSweep._VJP
    assert set(KINDS) <= set(table), sorted(set(KINDS) - set(table))
    for kind, name in table.items():  # a method that exists, or the explicit "no cotangent by design"
        assert name is None or callable(getattr(SeedBatchedSweep, name)), (kind, name)
    assert {k for k, name in table.items() if name is None} == {sw_mod.SIZE, sw_mod.GETITEM, sw_mod.SPLIT, sw_mod.CONST, "placeholder", "output"}


def test_every_kind_the_nhwc_walk_can_meet_is_served_or_falls_back():
    """a kind with a cotangent that `_split_eligible` does not send to the NCHW sweep has an NHWC rule or the parent's in the head"""
    from laplace_amd import sweep_nhwc
    from laplace_amd.sweep_nhwc import SplitSweep

    for kind in KINDS:
        if SeedBatchedSweep._VJP[kind] is None or kind in sweep_nhwc._NO_RULE:
            continue
        assert kind in SplitSweep._NHWC_VJP or kind in sweep_nhwc._HEAD, kind
    for name in SplitSweep._NHWC_VJP.values():
        assert callable(getattr(SplitSweep, name)), name
    # the fallback calls the parent's rule of the kind: it has one; and what it refuses by name is what the NHWC table lacks
    assert all(SeedBatchedSweep._VJP[k] is not None for k in sweep_nhwc._HEAD)
    assert {k for k, why in sweep_nhwc._HEAD.items() if why is None} == set(sweep_nhwc._HEAD) & set(SplitSweep._NHWC_VJP) - {sw_mod.MUL}


def test_an_unknown_kind_is_refused_by_name_instead_of_dropping_the_cotangent():
    """before the table the walk's ``if / elif`` chain had no ``else``: the cotangent was dropped and this passed silently"""
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(6, 5), nn.Tanh(), nn.Linear(5, 3)).eval()
    sw = SeedBatchedSweep(model, {"0": model[0], "2": model[2]})
    f = sw.forward(torch.randn(2, 6))
    act = next(n for n, r in sw.rule.items() if r.kind == sw_mod.ACT)
    sw.rule[act] = sw.rule[act]._replace(kind="invented", what="frobnicate")
    with pytest.raises(SweepUnsupported, match="frobnicate"):
        sw.backward(torch.randn(3, *f.shape))


def test_a_walk_that_raises_leaves_no_state_on_the_sweep():
    """a `SplitSweep.backward` that is refused mid-walk keeps nothing of that walk on the object (it used to keep the closure over
    its device words and the multiplier cache), and the next walk on it returns the bits of a fresh sweep"""
    from laplace_amd import _lib
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep_nhwc import SplitSweep
    from tests.emulated_kernels import EmulatedKernels
    from tests.test_sweep_nhwc import _model

    prev = _lib.set_kernels_for_testing(EmulatedKernels())
    try:
        model = _model(torch.relu)
        taps = {n: m for n, m in model.named_modules() if isinstance(m, (nn.Conv2d, nn.Linear))}
        torch.manual_seed(1)
        x, seeds = torch.randn(2, 3, 8, 8), torch.randn(3, 2, 5)
        sw = SplitSweep(model, taps, kernels=get_kernels)
        assert sw.split_ok, sw.split_reason
        sw.forward(x)
        before = set(vars(sw))
        # the last residual join receives the split cotangent of the activation behind it: as a reshape it is refused mid-walk
        join = [n for n, r in sw.rule.items() if r.kind == sw_mod.ADD][-1]
        rule = sw.rule[join]
        sw.rule[join] = rule._replace(kind=sw_mod.RESHAPE)
        with pytest.raises(SweepUnsupported, match="reshape inside the NHWC region"):
            sw.backward(seeds)
        sw.rule[join] = rule
        assert set(vars(sw)) - before <= {"grad_scale"}, sorted(set(vars(sw)) - before)
        assert not any(isinstance(v, sw_mod._Walk) or getattr(v, "__closure__", None) for v in vars(sw).values())
        fresh = SplitSweep(model, taps, kernels=get_kernels)
        fresh.forward(x)
        for defer in (False, True):
            got, want = sw.backward(seeds, defer_bn_scale=defer), fresh.backward(seeds, defer_bn_scale=defer)
            assert list(got) == list(want) and all(torch.equal(got[n], want[n]) for n in want)
            assert list(sw.grad_scale) == list(fresh.grad_scale)
    finally:
        _lib.set_kernels_for_testing(prev)
