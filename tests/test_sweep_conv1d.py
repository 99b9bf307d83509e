"""1-D convolutional networks on the CPU: ``nn.Conv1d``, the 1-D pools and the reductions these networks end in (``amax``,
``max(dim)[0]``, ``sum(dim)``, the adaptive max pools) go through ONE seed-batched sweep for all seeds and match one autograd pass per
seed - on the torch math of the rules and on the emulation of csrc/lk_reduce.hip (tests/emulated_reduce_kernels.py); ``HipGGN``
serves such a model as the unit-height Conv2d network it equals (``laplace_amd.conv.lift``), against the fp64 oracle, on the sweep and
on the autograd tape; what the rules do not serve is refused by name and the backend answers through the tape.

Before this existed the sweep refused every model here with "no VJP rule for module Conv1d", ``HipGGN._supported()`` was ``False``
(``jacobians`` / ``diag`` / ``full`` took the generic ``torch.func`` route) and ``kron`` raised ``NotImplementedError``."""
import copy

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from laplace_amd import _lib
from laplace_amd.sweep import _MAXRED, _SUMRED, CONV, IDENTITY, SeedBatchedSweep, SweepUnsupported, reduce_geometry
from laplace_amd.sweep_nhwc import SplitSweep
from tests import conv1d_fixtures as cf
from tests.norm_sweep_fixtures import autograd_reference


@pytest.fixture
def emulated():
    from tests.emulated_reduce_kernels import EmulatedReduceKernels

    K = EmulatedReduceKernels()
    prev = _lib.set_kernels_for_testing(K)
    yield K
    _lib.set_kernels_for_testing(prev)


class Net(nn.Module):
    """Conv1d - BatchNorm1d - tanh - max pools (module and functional) - a strided dilated Conv1d - a depthwise one - an average
    pool - ``head(x)`` - Linear; the BatchNorm sits in a residual join, so that the fused BN / add / activation VJP runs on
    ``[B, C, L]`` maps"""

    def __init__(self, head):
        super().__init__()
        self.c1, self.bn = nn.Conv1d(3, 4, 3, 1, 1), nn.BatchNorm1d(4)
        self.c0, self.bn0, self.relu = nn.Conv1d(4, 4, 1, bias=False), nn.BatchNorm1d(4), nn.ReLU()
        self.c2, self.dw = nn.Conv1d(4, 6, 3, 2, 2, dilation=2), nn.Conv1d(6, 6, 3, 1, 1, groups=6)
        self.mp, self.ap, self.gp, self.amp = nn.MaxPool1d(3, 2, 1), nn.AvgPool1d(2), nn.AdaptiveAvgPool1d(3), nn.AdaptiveMaxPool1d(1)
        self.amp2 = nn.AdaptiveMaxPool2d((1, 1))
        self.fc = nn.Linear(6, 3)
        self.head = head

    def forward(self, x):
        x = torch.tanh(self.bn(self.c1(x)))
        x = self.relu(self.bn0(self.c0(x)) + x)
        x = self.mp(x) + F.max_pool1d(x, 3, 2, 1)
        x = self.dw(self.c2(x))
        x = F.avg_pool1d(x, 1) + x
        return self.fc(self.head(self, x))


# every spelling of the reductions and the 1-D pools: name -> (head, kinds of the reduction nodes)
SPELLINGS = {
    "x.amax(2)": (lambda m, x: x.amax(2), [_MAXRED]),
    "torch.amax(x, dim=-1, keepdim=True)": (lambda m, x: torch.amax(x, dim=-1, keepdim=True).flatten(1), [_MAXRED]),
    "x.amax((1, 2)) of a 4-D view": (lambda m, x: x.view(x.size(0), 6, 2, -1).amax((-1, 2)), [_MAXRED]),
    "x.max(2)[0]": (lambda m, x: x.max(2)[0], [_MAXRED]),
    "torch.max(x, 2).values": (lambda m, x: torch.max(x, 2).values, [_MAXRED]),
    "torch.max(x, dim=2)[0]": (lambda m, x: torch.max(x, dim=2)[0], [_MAXRED]),
    "x.max(dim=2, keepdim=True)[0]": (lambda m, x: x.max(dim=2, keepdim=True)[0].flatten(1), [_MAXRED]),
    "x.transpose(1, 2).max(1)[0] (positions before channels)": (lambda m, x: x.transpose(1, 2).max(1)[0], [_MAXRED]),
    "x.transpose(1, 2).amax(-2)": (lambda m, x: x.transpose(1, 2).amax(-2), [_MAXRED]),
    "nn.AdaptiveMaxPool1d(1)": (lambda m, x: m.amp(x).flatten(1), [_MAXRED]),
    "F.adaptive_max_pool1d(x, 1)": (lambda m, x: F.adaptive_max_pool1d(x, 1).flatten(1), [_MAXRED]),
    "nn.AdaptiveMaxPool2d((1, 1))": (lambda m, x: m.amp2(x.view(x.size(0), 6, 2, -1)).flatten(1), [_MAXRED]),
    "F.adaptive_max_pool2d(x, 1)": (lambda m, x: F.adaptive_max_pool2d(x.view(x.size(0), 6, 2, -1), 1).flatten(1), [_MAXRED]),
    "x.sum(2)": (lambda m, x: x.sum(2), [_SUMRED]),
    "torch.sum(x, (2,), keepdim=True)": (lambda m, x: torch.sum(x, (2,), keepdim=True).flatten(1), [_SUMRED]),
    "x.sum((1, 3)) of a 4-D view": (lambda m, x: x.view(x.size(0), 2, 6, -1).sum((1, 3)), [_SUMRED]),
    "1-D average pools": (lambda m, x: m.gp(x).amax(2) + F.adaptive_avg_pool1d(x, 1).flatten(1) + m.ap(x).sum(-1)
                          + F.avg_pool1d(x, 3, 1, 1, False, False).amax(2), [_MAXRED, _SUMRED, _MAXRED]),
}


def _net(head, dtype):
    torch.manual_seed(7)
    m = Net(head).to(dtype).eval()
    for bn in (m.bn, m.bn0):
        bn.running_mean.normal_(0, 0.3), bn.running_var.uniform_(0.5, 2.0)
    return m, torch.randn(5, 3, 16, dtype=dtype)


def _taps(model):
    return {n: m for n, m in model.named_modules() if isinstance(m, (nn.Linear, nn.Conv1d, nn.Conv2d))}


def _against_autograd(m, X, kernels, S=4):
    taps = _taps(m)
    sweep = SeedBatchedSweep(m, taps, kernels=kernels)
    f = sweep.forward(X)
    torch.manual_seed(0)
    seeds = torch.randn(S, *f.shape, dtype=X.dtype)
    grads = sweep.backward(seeds)
    f_ref, ins, want = autograd_reference(m, taps, X, seeds)
    assert torch.allclose(f, f_ref.detach(), rtol=1e-4, atol=1e-7)
    for n in taps:
        # (the fused BatchNorm / activation kernel of the emulation rounds differently from the module: the last bit)
        assert torch.equal(sweep.taps[n]["a"], ins[n]) if kernels is None else torch.allclose(sweep.taps[n]["a"], ins[n], rtol=1e-4, atol=1e-7), n
        assert grads[n].shape == want[n].shape, n
        assert torch.allclose(grads[n], want[n], rtol=1e-4, atol=1e-7), (n, (grads[n] - want[n]).abs().max())
    return sweep


@pytest.mark.parametrize("name", sorted(SPELLINGS))
def test_sweep_matches_one_autograd_pass_per_seed(name):
    """fails without the rules: "no VJP rule for module Conv1d (c1)" at construction"""
    head, kinds = SPELLINGS[name]
    sweep = _against_autograd(*_net(head, torch.float64), kernels=None)
    assert [r.kind for r in sweep.rule.values() if r.kind in (_MAXRED, _SUMRED)] == kinds
    assert sum(r.kind == CONV for r in sweep.rule.values()) == 4
    assert sum(r.flavour == "1d" for r in sweep.rule.values()) >= 3  # (the 1-D pools are lifted at their nodes)


@pytest.mark.parametrize("name", sorted(SPELLINGS))
def test_sweep_on_the_emulation_matches_autograd(name, emulated):
    head, kinds = SPELLINGS[name]
    _against_autograd(*_net(head, torch.float32), kernels=_lib.get_kernels)
    calls = [s for s in emulated.seen if s[0].startswith("maxred")]
    assert bool(calls) == (_MAXRED in kinds)
    if "amax" in name:
        assert ("maxred_vjp", "even") in {s[:2] for s in calls}
    if ".max(" in name or "adaptive_max" in name.lower() or "AdaptiveMax" in name:
        assert ("maxred_vjp", "first") in {s[:2] for s in calls}


def test_the_switch_keeps_the_rule_on_torch_math(emulated, monkeypatch):
    monkeypatch.setattr(SeedBatchedSweep, "use_reduce_kernels", False)
    _against_autograd(*_net(SPELLINGS["x.amax(2)"][0], torch.float32), kernels=_lib.get_kernels)
    assert not any(s[0].startswith("maxred") for s in emulated.seen)
    emulated.seen.clear()
    monkeypatch.setattr(SeedBatchedSweep, "use_reduce_kernels", True)
    _against_autograd(*_net(SPELLINGS["x.amax(2)"][0], torch.float64), kernels=_lib.get_kernels)  # (not fp32: the torch math)
    assert not any(s[0].startswith("maxred") for s in emulated.seen)


class Ties(nn.Module):
    """a clamp makes whole runs of positions equal: ``max(dim)`` owes the cotangent to the FIRST maximum, ``amax`` an even split"""

    def __init__(self, head):
        super().__init__()
        self.c1, self.act, self.fc, self.head = nn.Conv1d(3, 4, 3, 1, 1), nn.Hardtanh(-0.1, 0.1), nn.Linear(4, 3), head

    def forward(self, x):
        return self.fc(self.head(self.act(self.c1(x))))


@pytest.mark.parametrize("head", [lambda x: x.max(2)[0], lambda x: x.amax(2), lambda x: F.adaptive_max_pool1d(x, 1).flatten(1)],
                         ids=["max", "amax", "adaptive"])
@pytest.mark.parametrize("kernels", [None, "emulation"])
def test_autograds_tie_rules_are_kept(head, kernels, emulated):
    torch.manual_seed(3)
    dtype = torch.float64 if kernels is None else torch.float32
    m, X = Ties(head).to(dtype).eval(), torch.randn(4, 3, 12, dtype=dtype) * 3
    out = m.act(m.c1(X))
    assert bool(((out == out.amax(2, keepdim=True)).sum(2) > 1).any())  # (there are ties)
    _against_autograd(m, X, None if kernels is None else _lib.get_kernels)


def test_the_tuple_of_a_max_is_no_new_kind_and_resolves_on_the_value():
    m, X = _net(SPELLINGS["x.max(2)[0]"][0], torch.float64)
    sweep = SeedBatchedSweep(m, {}, kernels=None)
    red = next(n for n, r in sweep.rule.items() if r.kind == _MAXRED)
    assert sweep.rule[red].args == ("max", (2,), False, "first", True)
    (item,) = red.users
    assert sweep.rule[item].kind == IDENTITY and sweep.rule[item].src == (red,)
    assert set(SeedBatchedSweep._VJP) >= {_MAXRED, _SUMRED} and SeedBatchedSweep._VJP[_MAXRED] is not None
    assert reduce_geometry((-1,), (5, 6, 4)) == ([2], 30, 4, 1) and reduce_geometry((2, 1), (5, 6, 4, 3)) == ([1, 2], 5, 24, 3)
    with pytest.raises(SweepUnsupported, match="dim 0"):
        reduce_geometry((-3,), (5, 6, 4))


# ---- refusals --------------------------------------------------------------------------------------------------------------------
REFUSED = {
    "max()": (lambda m, x: x.max().reshape(1, 1).expand(5, 6), "max.. without a dim"),
    "sum()": (lambda m, x: x.sum().reshape(1, 1).expand(5, 6), "sum.. without a dim"),
    "amax over dim 0": (lambda m, x: x.amax(0).unsqueeze(0), "amax over dim 0"),
    "sum over dim 0": (lambda m, x: x.sum((0, 2)), "sum over dim 0"),
    "max(x, other)": (lambda m, x: torch.max(x, x).mean(2), "max.x, other."),
    "x.max(2)[1]": (lambda m, x: x.max(2)[1].double(), "max: its indices"),
    "x.max(2).indices": (lambda m, x: x.max(2).indices.double(), "max: its indices"),
    "the pair itself": (lambda m, x: torch.relu(x.max(2)), "max.dim. returns .values, indices."),
    "non-adjacent dims": (lambda m, x: x.view(x.size(0), 6, 2, -1).amax((1, 3)), "amax over the non-adjacent dims"),
    "adaptive max pool to two cells": (lambda m, x: F.adaptive_max_pool1d(x, 2).mean(2), "adaptive_max_pool1d to 2 cells"),
    "AdaptiveMaxPool1d(2)": (lambda m, x: nn.AdaptiveMaxPool1d(2)(x).mean(2), "adaptive_max_pool1d to 2 cells"),
    "return_indices=True": (lambda m, x: F.adaptive_max_pool1d(x, 1, return_indices=True)[0].flatten(1), "adaptive_max_pool1d.return_indices=True."),
    "min": (lambda m, x: x.min(2)[0], "no VJP rule for method min .min is out of scope"),
    "amin": (lambda m, x: torch.amin(x, 2), "no VJP rule for function amin .amin is out of scope"),
    "logsumexp": (lambda m, x: x.logsumexp(2), "logsumexp is out of scope"),
    "dtype=": (lambda m, x: x.sum(2, dtype=torch.float64), "sum with dtype="),
    "out=": (lambda m, x: torch.amax(x, 2, out=torch.empty(5, 6)), "amax with an out= argument"),
    "max_pool1d(return_indices=True)": (lambda m, x: F.max_pool1d(x, 2, return_indices=True)[0].mean(2), "max_pool1d.return_indices=True."),
    "data-dependent pooling": (lambda m, x: F.max_pool1d(x, x.size(2)).flatten(1), "data-dependent pooling arguments"),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_what_is_not_served_is_refused_by_name(name):
    head, match = REFUSED[name]
    m, X = _net(head, torch.float32)
    if name == "AdaptiveMaxPool1d(2)":
        m.pool2 = nn.AdaptiveMaxPool1d(2)
        m.head = lambda mm, x: mm.pool2(x).mean(2)
    with pytest.raises(SweepUnsupported, match=match):
        SeedBatchedSweep(m, _taps(m), kernels=None).forward(X)


def test_string_padding_and_padding_modes_stay_refused():
    from laplace_amd.capture import Tape

    for conv in (nn.Conv1d(3, 4, 3, padding="same"), nn.Conv1d(3, 4, 3, padding=1, padding_mode="circular")):
        m = nn.Sequential(conv, nn.Tanh(), nn.AdaptiveMaxPool1d(1), nn.Flatten(), nn.Linear(4, 3)).eval()
        with pytest.raises(SweepUnsupported, match="unsupported convolution variant"):
            SeedBatchedSweep(m, {}, kernels=None)
        with pytest.raises(NotImplementedError, match="not supported"):
            Tape(m, list(m.parameters()))


def test_the_backend_still_answers_through_the_tape(emulated):
    from laplace_amd import HipGGN
    from oracle import curvature_oracle as co

    m, X = _net(lambda mm, x: x.logsumexp(2), torch.float64)
    backend = HipGGN(copy.deepcopy(m).float(), "classification")
    Js, f = backend.jacobians(X.float())
    assert "logsumexp" in backend._tape().sweep_reason
    Js64, f64 = co.jacobians(m, X)
    assert cf.rel(f, f64) < 1e-5 and cf.rel(Js, Js64) < 1e-4


def test_split_reason_names_the_node(emulated):
    from tests.emulated_kernels import EmulatedKernels  # noqa: F401  (the emulation offers the split-fp16 convolution)

    def reason(model):
        return SplitSweep(model.eval(), _taps(model), kernels=_lib.get_kernels).split_reason

    m, _ = _net(SPELLINGS["x.amax(2)"][0], torch.float32)
    assert reason(m) == "c1: Conv1d has no NHWC rule"
    two_d = nn.Sequential(nn.Conv2d(3, 32, 3, 1, 1), nn.Tanh(), nn.AdaptiveMaxPool2d(1), nn.Flatten(), nn.Linear(32, 3))
    assert reason(two_d) == "2: AdaptiveMaxPool2d (2) has no NHWC rule"

    class Amax(nn.Module):
        def __init__(self):
            super().__init__()
            self.c, self.fc = nn.Conv2d(3, 32, 3, 1, 1), nn.Linear(32, 3)

        def forward(self, x):
            return self.fc(torch.tanh(self.c(x)).amax((2, 3)))

    assert reason(Amax()) == "amax: amax has no NHWC rule"
    bn = nn.Sequential(nn.Linear(3, 4), nn.BatchNorm1d(4), nn.Tanh(), nn.Linear(4, 3))
    assert "BatchNorm1d" in reason(bn)


# ---- the backend: a Conv1d network is the unit-height Conv2d network it equals -------------------------------------------------------
def test_lift_is_a_view_with_the_geometry_as_pairs():
    from laplace_amd.conv import lift, lift_maps

    c = nn.Conv1d(4, 6, 3, 2, 5, dilation=2, groups=2)
    l = lift(c)
    assert isinstance(l, nn.Conv2d) and (l.kernel_size, l.stride, l.padding, l.dilation, l.groups) == ((1, 3), (1, 2), (0, 5), (1, 2), 2)
    assert l.weight.shape == (6, 2, 1, 3) and l.weight.data_ptr() == c.weight.data_ptr() and l.bias is c.bias
    assert torch.equal(l.weight.flatten(), c.weight.flatten()) and lift(c) is l
    v = l.weight._version
    with torch.no_grad():
        c.weight.mul_(2)
    assert l.weight._version == c.weight._version > v and torch.equal(l.weight.flatten(), c.weight.flatten())
    x = torch.randn(2, 4, 9)
    assert torch.equal(c(x), l(x.unsqueeze(2)).squeeze(2))
    a, g = lift_maps(c, x, torch.randn(3, 2, 6, 8))
    assert a.shape == (2, 4, 1, 9) and g.shape == (3, 2, 6, 1, 8) and a.data_ptr() == x.data_ptr()
    assert lift_maps(c, g=[torch.randn(2, 6, 8)])[1][0].shape == (2, 6, 1, 8)
    c2d = nn.Conv2d(3, 4, 3)
    assert lift(c2d) is c2d and lift_maps(c2d, x, x) == (x, x) and lift(nn.Linear(2, 2)).__class__ is nn.Linear
    c.double()
    assert lift(c).weight.dtype == torch.float64 and lift(c).weight.data_ptr() == c.weight.data_ptr()


@pytest.mark.parametrize("name", sorted(cf.FIXTURES))
def test_curvature_on_the_emulation_matches_the_oracle_with_the_kernels_on_and_off(name, emulated, monkeypatch):
    """fails without the feature: ``_supported()`` is ``False`` and ``kron`` raises "KFAC supports nn.Linear / nn.Conv2d parameters
    only"; the KFAC factors are held against ``oracle.kfac_ggn`` RUN ON THE TWIN"""
    fixture = cf.FIXTURES[name]()
    got = cf.run_curvature_checks("cpu", fixture, kron=name != "resnet1d-dw")
    tape = got["backend"]._tape()
    assert tape.sweep_reason is None if hasattr(tape, "sweep_reason") else True
    sweeps = [s for s in tape.sweeps.values() if s]
    assert sweeps and all(not getattr(s, "split_ok", False) for s in sweeps)  # (the NCHW walk)
    if name == "textcnn":
        assert {s[:2] for s in emulated.seen if s[0] == "maxred_vjp"} == {("maxred_vjp", "even")}
    emulated.seen.clear()
    monkeypatch.setattr(SeedBatchedSweep, "use_reduce_kernels", False)
    ref = cf.run_curvature_checks("cpu", fixture, kron=name != "resnet1d-dw")
    assert not any(s[0].startswith("maxred") for s in emulated.seen)
    for k in ("Js", "f", "h", "H", "dvar") + (("f_var",) if "f_var" in got else ()):
        assert cf.rel(got[k], ref[k]) < 1e-4, k


@pytest.mark.parametrize("name", sorted(cf.FIXTURES))
def test_the_hook_route_serves_the_same_quantities(name, emulated):
    def no_sweep(b):
        b.use_sweep = False

    got = cf.run_curvature_checks("cpu", cf.FIXTURES[name](), configure=no_sweep, kron=name != "resnet1d-dw")
    assert not got["backend"]._tape().sweeps


def test_kfac_refuses_a_grouped_conv1d_with_the_existing_message(emulated):
    from laplace_amd import HipGGN

    m, _, X, _, y = cf.resnet1d_fixture()
    backend = HipGGN(copy.deepcopy(m).float(), "classification")
    assert backend._supported()
    with pytest.raises(NotImplementedError, match="KFAC has no rule for a grouped convolution"):
        backend.kron(X.float(), y, N=X.shape[0])


def test_tracked_batchnorm1d_parameters_go_through_the_norm_taps(emulated):
    """``BatchNorm1d`` on ``[B, C, L]`` maps with tracked weight and bias: a norm tap beside the Conv1d taps"""
    from laplace_amd import HipGGN
    from laplace_amd.nets import ResNet1d
    from oracle import curvature_oracle as co

    m64 = cf._seeded(5, lambda: ResNet1d(3, 2, (4, 8), 1, nn.Tanh, freeze_norm=False))
    X64 = torch.randn(3, 2, 16, generator=torch.Generator().manual_seed(5)).double()
    backend = HipGGN(copy.deepcopy(m64).float(), "classification")
    assert backend._supported()
    Js, f = backend.jacobians(X64.float())
    tape = backend._tape()
    assert tape.norm_taps and "norm" in tape.route and all(s for s in tape.sweeps.values())
    Js64, f64 = co.jacobians(m64, X64)
    assert cf.rel(f, f64) < 1e-5 and cf.rel(Js, Js64) < 1e-4


def test_the_workloads_are_served(emulated):
    from laplace_amd import HipGGN
    from laplace_amd.nets import ResNet1d, TextCNN

    for model, X in ((ResNet1d(3, 2, (8, 8, 16, 16), 1), torch.randn(2, 2, 64)), (TextCNN(3, 20, 8, 6), torch.randint(20, (2, 9)))):
        backend = HipGGN(model.eval(), "classification")
        assert backend._supported()
        loss, H = backend.kron(X, torch.tensor([0, 2]), N=2)
        tape = backend._tape()
        assert getattr(tape, "sweep_reason", None) is None and tape.sweep not in (None, False)
        assert all(t.kind == "conv2d" for t in tape.taps[:-1]) and not tape.gconv_taps
