"""Upsampling and padding in the seed-batched reverse sweep (CPU): every spelling of ``nn.Upsample`` / ``F.interpolate`` and of
``F.pad`` / the padding modules goes through ONE reverse pass for all seeds and matches one autograd pass per seed - on the torch
math of the rule (two dense matrix products) and on the emulation of csrc/lk_resample.hip (tests/emulated_resample_kernels.py);
what the rule does not serve is refused by name; the workloads FPNSmall and TCNSmall reach the sweep and match the fp64 oracle.

Before this existed ``classify`` stopped at "no VJP rule for module Upsample (...)", "no VJP rule for function interpolate" or
"no VJP rule for function pad", and ``HipGGN.kron`` made one autograd pass per seed."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from laplace_amd import _lib
from laplace_amd import sweep as sw
from laplace_amd.sweep import CONST, SeedBatchedSweep, SweepUnsupported
from laplace_amd.sweep_nhwc import SplitSweep
from tests import conv1d_fixtures as cf
from tests import resample_fixtures as rf
from tests.norm_sweep_fixtures import autograd_reference


@pytest.fixture
def emulated():
    from tests.emulated_resample_kernels import EmulatedResampleKernels

    K = EmulatedResampleKernels()
    prev = _lib.set_kernels_for_testing(K)
    yield K
    _lib.set_kernels_for_testing(prev)


class Net2d(nn.Module):
    """Conv2d - tanh - ``body(x)`` (the resampling under test, twice where it takes a traced size) - Conv2d - mean - Linear"""

    def __init__(self, body, **mods):
        super().__init__()
        self.c1, self.c2, self.fc, self.body = nn.Conv2d(2, 3, 3, 1, 1), nn.Conv2d(3, 4, 3, 1, 1), nn.Linear(4, 3), body
        for n, m in mods.items():
            setattr(self, n, m)
        self.table = nn.Parameter(torch.linspace(-1, 1, 3 * 2 * 3).reshape(1, 3, 2, 3), requires_grad=False)  # (frozen: a constant)

    def forward(self, x):
        y = torch.tanh(self.c1(x))
        return self.fc(torch.tanh(self.c2(self.body(self, y))).mean((2, 3)))


class Net1d(nn.Module):
    def __init__(self, body, **mods):
        super().__init__()
        self.c1, self.c2, self.fc, self.body = nn.Conv1d(2, 3, 3, 1, 1), nn.Conv1d(3, 4, 3, 1, 1), nn.Linear(4, 3), body
        for n, m in mods.items():
            setattr(self, n, m)

    def forward(self, x):
        y = torch.tanh(self.c1(x))
        return self.fc(torch.tanh(self.c2(self.body(self, y))).mean(2))


# name -> (dims, body, modules the body uses, number of resampling nodes)
SPELLINGS = {
    "nn.Upsample(scale_factor=2)": (2, lambda m, x: m.up(x), dict(up=nn.Upsample(scale_factor=2, mode="nearest")), 1),
    "nn.Upsample(size, bilinear, align_corners=True)": (2, lambda m, x: m.up(x), dict(up=nn.Upsample(size=(9, 7), mode="bilinear", align_corners=True)), 1),
    "nn.Upsample(bicubic)": (2, lambda m, x: m.up(x), dict(up=nn.Upsample(scale_factor=2, mode="bicubic", align_corners=False)), 1),
    "nn.UpsamplingNearest2d": (2, lambda m, x: m.up(x), dict(up=nn.UpsamplingNearest2d(scale_factor=2)), 1),
    "nn.UpsamplingBilinear2d": (2, lambda m, x: m.up(x), dict(up=nn.UpsamplingBilinear2d(scale_factor=2)), 1),
    "nn.Upsample(linear) 1-D": (1, lambda m, x: m.up(x), dict(up=nn.Upsample(scale_factor=2, mode="linear", align_corners=False)), 1),
    "F.interpolate(size)": (2, lambda m, x: F.interpolate(x, size=(7, 11), mode="bilinear", align_corners=False), {}, 1),
    "F.interpolate(scale_factor=1.5)": (2, lambda m, x: F.interpolate(x, scale_factor=1.5, mode="bilinear", align_corners=False), {}, 1),
    "F.interpolate(scale_factor tuple, recompute)": (2, lambda m, x: F.interpolate(x, scale_factor=(2.0, 1.5), mode="bilinear", recompute_scale_factor=True), {}, 1),
    "F.interpolate(traced size=y.size()[2:])": (2, lambda m, x: F.interpolate(F.interpolate(x, scale_factor=0.5, mode="area"), size=x.size()[2:], mode="bilinear", align_corners=False) + x, {}, 2),
    "F.interpolate(traced size=(y.size(2), y.size(3)))": (2, lambda m, x: F.interpolate(F.avg_pool2d(x, 2), size=(x.size(2), x.size(3)), mode="nearest") + x, {}, 1),
    "F.interpolate positional": (2, lambda m, x: F.interpolate(x, None, 2, "bicubic", True), {}, 1),
    "F.interpolate(nearest-exact)": (2, lambda m, x: F.interpolate(x, size=(8, 9), mode="nearest-exact"), {}, 1),
    "F.interpolate(area)": (2, lambda m, x: F.interpolate(x, size=(3, 2), mode="area"), {}, 1),
    "F.interpolate(bilinear, antialias)": (2, lambda m, x: F.interpolate(x, size=(3, 3), mode="bilinear", align_corners=False, antialias=True), {}, 1),
    "F.interpolate(bicubic, antialias)": (2, lambda m, x: F.interpolate(x, size=(3, 4), mode="bicubic", align_corners=False, antialias=True), {}, 1),
    "F.interpolate(nearest) 1-D": (1, lambda m, x: F.interpolate(x, scale_factor=3), {}, 1),
    "F.interpolate(linear, align_corners=True) 1-D": (1, lambda m, x: F.interpolate(x, size=13, mode="linear", align_corners=True), {}, 1),
    "F.interpolate(area) 1-D": (1, lambda m, x: F.interpolate(x, size=4, mode="area"), {}, 1),
    "F.pad zeros 2-D": (2, lambda m, x: F.pad(x, (1, 2, 0, 1)), {}, 1),
    "F.pad last dim of a 4-D value": (2, lambda m, x: F.pad(x, (2, 0)), {}, 1),
    "F.pad with a value": (2, lambda m, x: F.pad(x, (1, 1, 2, 0), "constant", 0.5), {}, 1),
    "F.pad negative (crop)": (2, lambda m, x: F.pad(x, (-1, 2, 1, -2)), {}, 1),
    "F.pad trailing zero pairs": (2, lambda m, x: F.pad(x, (1, 0, 0, 2, 0, 0)), {}, 1),
    "F.pad reflect": (2, lambda m, x: F.pad(x, (2, 1, 1, 2), mode="reflect"), {}, 1),
    "F.pad replicate": (2, lambda m, x: F.pad(x, (2, 1, 0, 3), mode="replicate"), {}, 1),
    "F.pad circular": (2, lambda m, x: F.pad(x, (1, 2, 2, 1), mode="circular"), {}, 1),
    "F.pad causal 1-D": (1, lambda m, x: F.pad(x, (4, 0)), {}, 1),
    "F.pad [B, T, D] both dims": (1, lambda m, x: F.pad(x, (1, 1, 0, 0), value=-1.0)[:, :, 1:-1] + F.pad(x, (2, 0, 0, 0)).narrow(2, 0, 12), {}, 2),
    "F.pad reflect 1-D": (1, lambda m, x: F.pad(x, (3, 1), mode="reflect"), {}, 1),
    "nn.ZeroPad1d": (1, lambda m, x: m.p(x), dict(p=nn.ZeroPad1d((2, 1))), 1),
    "nn.ZeroPad2d": (2, lambda m, x: m.p(x), dict(p=nn.ZeroPad2d((0, 1, 0, 1))), 1),
    "nn.ConstantPad1d": (1, lambda m, x: m.p(x), dict(p=nn.ConstantPad1d(2, 0.25)), 1),
    "nn.ConstantPad2d": (2, lambda m, x: m.p(x), dict(p=nn.ConstantPad2d((1, 0, 2, 1), -0.5)), 1),
    "nn.ReflectionPad1d": (1, lambda m, x: m.p(x), dict(p=nn.ReflectionPad1d((2, 0))), 1),
    "nn.ReflectionPad2d": (2, lambda m, x: m.p(x), dict(p=nn.ReflectionPad2d(2)), 1),
    "nn.ReplicationPad1d": (1, lambda m, x: m.p(x), dict(p=nn.ReplicationPad1d((0, 3))), 1),
    "nn.ReplicationPad2d": (2, lambda m, x: m.p(x), dict(p=nn.ReplicationPad2d((1, 2, 3, 0))), 1),
    "nn.CircularPad1d": (1, lambda m, x: m.p(x), dict(p=nn.CircularPad1d(2)), 1),
    "nn.CircularPad2d": (2, lambda m, x: m.p(x), dict(p=nn.CircularPad2d((1, 0, 2, 1))), 1),
    "one module applied twice": (2, lambda m, x: m.up(F.avg_pool2d(m.up(x), 2)), dict(up=nn.Upsample(scale_factor=2, mode="bilinear")), 2),
}


def _net(name, dtype):
    import copy

    dims, body, mods, _ = SPELLINGS[name] if name in SPELLINGS else REFUSED[name][:4]
    torch.manual_seed(11)
    m = (Net2d if dims == 2 else Net1d)(body, **copy.deepcopy(mods)).to(dtype).eval()
    return m, torch.randn(*((4, 2, 6, 5) if dims == 2 else (4, 2, 12)), dtype=dtype)


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
    assert torch.equal(f, f_ref.detach()) if kernels is None else torch.allclose(f, f_ref.detach(), rtol=1e-4, atol=1e-7)
    tol = dict(rtol=1e-9, atol=1e-12) if X.dtype == torch.float64 else dict(rtol=1e-4, atol=1e-6)
    for n in taps:
        assert grads[n].shape == want[n].shape, n
        assert torch.allclose(grads[n], want[n], **tol), (n, (grads[n] - want[n]).abs().max())
    return sweep


@pytest.mark.parametrize("name", sorted(SPELLINGS))
def test_sweep_matches_one_autograd_pass_per_seed(name):
    """fails without the rule: "no VJP rule for module Upsample (up)", "no VJP rule for function interpolate" or "no VJP rule for
    function pad" at construction.  fp64, the torch math of the rule; the forward is torch's own call: bit-equal to the model's"""
    sweep = _against_autograd(*_net(name, torch.float64), kernels=None)
    assert sum(r.kind == sw._RESAMPLE for r in sweep.rule.values()) == SPELLINGS[name][3]
    assert all(v.startswith("torch math") for v in sweep.resample_route.values()) and sweep.resample_route


@pytest.mark.parametrize("name", sorted(SPELLINGS))
def test_sweep_on_the_emulation_matches_autograd(name, emulated):
    """fails without the rule, as above; fp32, every resampling node through ``resample_vjp`` of the kernel object"""
    sweep = _against_autograd(*_net(name, torch.float32), kernels=_lib.get_kernels)
    calls = [s for s in emulated.seen if s[0] == "resample_vjp"]
    assert len(calls) == SPELLINGS[name][3] and set(sweep.resample_route.values()) == {"kernel"}
    assert all(c[1] % (4 * 4) == 0 for c in calls)  # (P = S B C planes: all seeds in one call)


def test_the_tables_are_derived_once_per_geometry(emulated, monkeypatch):
    built = []
    real = sw.resample_tables
    monkeypatch.setattr(sw, "resample_tables", lambda *a, **k: built.append(a[:4]) or real(*a, **k))
    m, X = _net("one module applied twice", torch.float32)
    sweep = SeedBatchedSweep(m, _taps(m), kernels=_lib.get_kernels)
    for _ in range(2):
        sweep.forward(X)
    assert len(built) == 1  # (both applications map 6x5 to 12x10: one geometry, cached on the sweep)
    sweep.forward(X[:2])
    assert len(built) == 1  # (the batch size is no part of the geometry)
    sweep.forward(torch.randn(2, 2, 8, 5))
    assert len(built) == 2


def test_the_switch_and_the_dtype_keep_the_rule_on_torch_math(emulated, monkeypatch):
    monkeypatch.setattr(SeedBatchedSweep, "use_resample_kernels", False)
    s = _against_autograd(*_net("F.pad reflect", torch.float32), kernels=_lib.get_kernels)
    assert not any(c[0] == "resample_vjp" for c in emulated.seen) and "use_resample_kernels is off" in s.resample_route["pad"]
    monkeypatch.setattr(SeedBatchedSweep, "use_resample_kernels", True)
    s = _against_autograd(*_net("F.pad reflect", torch.float64), kernels=_lib.get_kernels)  # (not fp32: the torch math)
    assert not any(c[0] == "resample_vjp" for c in emulated.seen) and "float64" in s.resample_route["pad"]
    from tests.emulated_reduce_kernels import EmulatedReduceKernels

    prev = _lib.set_kernels_for_testing(EmulatedReduceKernels())  # (a kernel object without the entry)
    try:
        s = _against_autograd(*_net("F.pad reflect", torch.float32), kernels=_lib.get_kernels)
        assert "has no resample_vjp" in s.resample_route["pad"]
    finally:
        _lib.set_kernels_for_testing(prev)


def test_an_over_cap_geometry_takes_the_matmul_form_and_gives_the_same_numbers(emulated):
    """x17 nearest: 17 outputs read every input, one more than LK_RESAMPLE_MAX_TAPS - not refused: the torch math, said so in
    ``resample_route``; x16 (the cap itself) runs the kernel"""
    over = lambda m, x: F.interpolate(x, scale_factor=rf.CAP + 1, mode="nearest")  # noqa: E731
    torch.manual_seed(11)
    m, X = Net1d(over).eval(), torch.randn(4, 2, 12)
    s = _against_autograd(m, X, kernels=_lib.get_kernels)
    assert "17 taps per input exceed the kernel's cap of 16" in s.resample_route["interpolate"]
    assert not any(c[0] == "resample_vjp" for c in emulated.seen)
    ref = _against_autograd(m, X, kernels=None)
    at_cap = Net1d(lambda m, x: F.interpolate(x, scale_factor=rf.CAP, mode="nearest")).eval()
    s = _against_autograd(at_cap, X, kernels=_lib.get_kernels)
    assert s.resample_route["interpolate"] == "kernel" and emulated.seen[-1][-1] == rf.CAP
    assert ref.resample_route["interpolate"].startswith("torch math")


def test_the_math_form_is_two_matmuls_and_repeats_bit_for_bit():
    c = rf.CASES[6]
    t = rf.tables(c)
    g = rf.make_g(c, torch.Generator().manual_seed(3)).reshape(2, 3, *rf.out_extent(c))
    a, b = sw.resample_vjp_math(g, t.Mh, t.Mw, 2), sw.resample_vjp_math(g, t.Mh, t.Mw, 2)
    assert a.shape == (2, 3, c["H"], c["W"]) and torch.equal(a, b)
    ref, bound, _ = rf.vjp_reference(g.reshape(6, *g.shape[2:]), t.csr_h, t.csr_w)
    assert bool(((a.reshape(ref.shape).double() - ref).abs() <= 4 * bound + 1e-12).all())
    assert isinstance(t, sw.ResampleTables) and t.Mh.shape == (rf.out_extent(c)[0], c["H"])


# ---- refusals --------------------------------------------------------------------------------------------------------------------
REFUSED = {
    "trilinear": (2, lambda m, x: F.interpolate(x.reshape(x.size(0), 3, 1, 6, 5), scale_factor=2, mode="trilinear").mean(2), {}, 0, "interpolate in mode trilinear"),
    "a 5-D operand": (2, lambda m, x: F.interpolate(x.reshape(x.size(0), 3, 1, 6, 5), scale_factor=2, mode="nearest").mean(2), {}, 0, "interpolate of a 5-D value"),
    "pad of three dims": (2, lambda m, x: F.pad(x, (1, 1, 1, 1, 1, 1))[:, 1:-1], {}, 0, "pad.* pads more than the last two dims"),
    "a traced value": (2, lambda m, x: F.pad(x, (1, 1), value=x.size(2)), {}, 0, "pad with a traced value"),
    "a 2-D operand": (2, lambda m, x: F.pad(x.flatten(1), (1, 1))[:, 1:-1].reshape(4, 3, 6, 5), {}, 0, "pad of a value with 2 dims"),
    "a mode torch refuses": (2, lambda m, x: F.interpolate(x, scale_factor=2, mode="linear"), {}, 0, "interpolate: "),
    "reflect wider than the map": (2, lambda m, x: F.pad(x, (7, 0), mode="reflect"), {}, 0, "pad: "),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_what_is_not_served_is_refused_by_name(name):
    m, X = _net(name, torch.float32)
    with pytest.raises(SweepUnsupported, match=REFUSED[name][4]):
        SeedBatchedSweep(m, _taps(m), kernels=None).forward(X)


def test_the_integer_input_and_hand_made_calls_are_refused_by_name():
    import torch.fx as fx

    m, X = _net("F.pad causal 1-D", torch.float32)
    sweep = SeedBatchedSweep(m, _taps(m), kernels=None)
    node, r = next((n, r) for n, r in sweep.rule.items() if r.kind == sw._RESAMPLE)
    with pytest.raises(SweepUnsupported, match="pad: the operand is the integer input"):
        sweep._run_resample(node, r, torch.arange(12).reshape(1, 1, 12), r.call[1])
    with pytest.raises(SweepUnsupported, match="pad.* of a value with 3 dims pads dim 0"):
        sw.resample_dims("pad", {"pad": (0, 0, 0, 0, 1, 0)}, (4, 3, 12), "pad")
    assert sw.resample_dims("pad", {"pad": (1, 0, 0, 0, 0, 0)}, (4, 3, 12), "pad") == 1  # (trailing zero pairs pad nothing)
    # the argument checks of `classify`, on hand-made nodes (fx binds out= away for these two functions)
    g = fx.Graph()
    x = g.placeholder("x")
    modules = {"": nn.Module()}
    for target, kwargs, match in ((F.pad, dict(pad=(1, 1), out=x), "pad with an out= argument"),
                                  (F.interpolate, dict(scale_factor=2, out=x), "interpolate with an out= argument"),
                                  (F.pad, dict(pad=(1, 1), value=x), "pad with a traced value"),
                                  (F.pad, dict(pad=(1, x)), "pad with a data-dependent pad"),
                                  (F.pad, dict(pad=(1, 1, 1)), "pad must be a non-empty tuple"),
                                  (F.interpolate, dict(scale_factor=x), "interpolate with a data-dependent scale_factor"),
                                  (F.interpolate, dict(size=(x, 3)), "interpolate with a data-dependent size"),
                                  (F.interpolate, dict(scale_factor=2, mode=x), "interpolate with a data-dependent mode"),
                                  (F.interpolate, dict(scale_factor=2, mode="trilinear"), "interpolate in mode trilinear"),
                                  (F.interpolate, dict(scale_factor=2, bogus=1), "interpolate: unknown argument")):
        node = g.call_function(target, (x,), kwargs)
        with pytest.raises(SweepUnsupported, match=match):
            sw.classify(node, modules)
    with pytest.raises(SweepUnsupported, match="the operand must be a traced tensor"):
        sw.classify(g.call_function(F.pad, (1.0, (1, 1))), modules)


def test_convolution_padding_modes_stay_refused_exactly_as_before():
    for conv in (nn.Conv2d(2, 3, 3, padding="same"), nn.Conv2d(2, 3, 3, padding=1, padding_mode="reflect")):
        m = nn.Sequential(conv, nn.Tanh(), nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(3, 3)).eval()
        with pytest.raises(SweepUnsupported, match="^0: unsupported convolution variant$"):
            SeedBatchedSweep(m, {}, kernels=None)


def test_the_kind_is_module_private_and_has_a_reverse_rule():
    assert sw._RESAMPLE == "static-resampling" and SeedBatchedSweep._VJP[sw._RESAMPLE] == "_vjp_resample"
    public = [n for n, v in vars(sw).items() if n.isupper() and not n.startswith("_") and isinstance(v, str)]
    assert "RESAMPLE" not in public and sw._RESAMPLE not in {getattr(sw, n) for n in public}
    from laplace_amd import capture

    assert not any("resampl" in str(k).lower() or "pad" in str(k).lower() for k in capture.EXTRA_KINDS)


def test_a_constant_operand_is_a_constant(emulated):
    """a resampled frozen buffer (a position table stored at another resolution) is a CONST, as ``neg`` of one is"""
    body = lambda m, x: x + F.interpolate(m.table, size=x.size()[2:], mode="bilinear", align_corners=False) + F.pad(m.table, (1, 1, 2, 2))  # noqa: E731
    for dtype, kernels in ((torch.float64, None), (torch.float32, _lib.get_kernels)):
        torch.manual_seed(11)
        m, X = Net2d(body).to(dtype).eval(), torch.randn(4, 2, 6, 5, dtype=dtype)
        s = _against_autograd(m, X, kernels)
        kinds = [r.kind for n, r in s.rule.items() if n.name.startswith(("interpolate", "pad"))]
        assert kinds == [CONST, CONST] and not any(r.kind == sw._RESAMPLE for r in s.rule.values())
    assert not any(c[0] == "resample_vjp" for c in emulated.seen)


def test_split_reason_names_the_node(emulated):
    def reason(model):
        return SplitSweep(model.eval(), _taps(model), kernels=_lib.get_kernels).split_reason

    class Up(nn.Module):
        def __init__(self, functional):
            super().__init__()
            self.c, self.c2, self.up, self.fc, self.functional = nn.Conv2d(3, 32, 3, 1, 1), nn.Conv2d(32, 32, 3, 2, 1), nn.Upsample(scale_factor=2), nn.Linear(32, 3), functional
            self.pool = nn.AdaptiveAvgPool2d(1)

        def forward(self, x):
            y = torch.relu(self.c(x))
            z = torch.relu(self.c2(y))
            z = F.interpolate(z, size=y.size()[2:], mode="bilinear") if self.functional else self.up(z)
            return self.fc(torch.flatten(self.pool(y + z), 1))

    assert reason(Up(False)) == "up: Upsample (up) has no NHWC rule"
    assert reason(Up(True)) == "interpolate: interpolate has no NHWC rule"
    padded = nn.Sequential(nn.ZeroPad2d((0, 1, 0, 1)), nn.Conv2d(3, 32, 3, 2), nn.ReLU(), nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(32, 3))
    assert reason(padded) == "0: ZeroPad2d (0) has no NHWC rule"
    from laplace_amd.nets import FPNSmall

    assert reason(FPNSmall(3, (32, 32, 32), 32)) == "up: Upsample (up) has no NHWC rule"


# ---- the backend and the workloads -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rf.FIXTURES))
def test_curvature_on_the_emulation_matches_the_oracle_with_the_kernels_on_and_off(name, emulated, monkeypatch):
    """fails without the rule: ``tape.sweep_reason`` is "no VJP rule for module Upsample (up)" / "... function interpolate" / "...
    function pad" and no ``resample_vjp`` call is seen.  f, jacobians, diag, full, a two-minibatch kron fit and both GLM predictives
    against the fp64 oracle, the KFAC factors element-wise against ``oracle.kfac_ggn`` (the TCN: on its unit-height 2-D twin), to the
    bounds of ``conv1d_fixtures.run_curvature_checks``"""
    fixture = rf.FIXTURES[name]()
    got = cf.run_curvature_checks("cpu", fixture)
    tape = got["backend"]._tape()
    assert getattr(tape, "sweep_reason", None) is None
    sweeps = [s for s in tape.sweeps.values() if s]
    assert sweeps and all(not getattr(s, "split_ok", False) for s in sweeps)  # (the NCHW walk)
    assert any(s[0] == "resample_vjp" for s in emulated.seen)
    assert all(set(s.resample_route.values()) == {"kernel"} for s in sweeps if getattr(s, "resample_route", None))
    emulated.seen.clear()
    monkeypatch.setattr(SeedBatchedSweep, "use_resample_kernels", False)
    ref = cf.run_curvature_checks("cpu", fixture)
    assert not any(s[0] == "resample_vjp" for s in emulated.seen)
    for k in ("Js", "f", "h", "H", "dvar", "f_var"):
        assert cf.rel(got[k], ref[k]) < 1e-4, k


@pytest.mark.parametrize("name", sorted(rf.FIXTURES))
def test_the_hook_route_serves_the_same_quantities(name, emulated):
    def no_sweep(b):
        b.use_sweep = False

    got = cf.run_curvature_checks("cpu", rf.FIXTURES[name](), configure=no_sweep)
    assert not got["backend"]._tape().sweeps


def test_the_workloads_are_served(emulated):
    """fails without the rule: ``tape.sweep_reason`` names the Upsample / interpolate / pad node and ``tape.sweep`` is ``False``"""
    from laplace_amd import HipGGN
    from laplace_amd.nets import FPNSmall, TCNSmall

    for model, X in ((FPNSmall(3, (32, 32, 64), 32), torch.randn(2, 3, 16, 16)), (FPNSmall(3, (32, 32, 64), 32, "bilinear"), torch.randn(2, 3, 16, 16)),
                     (TCNSmall(3, 4, 8), torch.randn(2, 4, 24))):
        backend = HipGGN(model.eval(), "classification")
        assert backend._supported()
        y = torch.tensor([0, 2])
        backend.kron(X, y, N=2)
        tape = backend._tape()
        assert getattr(tape, "sweep_reason", None) is None and tape.sweep not in (None, False)
        assert set(tape.sweep.resample_route.values()) == {"kernel"}
        backend.diag(X, y), backend.full(X, y), backend.jacobians(X)
        assert getattr(backend._tape(), "sweep_reason", None) is None
    with pytest.raises(ValueError, match="mode must be"):
        FPNSmall(mode="bicubic")
