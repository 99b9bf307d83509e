"""The NORM rule for nn.RMSNorm and the NEG / SUB rules of the seed-batched reverse sweep (laplace_amd/sweep.py) on the CPU: the
parts of a LLaMA / Mistral / Gemma block the sweep did not serve - RMSNorm pre-norms and the ``-x`` of a rotary embedding's
rotate-half - and the difference that completes the arithmetic.  Models that use them go through ONE sweep for all seeds and match
one autograd pass per seed in fp64; the curvature of a small LLaMA network matches the fp64 oracle; the kernel branch runs on the
emulation (tests/emulated_rmsnorm_kernels.py); the split sweep names the nodes and leaves the model to the NCHW walk; tracked
RMSNorm weights are served by the norm taps; what the rules do not serve is refused by name.

Before the rules existed every model here was refused whole - "no VJP rule for module RMSNorm" / "function neg" / "function sub"
(the methods: "method neg", "method sub") at construction - and took the autograd tape."""
import copy
import operator

import pytest
import torch
from torch import nn

from laplace_amd import _lib
from laplace_amd._lib import get_kernels
from laplace_amd.sweep import CONST, NEG, NORM, SUB, SeedBatchedSweep, SweepUnsupported
from laplace_amd.sweep_nhwc import SplitSweep
from tests import rmsnorm_fixtures as rf
from tests.norm_sweep_fixtures import autograd_reference
from tests.slice_fixtures import run_curvature_checks


def _taps(model):
    return {n: m for n, m in model.named_modules() if isinstance(m, (nn.Linear, nn.Conv2d))}


def _isub(a, b):
    a -= b
    return a


NEG_SPELLINGS = {
    "operator": operator.neg, "torch.neg": torch.neg, "torch.negative": torch.negative, "method-neg": lambda a: a.neg(),
    "method-negative": lambda a: a.negative(), "method-neg_": lambda a: a.neg_(),
}
SUB_SPELLINGS = {
    "operator": operator.sub, "operator-isub": _isub, "torch.sub": torch.sub, "torch.subtract": torch.subtract,
    "method-sub": lambda a, b: a.sub(b), "method-subtract": lambda a, b: a.subtract(b), "method-sub_": lambda a, b: a.sub_(b),
}
INPLACE = ("operator-isub", "method-sub_")  # (a Python number has no in-place method: written ``-`` there)


def _check_against_autograd(m64, X, n_seeds=4, kinds=None):
    taps = _taps(m64)
    sweep = SeedBatchedSweep(m64, taps, kernels=None)
    for kind, count in (kinds or {}).items():
        assert sum(r.kind == kind for r in sweep.rule.values()) == count, (kind, [r.kind for r in sweep.rule.values()])
    f = sweep.forward(X)
    seeds = torch.randn(n_seeds, *f.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    grads = sweep.backward(seeds)
    f_ref, ins, want = autograd_reference(m64, taps, X, seeds)
    assert (f - f_ref.detach()).abs().max() <= 1e-10 * (1 + f_ref.abs().max())
    for n in taps:
        # (no in-place spelling wrote into a kept tensor; behind an RMSNorm the sweep's own forward differs from torch's in the last bit)
        assert (sweep.taps[n]["a"] - ins[n]).abs().max() <= 1e-10 * (1 + ins[n].abs().max()), n
        assert grads[n].shape == want[n].shape, n
        assert (grads[n] - want[n]).abs().max() <= 1e-10 * (1 + want[n].abs().max()), n
    return sweep


# ---- 1. every spelling against autograd ------------------------------------------------------------------------------------------
class Rotary(nn.Module):
    """the rotate-half of a rotary embedding with every spelling of the sign, and the negation of a frozen parameter (a constant)"""

    def __init__(self, spell):
        super().__init__()
        self.neg = NEG_SPELLINGS[spell]
        self.q, self.fc = nn.Linear(3, 8), nn.Linear(8, 3)
        ang = torch.arange(16, dtype=torch.float32).unsqueeze(1) * torch.linspace(0.1, 1.0, 4).repeat(2).unsqueeze(0)
        self.register_buffer("cos", ang.cos(), persistent=False)
        self.register_buffer("sin", ang.sin(), persistent=False)
        self.frozen = nn.Parameter(ang.sin(), requires_grad=False)  # (fx folds an operation on a plain buffer; not on a parameter)

    def forward(self, x):
        q = self.q(x.flatten(2).transpose(1, 2))  # [B, 16, 8]
        rot = torch.cat((self.neg(q[..., 4:] + 0), q[..., :4]), -1)
        q = q * self.cos + rot * self.sin
        return self.fc((q + q * operator.neg(self.frozen)).mean(1))


@pytest.mark.parametrize("spell", sorted(NEG_SPELLINGS))
def test_neg_matches_one_autograd_pass_per_seed(spell):
    """fails without the rule: "no VJP rule for function neg" (the methods: "method neg", ...) at construction"""
    torch.manual_seed(11)
    m = Rotary(spell).double().eval()
    sweep = _check_against_autograd(m, torch.randn(5, 3, 4, 4, dtype=torch.float64), kinds={NEG: 1})
    assert any(r.kind == CONST and r.what.startswith("constant neg of") for r in sweep.rule.values())  # (``-sin``: no cotangent)


class Difference(nn.Module):
    """two traced tensors, a traced tensor and a constant on either side, a traced tensor and a number on either side, ``h - h``"""

    def __init__(self, spell):
        super().__init__()
        self.sub, self.plain = SUB_SPELLINGS[spell], SUB_SPELLINGS["operator" if spell in INPLACE else spell]
        self.a, self.b, self.fc = nn.Linear(3, 6), nn.Linear(3, 6), nn.Linear(6, 3)
        self.register_buffer("shift", torch.linspace(-1.0, 1.0, 6))
        self.table = nn.Parameter(torch.linspace(0.5, 2.0, 16 * 6).reshape(16, 6), requires_grad=False)

    def forward(self, x):
        x = x.flatten(2).transpose(1, 2)  # [B, 16, 3]
        a, b = torch.tanh(self.a(x)), torch.sigmoid(self.b(x))
        h = self.sub(a + 0, b)  # two traced tensors: the minuend is a node of its own whose value a tap keeps
        h = self.sub(h + 0, self.shift)  # traced - constant [6]
        h = self.plain(self.table, h)  # constant [16, 6] - traced
        h = self.sub(h + 0, 1.0) if self.sub is not _isub else h - 1.0
        h = operator.sub(1, h) + (a - a)  # number - traced; a tensor minus itself
        return self.fc(h.mean(1))


@pytest.mark.parametrize("spell", sorted(SUB_SPELLINGS))
def test_sub_matches_one_autograd_pass_per_seed(spell):
    """fails without the rule: "no VJP rule for function sub" (the methods: "method sub", ...) at construction"""
    torch.manual_seed(12)
    m = Difference(spell).double().eval()
    _check_against_autograd(m, torch.randn(5, 3, 4, 4, dtype=torch.float64), kinds={SUB: 6})


class Normed(nn.Module):
    def __init__(self, affine, eps, shape=(6,)):
        super().__init__()
        self.embed, self.fc = nn.Linear(3, 6), nn.Linear(6, 3)
        self.n1 = nn.RMSNorm(6, eps=eps, elementwise_affine=affine)
        self.n2 = nn.RMSNorm(list(shape), eps=eps, elementwise_affine=affine)
        if affine:
            with torch.no_grad():
                self.n1.weight.copy_(torch.linspace(-1.0, 1.5, 6))
                self.n2.weight.copy_(torch.linspace(0.5, 2.0, self.n2.weight.numel()).reshape(self.n2.weight.shape))
            self.n1.weight.requires_grad_(False), self.n2.weight.requires_grad_(False)

    def forward(self, x):
        h = self.embed(x.flatten(2).transpose(1, 2))  # [B, 16, 6]
        h = h + torch.tanh(self.n1(h))
        return self.fc(self.n2(h).mean(1))


@pytest.mark.parametrize("shape", ((6,), (16, 6)), ids=("last-dim", "two-dims"))
@pytest.mark.parametrize("eps", (None, 1e-6, 0.5), ids=("eps-none", "eps-1e-6", "eps-0.5"))
@pytest.mark.parametrize("affine", (True, False), ids=("weight", "no-weight"))
def test_rmsnorm_matches_one_autograd_pass_per_seed(affine, eps, shape):
    """fails without the rule: "no VJP rule for module RMSNorm" at construction.  ``eps=None`` is torch's default of the module: the
    machine epsilon of the input's dtype"""
    torch.manual_seed(13)
    m = Normed(affine, eps, shape).double().eval()
    sweep = _check_against_autograd(m, torch.randn(5, 3, 4, 4, dtype=torch.float64), kinds={NORM: 2})
    kept = [sweep.saved[n] for n, r in sweep.rule.items() if r.kind == NORM]
    assert all(k[0] == "rms" for k in kept)  # (the input's view and rstd: no activation-sized xhat)
    assert [tuple(k[1].shape) for k in kept] == [(5 * 16, 6), (5 * 16, 6) if shape == (6,) else (5, 96)]
    assert [tuple(k[2].shape) for k in kept] == [(5 * 16,), (5 * 16,) if shape == (6,) else (5,)]


# ---- 2. refusals by name ---------------------------------------------------------------------------------------------------------------
class _Refused(nn.Module):
    def __init__(self, how):
        super().__init__()
        self.how, self.a, self.fc = how, nn.Linear(4, 6), nn.Linear(6, 3)
        self.g = nn.Linear(4, 1)
        self.u, self.v = (nn.Parameter(torch.ones(6), requires_grad=False) for _ in range(2))  # (fx folds plain buffers)
        self.register_buffer("table", torch.ones(5, 6))
        self.norm = nn.RMSNorm(5)

    def forward(self, x):  # [B, 4]
        how, h = self.how, torch.tanh(self.a(x))
        if how == "alpha":
            h = torch.sub(h, torch.sigmoid(h), alpha=2)
        elif how == "out":
            h = torch.sub(h, torch.sigmoid(h), out=h)
        elif how == "two-constants":
            h = h + (self.u - self.v)
        elif how == "different-shapes":
            h = h - torch.tanh(self.g(x))  # [B, 6] - [B, 1]
        elif how == "wide-constant":
            h = (h.view(-1, 1, 6) - self.table).mean(1)  # [B, 1, 6] against [5, 6]
        elif how == "functional":
            h = nn.functional.rms_norm(h, (6,))
        elif how == "shape-mismatch":
            h = self.norm(h)  # RMSNorm(5) on [B, 6]
        return self.fc(h)


AT_CONSTRUCTION = {"alpha": "sub with alpha != 1", "out": "sub with an out= argument", "two-constants": "sub of two constants",
                   "functional": "no VJP rule for function rms_norm"}
IN_THE_FORWARD = {"different-shapes": r"sub of \(3, 6\) and \(3, 1\): traced operands of different shapes \(the VJP needs a reduction\)",
                  "wide-constant": r"sub: \(3, 1, 6\) broadcasts against the constant table of shape \(5, 6\) \(the VJP needs a reduction\)",
                  "shape-mismatch": r"RMSNorm\(\(5,\)\) on an input of shape \(3, 6\)"}


@pytest.mark.parametrize("how", sorted(AT_CONSTRUCTION))
def test_what_is_not_served_is_refused_at_construction(how):
    model = _Refused(how).eval()
    with pytest.raises(SweepUnsupported, match=AT_CONSTRUCTION[how]) as e:
        SeedBatchedSweep(model, _taps(model), kernels=None)
    assert how == "functional" or "sub" in str(e.value)


@pytest.mark.parametrize("how", sorted(IN_THE_FORWARD))
def test_what_only_the_shapes_tell_is_refused_in_the_forward(how):
    model = _Refused(how).eval()
    sweep = SeedBatchedSweep(model, _taps(model), kernels=None)
    with pytest.raises(SweepUnsupported, match=IN_THE_FORWARD[how]) as e:
        sweep.forward(torch.randn(3, 4))
    assert how == "shape-mismatch" or "sub" in str(e.value)


def test_a_product_with_a_number_stays_refused():
    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = nn.Linear(4, 3)

        def forward(self, x):
            return -(self.fc(x) * 2.0)

    with pytest.raises(SweepUnsupported, match="mul by the Python number 2.0 is not served"):
        SeedBatchedSweep(M().eval(), {}, kernels=None)


# ---- 3. the kernel branch and the curvature on the emulation -------------------------------------------------------------------------
@pytest.fixture
def emulated():
    from tests.emulated_rmsnorm_kernels import EmulatedRmsNormKernels

    K = EmulatedRmsNormKernels()
    prev = _lib.set_kernels_for_testing(K)
    yield K
    _lib.set_kernels_for_testing(prev)


def test_the_llama_fixture_is_made_of_the_served_rules():
    m64, X, _ = rf.llama_fixture()
    sweep = _check_against_autograd(m64, X, n_seeds=2, kinds={NORM: 3, NEG: 2})
    assert len(_taps(m64)) == 9  # (embed, q, k, v, proj, w1, w3, w2, head: the oracle's nine KFAC blocks)
    assert all(isinstance(r.mod, nn.RMSNorm) for r in sweep.rule.values() if r.kind == NORM)


def test_the_kernel_branch_on_the_emulation_matches_autograd(emulated, monkeypatch):
    m64, X, _ = rf.llama_fixture()
    model, X32 = copy.deepcopy(m64).float(), X.float()
    taps = _taps(model)
    sweep = SeedBatchedSweep(model, taps, kernels=get_kernels)
    f = sweep.forward(X32)
    seeds = torch.randn(2, *f.shape, generator=torch.Generator().manual_seed(0))
    grads = sweep.backward(seeds)
    _, _, want = autograd_reference(m64, _taps(m64), X, seeds.double())
    for n in taps:
        assert rf.rel(grads[n], want[n]) < 1e-5, n
    # three layers on [B T, dim] rows; the final norm's VJP is not needed (nothing tapped lies before ... the embedding does)
    fwd = [s for s in emulated.seen if s[0] == "rmsnorm_forward"]
    vjp = [s for s in emulated.seen if s[0] == "rmsnorm_vjp"]
    assert fwd == [("rmsnorm_forward", 5 * 6, 32, True, pytest.approx(1e-6))] * 3
    assert vjp == [("rmsnorm_vjp", 2, 5 * 6, 32, True)] * 3
    # the switch, a kernel object without the entry points and another dtype all take the torch math, with the same numbers
    emulated.seen.clear()
    monkeypatch.setattr(SeedBatchedSweep, "use_rmsnorm_kernels", False)
    sweep.forward(X32)
    off = sweep.backward(seeds)
    assert not emulated.seen and all(rf.rel(off[n], grads[n]) < 1e-5 for n in taps)
    monkeypatch.setattr(SeedBatchedSweep, "use_rmsnorm_kernels", True)
    from tests.emulated_kernels import EmulatedKernels

    prev = _lib.set_kernels_for_testing(EmulatedKernels())
    try:
        sweep.forward(X32)
        stock = sweep.backward(seeds)
    finally:
        _lib.set_kernels_for_testing(prev)
    assert all(rf.rel(stock[n], grads[n]) < 1e-5 for n in taps)
    s64 = SeedBatchedSweep(m64, _taps(m64), kernels=get_kernels)
    s64.forward(X), s64.backward(seeds.double())
    assert not emulated.seen  # (fp64: torch math)


def test_curvature_on_the_emulation_matches_the_oracle(emulated, monkeypatch):
    """fails without the rules: the model takes the tape ("no VJP rule for module RMSNorm"), which `run_curvature_checks` refuses"""
    fixture = rf.llama_fixture()
    got = run_curvature_checks("cpu", fixture, want_split=False)
    calls = [s for s in emulated.seen if s[0] == "rmsnorm_vjp"]
    assert calls and {(s[2], s[3]) for s in calls} == {(B * 6, 32) for B in (2, 3, 5)}  # the batch of 5, the minibatches of 3 and 2
    emulated.seen.clear()
    monkeypatch.setattr(SeedBatchedSweep, "use_rmsnorm_kernels", False)
    ref = run_curvature_checks("cpu", fixture, want_split=False)
    assert not emulated.seen
    for k in ("Js", "f", "h", "f_var"):
        assert rf.rel(got[k], ref[k]) < 1e-4, k


# ---- 4. tracked RMSNorm weights ---------------------------------------------------------------------------------------------------------
def test_tracked_rmsnorm_weights_are_served_by_the_norm_taps(emulated):
    from laplace_amd import HipGGN
    from oracle import curvature_oracle as co

    m64, X64, y = rf.llama_fixture(track_norm=True)
    model, X = copy.deepcopy(m64).float(), X64.float()
    backend = HipGGN(model, "classification")
    tape = backend._tape()
    assert [t.name for t in tape.norm_taps] == ["blocks.0.norm1", "blocks.0.norm2", "norm"]
    assert all(t.kind == "norm" and t.w_off >= 0 and t.b_off == -1 for t in tape.norm_taps)
    assert tape.unserved == [] and backend._supported()
    Js64, f64 = co.jacobians(m64, X64)
    Js, f = backend.jacobians(X)
    assert Js.shape == Js64.shape == (5, 3, sum(p.numel() for p in m64.parameters() if p.requires_grad))
    assert rf.rel(f, f64) < 1e-5 and rf.rel(Js, Js64) < 1e-4, (rf.rel(f, f64), rf.rel(Js, Js64))
    for t in tape.norm_taps:  # (the layer's own columns, which are small beside the Linear layers')
        cols = slice(t.w_off, t.w_off + 32)
        assert rf.rel(Js[..., cols], Js64[..., cols]) < 1e-4, t.name
    assert getattr(tape, "sweep_reason", None) is None and tape.sweeps.get(frozenset({"norm"})) not in (None, False)
    _, h = backend.diag(X, y)
    assert rf.rel(h, co.ggn_diag(Js64, co.functional_hessian(f64, "classification"))) < 1e-4
    with pytest.raises(NotImplementedError, match="KFAC supports nn.Linear / nn.Conv2d parameters only"):
        backend.kron(X, y, N=len(X))


# ---- 5. the split sweep names the nodes -----------------------------------------------------------------------------------------------
class _Conv(nn.Module):
    def __init__(self, how):
        super().__init__()
        self.how, self.c0, self.c1, self.fc = how, nn.Conv2d(3, 32, 3, 1, 1), nn.Conv2d(32, 32, 3, 1, 1), nn.Linear(32, 3)
        self.norm = nn.RMSNorm(32)

    def forward(self, x):
        h = torch.tanh(self.c1(torch.tanh(self.c0(x))))
        if self.how == "neg":
            h = -h
        elif self.how == "sub":
            h = h - torch.sigmoid(h)
        h = h.mean((2, 3))
        return self.fc(self.norm(h) if self.how == "rmsnorm" else h)


@pytest.mark.parametrize("how,reason", (("rmsnorm", "norm: RMSNorm has no NHWC rule"), ("neg", "neg has no NHWC rule"),
                                        ("sub", "sub has no NHWC rule")))
def test_the_split_sweep_refuses_by_name_and_the_model_still_sweeps(how, reason, emulated):
    torch.manual_seed(14)
    m64 = _Conv(how).double().eval()
    X = torch.randn(3, 3, 6, 6, dtype=torch.float64)
    model = copy.deepcopy(m64).float()
    taps = _taps(model)
    sw = SplitSweep(model, taps, kernels=get_kernels)
    assert not sw.split_ok and sw.split_reason == reason
    f = sw.forward(X.float())
    seeds = torch.randn(2, *f.shape, generator=torch.Generator().manual_seed(1))
    grads = sw.backward(seeds)
    f_ref, _, want = autograd_reference(m64, _taps(m64), X, seeds.double())
    assert rf.rel(f, f_ref) < 1e-4  # (fp32 convolutions against fp64)
    for n in taps:
        assert rf.rel(grads[n], want[n]) < 1e-4, n
    # an attention node is still named first: a LLaMA block is on the NCHW walk because of it
    l64, _, _ = rf.llama_fixture()
    assert SplitSweep(l64.float(), _taps(l64), kernels=get_kernels).split_reason.endswith("scaled_dot_product_attention has no NHWC rule")
