"""The MUL rule of the seed-batched reverse sweep (laplace_amd/sweep.py) on the CPU: models that multiply two tensors of the graph
- squeeze-and-excitation gates, GLU / SwiGLU feed-forwards, self-gating, a frozen LayerScale - go through ONE sweep for all seeds and
match one autograd pass per seed; the curvature quantities built on it match the fp64 oracle; the kernel branch runs on the
emulation (tests/emulated_mul_kernels.py); the split sweep names the product and leaves the model to the NCHW walk; what the rule
does not serve is refused by name and the backend answers through the tape.

Before the rule existed every model here was refused whole - "no VJP rule for function mul" / "... method mul" at construction -
and took the autograd tape."""
import copy

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from laplace_amd import _lib
from laplace_amd._lib import get_kernels
from laplace_amd.sweep import CONST, MUL, SeedBatchedSweep, SweepUnsupported, mul_form
from laplace_amd.sweep_nhwc import SplitSweep
from tests import mul_fixtures as mf
from tests.norm_sweep_fixtures import autograd_reference


def _taps(model):
    return {n: m for n, m in model.named_modules() if isinstance(m, (nn.Linear, nn.Conv2d))}


# ---- 1. every spelling against autograd ------------------------------------------------------------------------------------------
SPELLINGS = {
    "operator": lambda a, b: a * b, "torch.mul": lambda a, b: torch.mul(a, b), "torch.multiply": lambda a, b: torch.multiply(a, b),
    "method-mul": lambda a, b: a.mul(b), "method-multiply": lambda a, b: a.multiply(b), "method-mul_": lambda a, b: a.mul_(b),
}


def _imul(a, b):
    a *= b
    return a


SPELLINGS["operator-imul"] = _imul
INPLACE = ("operator-imul", "method-mul_")  # (torch itself refuses these with the smaller operand first: written `*` there)


class Gate(nn.Module):
    """a squeeze-and-excitation gate ``[B, C, 1, 1]`` on a ``[B, C, H, W]`` map, as the first or the second operand; the gated map
    is also consumed whole and sliced.  The first operand is a node of its own (``h + 0``) whose value the VJP keeps: an in-place
    spelling evaluated in place would overwrite it"""

    def __init__(self, spell, gate_first):
        super().__init__()
        self.spell, self.gate_first = SPELLINGS["operator" if gate_first and spell in INPLACE else spell], gate_first
        self.c0, self.f1, self.f2, self.c1, self.fc = nn.Conv2d(3, 6, 3, 1, 1), nn.Conv2d(6, 2, 1), nn.Conv2d(2, 6, 1), nn.Conv2d(6, 4, 1), nn.Linear(4, 3)

    def forward(self, x):
        h = torch.tanh(self.c0(x))
        gate = torch.sigmoid(self.f2(torch.tanh(self.f1(F.adaptive_avg_pool2d(h, 1)))))
        y = self.spell(gate, h + 0) if self.gate_first else self.spell(h + 0, gate)
        z = self.c1(y + h) + y[:, 1:5] + y[:, :4]
        return self.fc(z.mean((2, 3)))


class Full(nn.Module):
    """the gated feed-forward ``w2(silu(w1 x) * w3 x)`` on ``[B, T, D]``, self-gating ``h * sigmoid(h)``, ``x * x`` and a ``[B, T, 1]``
    gate on either side"""

    def __init__(self, spell):
        super().__init__()
        self.spell, self.small_first = SPELLINGS[spell], SPELLINGS["operator" if spell in INPLACE else spell]
        self.embed, self.w1, self.w3, self.w2, self.g, self.fc = (nn.Linear(3, 6), nn.Linear(6, 7), nn.Linear(6, 7), nn.Linear(7, 6),
                                                                   nn.Linear(6, 1), nn.Linear(6, 3))

    def forward(self, x):
        x = self.embed(x.flatten(2).transpose(1, 2))  # [B, 16, 6]
        h = self.w2(self.spell(F.silu(self.w1(x)), self.w3(x)))
        h = self.spell(h + 0, torch.sigmoid(h))  # self-gating
        t = torch.tanh(self.g(x))  # [B, 16, 1]
        h = self.spell(h + 0, t) + self.small_first(t + 0, x)
        sq = h + 0
        return self.fc(self.small_first(sq, sq).mean(1))  # (autograd itself refuses ``sq.mul_(sq)``)


class LayerScale(nn.Module):
    """a frozen LayerScale ``gamma`` ``[C, 1, 1]`` on either side, and a frozen vector expanded to the operand's shape"""

    def __init__(self, spell):
        super().__init__()
        self.spell, self.const_first = SPELLINGS[spell], SPELLINGS["operator" if spell in INPLACE else spell]
        self.c0, self.c1, self.fc = nn.Conv2d(3, 6, 3, 1, 1), nn.Conv2d(6, 6, 1), nn.Linear(6, 3)
        self.gamma = nn.Parameter(torch.linspace(0.5, 1.5, 6).reshape(6, 1, 1), requires_grad=False)
        self.beta = nn.Parameter(torch.linspace(-1.0, 1.0, 6).reshape(1, 6, 1, 1), requires_grad=False)

    def forward(self, x):
        h = torch.tanh(self.c0(x))
        a = self.const_first(self.gamma, self.c1(h))
        b = self.spell(h + 0, self.beta.expand(h.size(0), -1, 4, 4))
        return self.fc((a + self.spell(b, self.gamma)).mean((2, 3)))


# (model, gate first) -> number of MUL nodes
MODELS = {("gate", False): 1, ("gate", True): 1, ("full", None): 5, ("layer-scale", None): 3}


def _build(kind, spell, gate_first):
    torch.manual_seed(11)
    cls = {"gate": lambda: Gate(spell, gate_first), "full": lambda: Full(spell), "layer-scale": lambda: LayerScale(spell)}[kind]
    return cls().double().eval(), torch.randn(5, 3, 4, 4, dtype=torch.float64)


@pytest.mark.parametrize("spell", sorted(SPELLINGS))
@pytest.mark.parametrize("kind,gate_first", sorted(MODELS, key=str))
def test_sweep_matches_one_autograd_pass_per_seed(kind, gate_first, spell):
    """fails without the rule: every model is refused at construction with "no VJP rule for function mul" (the methods: "... method
    mul")"""
    m64, X = _build(kind, spell, gate_first)
    taps = _taps(m64)
    sweep = SeedBatchedSweep(m64, taps, kernels=None)
    assert sum(r.kind == MUL for r in sweep.rule.values()) == MODELS[(kind, gate_first)]
    f = sweep.forward(X)
    forms = [sweep.saved[n][0] for n, r in sweep.rule.items() if r.kind == MUL]
    assert set(forms) == {"gate": {"row"}, "full": {"full", "row"}, "layer-scale": {"const"}}[kind]
    torch.manual_seed(0)
    seeds = torch.randn(4, *f.shape, dtype=torch.float64)
    grads = sweep.backward(seeds)
    f_ref, ins, want = autograd_reference(m64, taps, X, seeds)
    assert (f - f_ref.detach()).abs().max() <= 1e-12 * (1 + f_ref.abs().max())
    for n in taps:
        assert torch.equal(sweep.taps[n]["a"], ins[n]), n  # (no in-place spelling wrote into a kept tensor)
        assert grads[n].shape == want[n].shape, n
        assert (grads[n] - want[n]).abs().max() <= 1e-12 * (1 + want[n].abs().max()), n


def test_the_forms_are_resolved_on_the_shapes():
    assert mul_form((4, 6, 3, 3), (4, 6, 3, 3)) == ("full", None, 0)
    assert mul_form((4, 6, 1, 1), (4, 6, 3, 3)) == ("row", 0, 2) and mul_form((4, 6, 3, 3), (4, 6, 1, 1)) == ("row", 1, 2)
    assert mul_form((4, 5, 7), (4, 5, 1)) == ("row", 1, 2) and mul_form((4, 1, 1), (4, 5, 7)) == ("row", 0, 1)
    assert mul_form((4, 1, 1, 1), (4, 1, 3, 3)) == ("row", 0, 2)  # (a map with one channel: the gate is its trailing ones)
    for sa, sb in (((4, 1, 3, 3), (4, 6, 3, 3)), ((4, 5, 7), (4, 1, 7)), ((4, 6, 1, 3), (4, 6, 3, 3)), ((1, 6, 1, 1), (4, 6, 3, 3))):
        with pytest.raises(SweepUnsupported, match=r"mul of .* and .*needs a strided reduction"):
            mul_form(sa, sb)
    for sa, sb in (((4, 6), (4, 6, 3, 3)), ((4, 5, 7), (4, 5, 6)), ((6, 1, 1), (4, 6, 3, 3))):
        with pytest.raises(SweepUnsupported, match=r"mul of \(.*\) and \(.*\): the traced operands must have equal shapes"):
            mul_form(sa, sb)


def test_a_constant_and_the_input_receive_nothing():
    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = nn.Linear(4, 3)
            self.register_buffer("scale", torch.linspace(1, 2, 4))

        def forward(self, x):
            return self.fc(x * self.scale) * torch.sigmoid(x[:, :3])

    m = M().double().eval()
    sweep = SeedBatchedSweep(m, _taps(m), kernels=None)
    assert [r.kind for r in sweep.rule.values()].count(MUL) == 2 and [r.kind for r in sweep.rule.values()].count(CONST) == 1
    X = torch.randn(5, 4, dtype=torch.float64)
    f = sweep.forward(X)
    seeds = torch.randn(2, *f.shape, dtype=torch.float64)
    grads = sweep.backward(seeds)
    _, _, want = autograd_reference(m, _taps(m), X, seeds)
    assert (grads["fc"] - want["fc"]).abs().max() <= 1e-12 * (1 + want["fc"].abs().max())


# ---- 2. the kernel branch and the curvature on the emulation -------------------------------------------------------------------------
@pytest.fixture
def emulated():
    from tests.emulated_mul_kernels import EmulatedMulKernels

    K = EmulatedMulKernels()
    prev = _lib.set_kernels_for_testing(K)
    yield K
    _lib.set_kernels_for_testing(prev)


@pytest.mark.parametrize("kind,gate_first", sorted(MODELS, key=str))
def test_the_kernel_branch_on_the_emulation_matches_autograd(kind, gate_first, emulated, monkeypatch):
    m64, X = _build(kind, "operator", gate_first)
    model, X32 = copy.deepcopy(m64).float(), X.float()
    taps = _taps(model)
    sweep = SeedBatchedSweep(model, taps, kernels=get_kernels)
    f = sweep.forward(X32)
    seeds = torch.randn(3, *f.shape, generator=torch.Generator().manual_seed(0))
    grads = sweep.backward(seeds)
    _, _, want = autograd_reference(m64, _taps(m64), X, seeds.double())
    for n in taps:
        assert mf.rel(grads[n], want[n]) < 1e-5, n
    calls = [s for s in emulated.seen if s[0] == "mul_vjp"]
    if kind == "gate":  # ONE call: the gate is the kernel's b whichever side it is written on; R = B C rows of H W
        assert calls == [("mul_vjp", "row", 3, 5 * 6, 16, (True, True))]
    elif kind == "full":
        assert [c[1] for c in calls].count("full") == 3 and [c[1] for c in calls].count("row") == 2
        assert ("mul_vjp", "row", 3, 5 * 16, 6, (True, True)) in calls and ("mul_vjp", "full", 3, 5, 16 * 7, (True, True)) in calls
    else:
        assert not calls  # (a constant operand is plain torch math: no kernel)
    # the switch, a kernel object without the entry point and another dtype all take the torch math, with the same numbers
    emulated.seen.clear()
    monkeypatch.setattr(SeedBatchedSweep, "use_mul_kernels", False)
    sweep.forward(X32)
    off = sweep.backward(seeds)
    assert not emulated.seen and all(mf.rel(off[n], grads[n]) < 1e-5 for n in taps)
    monkeypatch.setattr(SeedBatchedSweep, "use_mul_kernels", True)
    from tests.emulated_kernels import EmulatedKernels

    prev = _lib.set_kernels_for_testing(EmulatedKernels())
    try:
        sweep.forward(X32)
        stock = sweep.backward(seeds)
    finally:
        _lib.set_kernels_for_testing(prev)
    assert all(mf.rel(stock[n], grads[n]) < 1e-5 for n in taps)


def test_non_contiguous_operands_are_made_contiguous(emulated):
    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b, self.fc = nn.Linear(4, 6), nn.Linear(4, 6), nn.Linear(5, 3)

        def forward(self, x):  # [B, 5, 4]
            return self.fc((self.a(x).transpose(1, 2) * self.b(x).transpose(1, 2)).mean(1))

    torch.manual_seed(3)
    m = M().eval()
    X = torch.randn(4, 5, 4)
    sweep = SeedBatchedSweep(m, _taps(m), kernels=get_kernels)
    f = sweep.forward(X)
    seeds = torch.randn(2, *f.shape)
    grads = sweep.backward(seeds)  # (the emulation asserts contiguity)
    assert [s[1] for s in emulated.seen] == ["full"]
    m64 = copy.deepcopy(m).double()
    _, _, want = autograd_reference(m64, _taps(m64), X.double(), seeds.double())
    assert all(mf.rel(grads[n], want[n]) < 1e-5 for n in grads)


@pytest.mark.parametrize("which", ("se", "swiglu"))
def test_curvature_on_the_emulation_matches_the_oracle(which, emulated, monkeypatch):
    """fails without the rule: the model takes the tape ("no VJP rule for function mul"), which `run_curvature_checks` refuses"""
    fixture = mf.se_fixture() if which == "se" else mf.swiglu_fixture()
    got = mf.run_curvature_checks("cpu", fixture, want_split=False)
    calls = [s for s in emulated.seen if s[0] == "mul_vjp"]
    assert calls and {s[1] for s in calls} == ({"row"} if which == "se" else {"full"})
    if which == "se":  # R = B C rows of H W elements, for the whole batch of 4 and the minibatches of 2
        assert {(s[3], s[4]) for s in calls} == {(B * 8, 64) for B in (2, 4)} | {(B * 16, 16) for B in (2, 4)}
        assert all(s[5] == (True, True) for s in calls)
    else:  # the whole batch of 3 and the minibatches of 2 and 1
        assert {(s[3], s[4]) for s in calls} == {(B, 5 * 85) for B in (1, 2, 3)}
    emulated.seen.clear()
    monkeypatch.setattr(SeedBatchedSweep, "use_mul_kernels", False)
    ref = mf.run_curvature_checks("cpu", fixture, want_split=False)
    assert not emulated.seen
    for k in ("Js", "f", "h", "f_var"):
        assert mf.rel(got[k], ref[k]) < 1e-4, k


# ---- 3. the split sweep names the product -----------------------------------------------------------------------------------------------
def test_the_split_sweep_refuses_by_name_and_the_model_still_sweeps(emulated):
    m64, X, _ = mf.se_fixture()
    model = copy.deepcopy(m64).float()
    taps = _taps(model)
    sw = SplitSweep(model, taps, kernels=get_kernels)
    assert not sw.split_ok and sw.split_reason == "mul has no NHWC rule"
    f = sw.forward(X.float())
    seeds = torch.randn(2, *f.shape, generator=torch.Generator().manual_seed(1))
    grads = sw.backward(seeds)
    f_ref, _, want = autograd_reference(m64, _taps(m64), X, seeds.double())
    assert mf.rel(f, f_ref) < 1e-5
    for n in taps:
        assert mf.rel(grads[n], want[n]) < 1e-4, n
    assert any(s[0] == "mul_vjp" for s in emulated.seen)
    # an attention node is still named first: a transformer block is on the NCHW walk because of it
    v64, _, _ = mf.swiglu_fixture()
    assert SplitSweep(v64.float(), _taps(v64), kernels=get_kernels).split_reason.endswith("scaled_dot_product_attention has no NHWC rule")


# ---- 4. refusals by name; the tape answers ---------------------------------------------------------------------------------------------
class _Refused(nn.Module):
    def __init__(self, how):
        super().__init__()
        self.how, self.c0, self.fc = how, nn.Conv2d(3, 4, 3, 1, 1), nn.Linear(4, 3)
        if how == "channel-gate":
            self.g = nn.Conv2d(4, 1, 1)

    def forward(self, x):
        how, h = self.how, torch.tanh(self.c0(x))
        if how == "number":
            h = h * 2.0
        elif how == "number-first":
            h = 2.0 * h
        elif how == "out":
            h = torch.mul(h, torch.sigmoid(h), out=h)
        elif how == "keyword":
            h = torch.mul(h, other=torch.sigmoid(h))
        elif how == "channel-gate":
            h = h * torch.sigmoid(self.g(h))  # [B, 1, H, W]
        elif how == "token-gate":
            t = h.flatten(2)  # [B, 4, 16]
            h = (t * torch.sigmoid(t.mean(1, keepdim=True))).view(-1, 4, 4, 4)  # [B, 1, 16]
        elif how == "expand_as":
            h = h * torch.sigmoid(F.adaptive_avg_pool2d(h, 1)).expand_as(h)
        return self.fc(h.mean((2, 3)))


AT_CONSTRUCTION = {"number": "mul by the Python number 2.0 is not served", "number-first": "mul by the Python number 2.0 is not served",
                   "out": "mul with an out= argument", "keyword": r"mul: expected two positional operands, got 1 and the keywords \['other'\]",
                   "expand_as": "method expand_as of a traced tensor"}
IN_THE_FORWARD = {"channel-gate": r"mul of \(3, 4, 4, 4\) and \(3, 1, 4, 4\): .*needs a strided reduction",
                  "token-gate": r"mul of \(3, 4, 16\) and \(3, 1, 16\): .*needs a strided reduction"}


def _tape_answers(model, X, fragment):
    """the backend falls to the tape with the refusal as its reason, and gives the oracle's numbers"""
    from laplace_amd import HipGGN
    from oracle import curvature_oracle as co
    from tests.emulated_mul_kernels import EmulatedMulKernels

    prev = _lib.set_kernels_for_testing(EmulatedMulKernels())
    try:
        backend = HipGGN(model, "classification")
        Js, f = backend.jacobians(X)
        assert fragment in backend._tape().sweep_reason, backend._tape().sweep_reason
        y = torch.arange(X.shape[0]) % 3
        _, h = backend.diag(X, y)
    finally:
        _lib.set_kernels_for_testing(prev)
    m64 = copy.deepcopy(model).double()
    Js64, f64 = co.jacobians(m64, X.double())
    assert mf.rel(f, f64) < 1e-5 and mf.rel(Js, Js64) < 1e-4
    assert mf.rel(h, co.ggn_diag(Js64, co.functional_hessian(f64, "classification"))) < 1e-4


@pytest.mark.parametrize("how", sorted(AT_CONSTRUCTION))
def test_what_is_not_served_is_refused_at_construction_and_the_tape_answers(how):
    torch.manual_seed(1)
    model, X = _Refused(how).eval(), torch.randn(3, 3, 4, 4)
    with pytest.raises(SweepUnsupported, match=AT_CONSTRUCTION[how]) as e:
        SeedBatchedSweep(model, _taps(model), kernels=None)
    if how != "expand_as":
        assert "mul" in str(e.value)
    if how == "out":  # (autograd itself refuses an out= argument on a tensor that requires grad: there is no tape to answer)
        return
    _tape_answers(model, X, {"number": "mul by the Python number", "number-first": "mul by the Python number", "out": "out= argument",
                             "keyword": "two positional operands", "expand_as": "expand_as of a traced tensor"}[how])


@pytest.mark.parametrize("how", sorted(IN_THE_FORWARD))
def test_what_only_the_shapes_tell_is_refused_in_the_forward_and_the_tape_answers(how):
    torch.manual_seed(1)
    model, X = _Refused(how).eval(), torch.randn(3, 3, 4, 4)
    sweep = SeedBatchedSweep(model, _taps(model), kernels=None)
    with pytest.raises(SweepUnsupported, match=IN_THE_FORWARD[how]):
        sweep.forward(X)
    _tape_answers(model, X, "needs a strided reduction")


def test_a_constant_that_the_operand_would_broadcast_to_is_refused():
    class Wide(nn.Module):
        def __init__(self):
            super().__init__()
            self.l, self.fc = nn.Linear(4, 4), nn.Linear(4, 3)
            self.register_buffer("table", torch.ones(5, 4))

        def forward(self, x):  # x [B, 4]; l(x)[:, None] is [B, 1, 4] and broadcasts against the [5, 4] table to [B, 5, 4]
            return self.fc((self.l(x).view(-1, 1, 4) * self.table).mean(1))

    m = Wide().eval()
    sweep = SeedBatchedSweep(m, _taps(m), kernels=None)
    with pytest.raises(SweepUnsupported, match=r"mul: \(3, 1, 4\) broadcasts against the constant table of shape \(5, 4\)"):
        sweep.forward(torch.randn(3, 4))


def test_two_constants_are_refused():
    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = nn.Linear(4, 3)
            self.u, self.v = (nn.Parameter(torch.ones(4), requires_grad=False) for _ in range(2))  # (fx folds plain buffers)

        def forward(self, x):
            return self.fc(x + self.u * self.v)

    with pytest.raises(SweepUnsupported, match="mul of two constants"):
        SeedBatchedSweep(M().eval(), {}, kernels=None)
