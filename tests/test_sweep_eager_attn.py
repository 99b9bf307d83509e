"""The MATMUL, SOFTMAX and SCALE rules of the seed-batched reverse sweep (laplace_amd/sweep.py) on the CPU: models that write
attention out - ``softmax(q @ k^T / sqrt(d) [+ bias]) @ v`` -, attention pooling, ``x @ x^T``, products with a frozen matrix,
log-softmax head features and softmaxes over another dim go through ONE sweep for all seeds and match one autograd pass per seed;
the curvature quantities built on it match the fp64 oracle; the kernel branches run on the emulations
(tests/emulated_softmax_kernels.py, tests/emulated_matmul_kernels.py); the split sweep names the matrix product and leaves the model
to the NCHW walk; what the rules do not serve is refused by name and the backend answers through the tape.

Before the rules existed every model here was refused whole - "no VJP rule for function matmul" / "... method softmax" /
"... function truediv" (or the spelling's own name) at construction - and took the autograd tape."""
import copy
import math
import warnings

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from laplace_amd import _lib
from laplace_amd._lib import get_kernels
from laplace_amd.sweep import CONST, MATMUL, SCALE, SOFTMAX, SeedBatchedSweep, SweepUnsupported, matmul_vjp_math, softmax_vjp_math
from laplace_amd.sweep_nhwc import SplitSweep
from tests import eager_attn_fixtures as ef
from tests.norm_sweep_fixtures import autograd_reference


def _taps(model):
    return {n: m for n, m in model.named_modules() if isinstance(m, (nn.Linear, nn.Conv2d))}


def _idiv(a, c):
    a /= c
    return a


MATMULS = {"operator": lambda a, b: a @ b, "torch.matmul": lambda a, b: torch.matmul(a, b), "method-matmul": lambda a, b: a.matmul(b),
           "torch.bmm": lambda a, b: torch.bmm(a, b), "method-bmm": lambda a, b: a.bmm(b)}
SOFTMAXES = {"F": lambda t, d: F.softmax(t, d), "F-keyword": lambda t, d: F.softmax(t, dim=d), "torch": lambda t, d: torch.softmax(t, d),
             "method": lambda t, d: t.softmax(d), "method-keyword": lambda t, d: t.softmax(dim=d), "module": None}
LOG_SOFTMAXES = {"F": lambda t, d: F.log_softmax(t, d), "torch": lambda t, d: torch.log_softmax(t, dim=d),
                 "method": lambda t, d: t.log_softmax(d), "module": None}
DIVS = {"operator": lambda a, c: a / c, "torch.div": lambda a, c: torch.div(a, c), "torch.true_divide": lambda a, c: torch.true_divide(a, c),
        "method-div": lambda a, c: a.div(c), "method-true_divide": lambda a, c: a.true_divide(c), "method-div_": lambda a, c: a.div_(c),
        "operator-idiv": _idiv}


class Eager(nn.Module):
    """one attention layer on ``[B, T, 6]`` tokens written out, then a head.  ``shape``: ``"heads"`` (``[B, 2, T, 4]`` operands),
    ``"single"`` (``[B, T, 8]``: what ``bmm`` takes), ``"cross"`` (three pooled queries against all T keys: Tq != Tk); ``bias``: a
    frozen ``[1, H, T, T]`` buffer on the scores; ``head``: ``"mean"``, ``"log-features"`` (log-softmax of the features before the
    head) or ``"token-softmax"`` (attention pooling: a softmax over the token dim, dim 1, weighs the tokens)"""

    def __init__(self, mm="operator", sm="method", div="operator", shape="heads", bias=False, head="mean", T=5):
        super().__init__()
        self.mm, self.sm, self.div, self.shape, self.head_kind = MATMULS[mm], SOFTMAXES[sm], DIVS[div], shape, head
        self.heads, self.head_dim = (2, 4) if shape != "single" else (1, 8)
        self.q, self.k, self.v, self.proj, self.fc = nn.Linear(6, 8), nn.Linear(6, 8), nn.Linear(6, 8), nn.Linear(8, 8), nn.Linear(8, 3)
        self.softmax = nn.Softmax(-1) if sm == "module" else None
        self.log_softmax = nn.LogSoftmax(-1) if head == "log-features" else None
        self.gate = nn.Linear(8, 1) if head == "token-softmax" else None
        if bias:
            lead = (1, self.heads) if shape != "single" else (1,)
            self.register_buffer("bias", torch.randn(*lead, 3 if shape == "cross" else T, T))
        else:
            self.bias = None

    def split(self, t, B):
        return t.view(B, -1, self.heads, self.head_dim).transpose(1, 2) if self.shape != "single" else t

    def forward(self, x):
        B = x.size(0)
        q, k, v = self.split(self.q(x[:, :3] if self.shape == "cross" else x), B), self.split(self.k(x), B), self.split(self.v(x), B)
        scores = self.div(self.mm(q, k.transpose(-2, -1)), math.sqrt(self.head_dim))
        if self.bias is not None:
            scores = scores + self.bias
        p = self.softmax(scores) if self.softmax is not None else self.sm(scores, -1)
        o = self.mm(p, v)
        o = o.transpose(1, 2).reshape(B, -1, 8) if self.shape != "single" else o
        h = torch.tanh(self.proj(o))
        if self.head_kind == "log-features":
            return self.fc(self.log_softmax(h).mean(1))
        if self.head_kind == "token-softmax":
            w = torch.softmax(self.gate(h), 1)  # [B, T, 1] over the tokens
            return self.fc((w.transpose(1, 2) @ h).flatten(1))
        return self.fc(h.mean(1))


def _build(**kw):
    torch.manual_seed(13)
    return Eager(**kw).double().eval(), torch.randn(4, 5, 6, dtype=torch.float64)


def _against_autograd(m64, X, S=4, tol=1e-12):
    taps = _taps(m64)
    sweep = SeedBatchedSweep(m64, taps, kernels=None)
    f = sweep.forward(X)
    seeds = torch.randn(S, *f.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    grads = sweep.backward(seeds)
    f_ref, ins, want = autograd_reference(m64, taps, X, seeds)
    assert (f - f_ref.detach()).abs().max() <= tol * (1 + f_ref.abs().max())
    for n in taps:
        assert torch.equal(sweep.taps[n]["a"], ins[n]), n  # (no in-place spelling wrote into a kept tensor)
        assert grads[n].shape == want[n].shape, n
        assert (grads[n] - want[n]).abs().max() <= tol * (1 + want[n].abs().max()), n
    return sweep


# ---- 1. every spelling against autograd ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", (False, True), ids=("plain", "bias"))
@pytest.mark.parametrize("mm", sorted(MATMULS))
def test_every_matmul_spelling_matches_one_autograd_pass_per_seed(mm, bias):
    """fails without the rule: "no VJP rule for function matmul" (``bmm``, "method matmul", ...) at construction"""
    sweep = _against_autograd(*_build(mm=mm, shape="single" if "bmm" in mm else "heads", bias=bias))
    kinds = [r.kind for r in sweep.rule.values()]
    assert kinds.count(MATMUL) == 2 and kinds.count(SOFTMAX) == 1 and kinds.count(SCALE) == 1 and kinds.count(CONST) == int(bias)
    assert all(sweep.saved[n][0] == "full" for n, r in sweep.rule.items() if r.kind == MATMUL)


@pytest.mark.parametrize("sm", sorted(SOFTMAXES))
def test_every_softmax_spelling_matches_one_autograd_pass_per_seed(sm):
    """fails without the rule: "no VJP rule for method softmax" / "function softmax" / "module Softmax" at construction"""
    _against_autograd(*_build(sm=sm, bias=True))


@pytest.mark.parametrize("div", sorted(DIVS))
def test_every_division_spelling_matches_one_autograd_pass_per_seed(div):
    """fails without the rule: "no VJP rule for function truediv" (``div``, "method div_", ...) at construction; the in-place
    spellings (``/=``, ``div_``) are evaluated out of place: the tapped inputs keep their values"""
    _against_autograd(*_build(div=div))


class LogHead(nn.Module):
    def __init__(self, spell):
        super().__init__()
        self.spell, self.l1, self.fc = LOG_SOFTMAXES[spell], nn.Linear(6, 7), nn.Linear(7, 3)
        self.mod = nn.LogSoftmax(2) if spell == "module" else None

    def forward(self, x):
        h = self.l1(x)
        h = self.mod(h) if self.mod is not None else self.spell(h, -1)
        return self.fc(h.mean(1))


@pytest.mark.parametrize("spell", sorted(LOG_SOFTMAXES))
def test_every_log_softmax_spelling_matches_one_autograd_pass_per_seed(spell):
    """fails without the rule: "no VJP rule for function log_softmax" / "method log_softmax" / "module LogSoftmax\""""
    torch.manual_seed(5)
    sweep = _against_autograd(LogHead(spell).double().eval(), torch.randn(4, 5, 6, dtype=torch.float64))
    (saved,) = [sweep.saved[n] for n, r in sweep.rule.items() if r.kind == SOFTMAX]
    assert saved[1:] == (2, True)  # (the dim resolved on the value, the log form)


@pytest.mark.parametrize("kw", [dict(shape="cross"), dict(shape="cross", bias=True), dict(head="log-features"), dict(head="token-softmax"),
                                dict(shape="single", sm="module")], ids=lambda kw: "-".join(f"{v}" for v in kw.values()))
def test_cross_attention_log_features_and_a_softmax_over_another_dim(kw):
    """Tq != Tk (three queries, five keys), log-softmax features, attention pooling with a softmax over dim 1 (a traced
    ``[B, 1, T] @ [B, T, D]`` product behind it) - each refused without the rules"""
    sweep = _against_autograd(*_build(**kw))
    dims = [sweep.saved[n][1] for n, r in sweep.rule.items() if r.kind == SOFTMAX]
    if kw.get("head") == "token-softmax":
        assert 1 in dims


class Others(nn.Module):
    """``x @ x^T`` (one node is both operands), a frozen matrix on the right (2-D) and on the left (2-D, and with leading ones)"""

    def __init__(self):
        super().__init__()
        self.l1, self.fc = nn.Linear(6, 8), nn.Linear(4, 3)
        self.right = nn.Parameter(torch.randn(8, 4), requires_grad=False)
        self.left = nn.Parameter(torch.randn(3, 5), requires_grad=False)
        self.left3 = nn.Parameter(torch.randn(1, 5, 5), requires_grad=False)

    def forward(self, x):
        h = torch.tanh(self.l1(x))  # [B, 5, 8]
        gram = h @ h.transpose(-2, -1)  # [B, 5, 5]
        h = torch.softmax(gram / 8, -1) @ h
        h = self.left3 @ (h @ self.right)  # [B, 5, 4]
        return self.fc((self.left @ h).mean(1))


def test_a_node_on_both_sides_and_a_constant_on_either_side():
    torch.manual_seed(2)
    sweep = _against_autograd(Others().double().eval(), torch.randn(4, 5, 6, dtype=torch.float64))
    forms = [(sweep.saved[n][0], sweep.saved[n][3]) for n, r in sweep.rule.items() if r.kind == MATMUL]
    assert forms == [("full", None), ("full", None), ("const", 1), ("const", 0), ("const", 0)]


def test_the_torch_math_of_the_rules_is_chunked_under_a_memory_cap():
    gen = torch.Generator().manual_seed(1)
    S, B = 5, 2
    a, b = torch.randn(B, 3, 4, 6, generator=gen, dtype=torch.float64), torch.randn(B, 3, 6, 5, generator=gen, dtype=torch.float64)
    g = torch.randn(S * B, 3, 4, 5, generator=gen, dtype=torch.float64)
    want = matmul_vjp_math(g, a, b, S)
    for cap in (1, (a.numel() + b.numel()) * 8 * 2, 1 << 40):
        got = matmul_vjp_math(g, a, b, S, max_bytes=cap)
        assert all(torch.equal(x, y) for x, y in zip(got, want))
    assert matmul_vjp_math(g, a, b, S, (True, False))[1] is None and matmul_vjp_math(g, a, b, S, (False, True))[0] is None
    ref = torch.einsum("sbhmn,bhkn->sbhmk", g.reshape(S, B, 3, 4, 5), b).reshape(S * B, 3, 4, 6)
    assert (want[0] - ref).abs().max() < 1e-12
    y = torch.softmax(torch.randn(B, 3, 4, generator=gen, dtype=torch.float64), 1)
    gs = torch.randn(S * B, 3, 4, generator=gen, dtype=torch.float64)
    for is_log in (False, True):
        yy = y.log() if is_log else y
        full = softmax_vjp_math(gs, yy, S, 1, is_log)
        assert torch.equal(softmax_vjp_math(gs, yy, S, 1, is_log, max_bytes=1), full)
        x = torch.randn(B, 3, 4, dtype=torch.float64, requires_grad=True)
        out = torch.log_softmax(x, 1) if is_log else torch.softmax(x, 1)
        yd = out.detach()
        one = torch.autograd.grad(out, x, gs[:B])[0]
        assert (softmax_vjp_math(gs, yd, S, 1, is_log)[:B] - one).abs().max() < 1e-12


# ---- 2. the kernel branches and the curvature on the emulations ----------------------------------------------------------------------
@pytest.fixture
def emulated(monkeypatch):
    from tests.emulated_matmul_kernels import EmulatedEagerAttnKernels

    K = EmulatedEagerAttnKernels()
    prev = _lib.set_kernels_for_testing(K)
    monkeypatch.setattr(SeedBatchedSweep, "use_matmul_kernels", True)
    monkeypatch.setattr(SeedBatchedSweep, "use_softmax_kernels", True)
    yield K
    _lib.set_kernels_for_testing(prev)


def _sweep32(m64, X, S=3):
    model, X32 = copy.deepcopy(m64).float(), X.float()
    taps = _taps(model)
    sweep = SeedBatchedSweep(model, taps, kernels=get_kernels)
    f = sweep.forward(X32)
    seeds = torch.randn(S, *f.shape, generator=torch.Generator().manual_seed(0))
    grads = sweep.backward(seeds)
    _, _, want = autograd_reference(m64, _taps(m64), X, seeds.double())
    return sweep, X32, seeds, grads, want


def test_the_kernel_branches_on_the_emulations_match_autograd(emulated, monkeypatch):
    m64, X = _build(bias=True, head="token-softmax")
    sweep, X32, seeds, grads, want = _sweep32(m64, X)
    for n in grads:
        assert ef.rel(grads[n], want[n]) < 1e-5, n
    # q @ k^T and p @ v on [4 x 2] sample matrices (k^T arrives as a view: the emulation asserts contiguity), the pooling product
    # [B, 1, T] @ [B, T, 8]; the softmax over the keys on the kernel, the one over the tokens (dim 1) on the torch math
    assert [s for s in emulated.seen if s[0] == "matmul_vjp"] == [("matmul_vjp", 3, 4, 1, 5, 8, (True, True)),
                                                                   ("matmul_vjp", 3, 8, 5, 5, 4, (True, True)),
                                                                   ("matmul_vjp", 3, 8, 5, 4, 5, (True, True))]
    assert [s for s in emulated.seen if s[0] == "softmax_vjp"] == [("softmax_vjp", "softmax", 3, 4 * 2 * 5, 5)]
    # each switch alone, a kernel object without the entry points and another dtype take the torch math, with the same numbers
    for name, gone in (("use_matmul_kernels", "matmul_vjp"), ("use_softmax_kernels", "softmax_vjp")):
        emulated.seen.clear()
        monkeypatch.setattr(SeedBatchedSweep, name, False)
        sweep.forward(X32)
        off = sweep.backward(seeds)
        assert emulated.seen and not any(s[0] == gone for s in emulated.seen)
        assert all(ef.rel(off[n], grads[n]) < 1e-5 for n in grads)
        monkeypatch.setattr(SeedBatchedSweep, name, True)
    from tests.emulated_kernels import EmulatedKernels

    prev = _lib.set_kernels_for_testing(EmulatedKernels())
    try:
        sweep.forward(X32)
        stock = sweep.backward(seeds)
    finally:
        _lib.set_kernels_for_testing(prev)
    assert all(ef.rel(stock[n], grads[n]) < 1e-5 for n in grads)
    emulated.seen.clear()
    _against_autograd(m64, X)  # (fp64, kernels=None)
    sw64 = SeedBatchedSweep(m64, _taps(m64), kernels=get_kernels)
    f = sw64.forward(X)
    sw64.backward(torch.randn(2, *f.shape, dtype=torch.float64))
    assert not emulated.seen


def test_a_constant_operand_and_the_log_form_on_the_emulations(emulated):
    torch.manual_seed(2)
    _, _, _, grads, want = _sweep32(Others().double().eval(), torch.randn(4, 5, 6, dtype=torch.float64))
    assert all(ef.rel(grads[n], want[n]) < 1e-5 for n in grads)
    # x @ x^T (x receives both parts) and softmax(..) @ h on the kernel; a constant operand is plain torch math: no kernel
    assert [s[1:] for s in emulated.seen if s[0] == "matmul_vjp"] == [(3, 4, 5, 5, 8, (True, True)), (3, 4, 5, 8, 5, (True, True))]
    emulated.seen.clear()
    torch.manual_seed(5)
    _, _, _, grads, want = _sweep32(LogHead("F").double().eval(), torch.randn(4, 5, 6, dtype=torch.float64))
    assert all(ef.rel(grads[n], want[n]) < 1e-5 for n in grads)
    assert emulated.seen == [("softmax_vjp", "log", 3, 20, 7)]


def test_the_defaults_of_the_switches_are_the_documented_ones():
    """README.md states them next to the measurement that decided them (tools/eager_attn_bench.py)"""
    import os

    readme = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "README.md")).read()
    for name in ("use_matmul_kernels", "use_softmax_kernels"):
        assert f"`{name} = {getattr(SeedBatchedSweep, name)}`" in readme, name


@pytest.mark.parametrize("T,bias", [(5, True), (17, False)], ids=("T5-bias", "T17-plain"))
def test_curvature_on_the_emulations_matches_the_oracle(T, bias, emulated, monkeypatch):
    """fails without the rules: the model takes the tape ("no VJP rule for function matmul"), which `run_curvature_checks` refuses"""
    fixture = ef.vit_eager_fixture(T=T, rel_bias=bias, softmax_module=bias)
    got = ef.run_curvature_checks("cpu", fixture, want_split=False)
    mm, sm = [s for s in emulated.seen if s[0] == "matmul_vjp"], [s for s in emulated.seen if s[0] == "softmax_vjp"]
    # two heads of dim 16 on T tokens, for the whole batch of 3 and the minibatches of 2 and 1
    assert {s[2:6] for s in mm} == {(B * 2, T, 16, T) for B in (1, 2, 3)} | {(B * 2, T, T, 16) for B in (1, 2, 3)}
    assert {s[3:] for s in sm} == {(B * 2 * T, T) for B in (1, 2, 3)} and all(s[6] == (True, True) for s in mm)
    emulated.seen.clear()
    monkeypatch.setattr(SeedBatchedSweep, "use_matmul_kernels", False)
    monkeypatch.setattr(SeedBatchedSweep, "use_softmax_kernels", False)
    ref = ef.run_curvature_checks("cpu", fixture, want_split=False)
    assert not emulated.seen
    for k in ("Js", "f", "h", "f_var"):
        assert ef.rel(got[k], ref[k]) < 1e-4, k


# ---- 3. the split sweep names the node ---------------------------------------------------------------------------------------------
def test_the_split_sweep_refuses_by_name_and_the_model_still_sweeps(emulated):
    m64, X, _ = ef.vit_eager_fixture()
    model = copy.deepcopy(m64).float()
    taps = _taps(model)
    sw = SplitSweep(model, taps, kernels=get_kernels)
    assert not sw.split_ok and sw.split_reason == "matmul has no NHWC rule"
    f = sw.forward(X.float())
    seeds = torch.randn(2, *f.shape, generator=torch.Generator().manual_seed(1))
    grads = sw.backward(seeds)
    f_ref, _, want = autograd_reference(m64, _taps(m64), X, seeds.double())
    assert ef.rel(f, f_ref) < 1e-5
    for n in taps:
        assert ef.rel(grads[n], want[n]) < 1e-4, n
    assert any(s[0] == "matmul_vjp" for s in emulated.seen) and any(s[0] == "softmax_vjp" for s in emulated.seen)
    torch.manual_seed(5)
    assert SplitSweep(LogHead("F").eval(), {}, kernels=get_kernels).split_reason == "log_softmax has no NHWC rule"

    class Div(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = nn.Linear(4, 3)

        def forward(self, x):
            return self.fc(x) / 2

    assert SplitSweep(Div().eval(), {}, kernels=get_kernels).split_reason == "div has no NHWC rule"


# ---- 4. refusals by name; the tape answers ---------------------------------------------------------------------------------------------
class _Refused(nn.Module):
    def __init__(self, how):
        super().__init__()
        self.how, self.l1, self.fc = how, nn.Linear(6, 6), nn.Linear(6, 3)
        self.u, self.w = (nn.Parameter(torch.randn(6, 6), requires_grad=False) for _ in range(2))

    def forward(self, x):  # [B, 2, 6]
        how, h = self.how, torch.tanh(self.l1(x))
        ht = h.transpose(-2, -1)
        if how == "matmul-out":
            h = torch.matmul(h, ht, out=h)
        elif how == "matmul-keyword":
            h = torch.matmul(h, other=self.w)
        elif how == "matmul-2d":
            h = (h.mean(1) @ self.w).view(-1, 1, 6) + h  # a traced [B, 6] operand
        elif how == "matmul-broadcast":
            h = (h.view(-1, 2, 1, 6) @ ht.reshape(-1, 1, 6, 2)).mean(3) + h  # [B, 2, 1, 6] @ [B, 1, 6, 2]
        elif how == "matmul-constants":
            h = h + self.u @ self.w
        elif how == "einsum":
            h = torch.einsum("btd,bsd->bts", h, h) @ h
        elif how == "baddbmm":
            h = torch.baddbmm(h, h, self.w.expand(x.size(0), 6, 6))
        elif how == "softmax-dtype":
            h = F.softmax(h, -1, dtype=torch.float64).to(h.dtype)
        elif how == "softmax-dtype-method":
            h = h.softmax(-1, torch.float64).to(h.dtype)
        elif how == "softmax-implicit":
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                h = F.softmax(h)
        elif how == "softmax-none":
            h = F.log_softmax(h, dim=None, _stacklevel=5)
        elif how == "softmax-batch":
            h = torch.softmax(h, 0)
        elif how == "softmax-batch-negative":
            h = h.softmax(-3)
        elif how == "softmax-traced-dim":
            h = h.softmax(x.size(1))  # (two tokens: dim 2, the last one)
        elif how == "div-rounding":
            h = torch.div(h, 2.0, rounding_mode="floor") + h
        elif how == "div-number-first":
            h = 2.0 / (h + 3.0)
        elif how == "div-traced":
            h = h / x.size(-1)
        elif how == "div-tensors":
            h = h / (h * h + 1.0)
        return self.fc(h.mean(1))


AT_CONSTRUCTION = {
    "matmul-out": "matmul with an out= argument", "matmul-keyword": r"matmul: expected two positional operands, got 1 and the keywords \['other'\]",
    "matmul-constants": "matmul of two constants",
    "einsum": "einsum is out of scope: matmul, @ and bmm are what the sweep serves",
    "baddbmm": "baddbmm is out of scope: matmul, @ and bmm are what the sweep serves",
    "softmax-dtype": "softmax with dtype=", "softmax-dtype-method": "softmax with dtype=",
    "softmax-implicit": "softmax without a dim .*implicit-dim legacy", "softmax-none": "log_softmax without a dim .*implicit-dim legacy",
    "softmax-batch": r"softmax along dim 0 \(the batch dim", "softmax-traced-dim": "softmax with a data-dependent dim",
    "div-rounding": "div with a rounding_mode", "div-number-first": r"div of the number 2.0 by a tensor \(number / tensor",
    "div-traced": "div by the traced value size", "div-tensors": r"div of the tensor \w+ by the tensor \w+ \(tensor / tensor needs the quotient rule: out of scope\)",
}
IN_THE_FORWARD = {
    "matmul-2d": r"matmul of \(3, 6\) and \(6, 6\): a traced operand must be \[B, \*, rows, columns\].*the VJP needs a reduction",
    "matmul-broadcast": r"matmul of \(3, 2, 1, 6\) and \(3, 1, 6, 2\): the leading dims .*the VJP needs a reduction",
    "softmax-batch-negative": r"softmax along dim -3 of a value with 3 dims \(the batch dim",
}
# autograd refuses an out= argument itself; two constants leave nothing traced to differentiate; a softmax over the batch dim (the
# implicit-dim legacy picks dim 0 for a 3-D value) mixes the samples, so the per-sample oracle is not its reference
NO_TAPE = ("matmul-out", "matmul-constants", "softmax-batch", "softmax-implicit", "softmax-none")


def _tape_answers(model, X, fragment):
    """the backend falls to the tape with the refusal as its reason, and gives the oracle's numbers"""
    from laplace_amd import HipGGN
    from oracle import curvature_oracle as co
    from tests.emulated_matmul_kernels import EmulatedEagerAttnKernels

    prev = _lib.set_kernels_for_testing(EmulatedEagerAttnKernels())
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
    assert ef.rel(f, f64) < 1e-5 and ef.rel(Js, Js64) < 1e-4
    assert ef.rel(h, co.ggn_diag(Js64, co.functional_hessian(f64, "classification"))) < 1e-4


@pytest.mark.parametrize("how", sorted(AT_CONSTRUCTION))
def test_what_is_not_served_is_refused_at_construction_and_the_tape_answers(how):
    torch.manual_seed(1)
    model, X = _Refused(how).eval(), torch.randn(3, 2, 6)
    with pytest.raises(SweepUnsupported, match=AT_CONSTRUCTION[how]) as e:
        SeedBatchedSweep(model, _taps(model), kernels=None)
    word = "matmul" if how in ("einsum", "baddbmm") else how.split("-")[0]
    assert word in str(e.value)
    if how in NO_TAPE:
        return
    _tape_answers(model, X, {"matmul-keyword": "two positional operands", "einsum": "einsum is out of scope", "baddbmm": "baddbmm is out of scope",
                             "softmax-dtype": "with dtype=", "softmax-dtype-method": "with dtype=", "softmax-implicit": "without a dim",
                             "softmax-none": "without a dim", "softmax-batch": "the batch dim", "softmax-traced-dim": "data-dependent dim",
                             "div-rounding": "rounding_mode", "div-number-first": "number / tensor", "div-traced": "traced value",
                             "div-tensors": "quotient rule"}[how])


@pytest.mark.parametrize("how", sorted(IN_THE_FORWARD))
def test_what_only_the_shapes_tell_is_refused_in_the_forward_and_the_tape_answers(how):
    torch.manual_seed(1)
    model, X = _Refused(how).eval(), torch.randn(3, 2, 6)
    sweep = SeedBatchedSweep(model, _taps(model), kernels=None)
    with pytest.raises(SweepUnsupported, match=IN_THE_FORWARD[how]) as e:
        sweep.forward(X)
    assert how.split("-")[0] in str(e.value)
    if "softmax" not in how:  # (a softmax over the batch dim mixes the samples: the per-sample oracle is not its reference)
        _tape_answers(model, X, "the VJP needs a reduction")


def test_an_operand_that_is_no_tensor_is_refused():
    """torch itself refuses ``matmul(tensor, number)`` while tracing; the rule's own check is met on a hand-built graph"""
    import torch.fx as fx

    from laplace_amd.sweep import classify

    for target, args in ((torch.matmul, (None, 2.0)), (torch.bmm, ([1.0], None)), ("matmul", (None, 3))):
        g = fx.Graph()
        x = g.placeholder("x")
        args = tuple(x if a is None else a for a in args)
        n = g.call_method(target, args) if isinstance(target, str) else g.call_function(target, args)
        with pytest.raises(SweepUnsupported, match=r"matmul: an operand is not a tensor of the graph \((float|immutable_list|int)\)"):
            classify(n, {})


def test_a_constant_operand_of_another_rank_is_refused():
    class Wide(nn.Module):
        def __init__(self):
            super().__init__()
            self.l, self.fc = nn.Linear(4, 4), nn.Linear(4, 3)
            self.register_buffer("table", torch.ones(2, 7, 4, 4))

        def forward(self, x):  # [B, 5, 4] @ [2, 7, 4, 4] broadcasts to [2, 7, 5, 4] for B = 7 ... or fails; either way no rule
            return self.fc((self.l(x) @ self.table).mean((0, 2)))

    m = Wide().eval()
    sweep = SeedBatchedSweep(m, _taps(m), kernels=None)
    with pytest.raises(SweepUnsupported, match=r"matmul: the constant table of shape \(2, 7, 4, 4\) must be 2-D or have the leading dims"):
        sweep.forward(torch.randn(7, 5, 4))


def test_tensor_times_number_stays_refused():
    """``* d ** -0.5`` is a product with a Python number: the scale of hand-written attention is served as ``/ math.sqrt(d)`` only"""
    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = nn.Linear(4, 3)

        def forward(self, x):
            return self.fc(x) * 4 ** -0.5

    with pytest.raises(SweepUnsupported, match="mul by the Python number 0.5 is not served"):
        SeedBatchedSweep(M().eval(), {}, kernels=None)
