"""The SPLIT / SLICE rules of both seed-batched reverse sweeps (laplace_amd/sweep.py, laplace_amd/sweep_nhwc.py) on the CPU: models
that chunk, split, narrow or index a tensor go through ONE sweep for all seeds and match one autograd pass per seed; the curvature
quantities built on it match the fp64 oracle; what the rules do not serve is refused by name and the backend answers through the
tape; the kernel branches of both sweeps run on the emulation (tests/emulated_slice_kernels.py).

Before the rules existed every model here was refused whole - "no VJP rule for method chunk" at construction, or "tensor
indexing" in the forward - and took the autograd tape."""
import copy
import operator

import pytest
import torch
import torch.fx as fx
import torch.nn.functional as F
from torch import nn

from laplace_amd import _lib
from laplace_amd._lib import get_kernels, is_channels_last
from laplace_amd.sweep import CONST, IDENTITY, SLICE, SPLIT, Rule, SeedBatchedSweep, SweepUnsupported, classify, slice_range
from laplace_amd.sweep_nhwc import SplitSweep
from tests import slice_fixtures as sf
from tests.norm_sweep_fixtures import autograd_reference


def _taps(model):
    return {n: m for n, m in model.named_modules() if isinstance(m, (nn.Linear, nn.Conv2d))}


# ---- 1. every spelling against autograd ------------------------------------------------------------------------------------------
class Chunk(nn.Module):
    """``Tensor.chunk`` with a ragged last part (5 channels in chunks of 2, 2, 1), every part used"""

    def __init__(self):
        super().__init__()
        self.c0, self.c1, self.c2, self.fc = nn.Conv2d(3, 5, 3, 1, 1), nn.Conv2d(2, 2, 3, 1, 1), nn.Conv2d(5, 4, 1), nn.Linear(4, 3)

    def forward(self, x):
        x = self.c0(x)
        a, b, c = x.chunk(3, 1)
        return self.fc(self.c2(torch.cat([a, self.c1(torch.tanh(b)), c], 1)).mean((2, 3)))


class Sections(nn.Module):
    """``torch.split`` with a list of sections along dim=-3, one part left unused; ``torch.chunk`` and an int split size"""

    def __init__(self):
        super().__init__()
        self.c0, self.c1, self.fc = nn.Conv2d(3, 6, 3, 1, 1), nn.Conv2d(3, 4, 1), nn.Linear(4, 3)

    def forward(self, x):
        x = torch.tanh(self.c0(x))
        a, unused, c = torch.split(x, [1, 2, 3], dim=-3)
        u, v = torch.chunk(c, chunks=2, dim=1)  # (2, 1)
        p, q = x.split(4, 1)  # (4, 2)
        return self.fc(self.c1(torch.cat([a, u], 1) + p[:, 1:] + torch.cat([q, v], 1)).mean((2, 3)))


class Overlap(nn.Module):
    """the same source sliced by overlapping ranges (negative bounds among them) and also consumed whole"""

    def __init__(self):
        super().__init__()
        self.c0, self.c1, self.c2, self.fc = nn.Conv2d(3, 6, 3, 1, 1), nn.Conv2d(6, 4, 1), nn.Conv2d(4, 4, 1), nn.Linear(4, 3)

    def forward(self, x):
        x = self.c0(x)
        y = x[:, 0:4] + x[:, 1:-1] + x[:, -4:] + x.narrow(1, 2, 4) + torch.narrow(x, -3, -5, 4)
        return self.fc((self.c1(x) + self.c2(torch.tanh(y))).mean((2, 3)))


class Tokens(nn.Module):
    """a sequence model: an int index (the class token), ``x[..., -1]``, a frozen token prepended through ``expand`` + ``cat``,
    a packed projection split in three, slice after slice"""

    def __init__(self):
        super().__init__()
        self.embed, self.qkv, self.fc = nn.Linear(3, 6), nn.Linear(6, 18), nn.Linear(6, 3)
        self.cls = nn.Parameter(torch.linspace(-1, 1, 6).reshape(1, 1, 6), requires_grad=False)

    def forward(self, x):
        x = self.embed(x.flatten(2).transpose(1, 2))  # [B, 16, 6]
        x = torch.cat([self.cls.expand(x.size(0), -1, -1), x], 1)
        q, k, v = self.qkv(x).split(6, dim=2)
        h = torch.tanh(q) + k + v  # [B, 17, 6]
        tail = h[:, 2:][:, :-3][..., 1:4, :]  # slice after slice: positions 3, 4, 5
        return self.fc(h[:, 0] + h[:, -1, :] + tail.mean(1) + h.transpose(1, 2)[..., 5] + h[...][:, 1])


class ClassToken(nn.Module):
    """the head of a ViT / BERT classifier: ``x[:, 0]`` of a sequence"""

    def __init__(self):
        super().__init__()
        self.embed, self.fc = nn.Linear(3, 6), nn.Linear(6, 3)

    def forward(self, x):
        return self.fc(torch.tanh(self.embed(x.flatten(2).transpose(1, 2)))[:, 0])


MODELS = {"chunk": Chunk, "sections": Sections, "overlap": Overlap, "tokens": Tokens, "class-token": ClassToken}
# (SPLIT nodes, SLICE nodes)
KINDS = {"chunk": (1, 3), "sections": (3, 8), "overlap": (0, 5), "tokens": (1, 10), "class-token": (0, 1)}


def _build(name):
    torch.manual_seed(5 + len(name))
    return MODELS[name]().double().eval(), torch.randn(5, 3, 4, 4, dtype=torch.float64)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_sweep_matches_one_autograd_pass_per_seed(name):
    """fails without the rules: `chunk` is refused at construction with "no VJP rule for method chunk" (`sections`: "... function
    split", `overlap`: "... method narrow", `tokens`: "... method expand"), and `class-token` - the ``x[:, 0]`` model - in the
    forward with "tensor indexing" """
    m64, X = _build(name)
    taps = _taps(m64)
    sweep = SeedBatchedSweep(m64, taps, kernels=None)
    assert (sum(r.kind == SPLIT for r in sweep.rule.values()), sum(r.kind == SLICE for r in sweep.rule.values())) == KINDS[name]
    f = sweep.forward(X)
    torch.manual_seed(0)
    seeds = torch.randn(4, *f.shape, dtype=torch.float64)
    grads = sweep.backward(seeds)
    f_ref, ins, want = autograd_reference(m64, taps, X, seeds)
    assert torch.equal(f, f_ref.detach())
    for n in taps:
        assert torch.equal(sweep.taps[n]["a"], ins[n]), n
        assert grads[n].shape == want[n].shape, n
        assert (grads[n] - want[n]).abs().max() <= 1e-12 * (1 + want[n].abs().max()), n


def test_the_rules_look_through_the_split_and_resolve_on_the_value():
    m64, X = _build("chunk")
    sweep = SeedBatchedSweep(m64, {}, kernels=None)
    split = next(n for n, r in sweep.rule.items() if r.kind == SPLIT)
    parts = [r for r in sweep.rule.values() if r.kind == SLICE]
    assert sweep.rule[split].args == ("chunk", 3, 1) and sweep.rule[split].fn is torch.Tensor.chunk
    assert all(r.src == sweep.rule[split].src for r in parts)  # (the source is the split's source, not the tuple)
    assert [r.args for r in parts] == [("split", "chunk", 3, 1, i) for i in range(3)]
    sweep.forward(X)
    saved = [sweep.saved[n] for n, r in sweep.rule.items() if r.kind == SLICE]
    assert saved == [(1, 0, 2, False, X.shape[:1] + (5, 4, 4)), (1, 2, 2, False, X.shape[:1] + (5, 4, 4)),
                     (1, 4, 1, False, X.shape[:1] + (5, 4, 4))]  # (dim, start, length, dropped, input shape)
    # chunk / split as torch resolves them: fewer parts than asked, a ragged tail, sections, negative dims and parts
    assert slice_range(("split", "chunk", 4, 1, 2), (2, 6)) == (1, 4, 2, False)  # 6 in 4 chunks: 2, 2, 2
    with pytest.raises(SweepUnsupported, match="part 3 of 3"):
        slice_range(("split", "chunk", 4, 1, 3), (2, 6))
    assert slice_range(("split", "split", 4, -1, -1), (2, 3, 10)) == (2, 8, 2, False)
    assert slice_range(("split", "split", (1, 0, 3), 1, 2), (2, 4)) == (1, 1, 3, False)
    with pytest.raises(SweepUnsupported, match="empty range"):
        slice_range(("split", "split", (1, 0, 3), 1, 1), (2, 4))
    with pytest.raises(SweepUnsupported, match="do not sum"):
        slice_range(("split", "split", (1, 2), 1, 0), (2, 4))
    assert slice_range(("index", (slice(None), -1), 1), (2, 4, 3)) == (1, 3, 1, True)
    assert slice_range(("index", (Ellipsis, slice(-2, None)), 1), (2, 4, 3)) == (2, 1, 2, False)
    assert slice_range(("index", (Ellipsis, 0, slice(None)), 1), (2, 4, 3)) == (1, 0, 1, True)
    assert slice_range(("narrow", -1, -2, 2), (2, 4, 3)) == (2, 1, 2, False)
    with pytest.raises(SweepUnsupported, match="the batch dim"):
        slice_range(("index", (Ellipsis, 0), 1), (4,))
    with pytest.raises(SweepUnsupported, match="out of range"):
        slice_range(("index", (slice(None), 4), 1), (2, 4))
    with pytest.raises(SweepUnsupported, match="leaves dim 1"):
        slice_range(("narrow", 1, 3, 2), (2, 4))


def test_an_expanded_constant_is_a_constant_and_an_expanded_tensor_is_refused():
    m64, X = _build("tokens")
    sweep = SeedBatchedSweep(m64, _taps(m64), kernels=None)
    consts = [r for r in sweep.rule.values() if r.kind == CONST]
    assert [r.args for r in consts] == [("cls",), ()] and consts[1].fn is torch.Tensor.expand and "expand" in consts[1].what
    assert sum(r.kind == IDENTITY for r in sweep.rule.values()) == 1  # (h[...]: a view of everything)

    class Traced(nn.Module):
        def __init__(self, how):
            super().__init__()
            self.how, self.l, self.fc = how, nn.Linear(4, 4), nn.Linear(4, 3)

        def forward(self, x):
            h = self.l(x)
            h = h.expand(2, -1, -1, -1).mean(0) if self.how == "expand" else h.expand_as(x)
            return self.fc(h)

    for how in ("expand", "expand_as"):
        with pytest.raises(SweepUnsupported, match=f"method {how} of a traced tensor"):
            SeedBatchedSweep(Traced(how).eval(), {}, kernels=None)


# ---- 2. curvature against the oracle -------------------------------------------------------------------------------------------------
@pytest.fixture
def emulated():
    from tests.emulated_slice_kernels import EmulatedSliceKernels

    K = EmulatedSliceKernels()
    prev = _lib.set_kernels_for_testing(K)
    yield K
    _lib.set_kernels_for_testing(prev)


def _small_csp():
    return sf.csp_fixture(widths=(64,), depth=1, B=6, hw=4, classes=3, seed=33)


def _small_vit():
    return sf.vit_fixture(dim=8, depth=1, heads=2, B=6, classes=3, seed=34)


def test_curvature_of_a_csp_model_on_the_emulation_matches_the_oracle(emulated):
    """fails without the rules: the model takes the tape ("no VJP rule for method chunk"), which `run_curvature_checks` refuses"""
    got = sf.run_curvature_checks("cpu", _small_csp())
    fwd = [s for s in emulated.seen if s[0] == "slice_forward"]
    vjp = [s for s in emulated.seen if s[0] == "slice_vjp"]
    assert fwd and vjp and all(s[2:] in ((64, 0, 32), (64, 32, 32)) for s in fwd)
    # ONE launch per sliced map: the half that went through the blocks (a split tensor and the fp32 map of the residual add) and the
    # half that went straight to the concatenation, each with a max|.| word
    assert all(s[1] == (("split", 32, 32), ("f32", 32, 32), ("f32", 0, 32)) and s[3] == 64 and s[4] for s in vjp)

    # the NCHW sweep (rule 1 alone, kernels on and off) gives the same numbers
    def nchw(b):
        b.use_split_sweep = False

    ref = sf.run_curvature_checks("cpu", _small_csp(), configure=nchw, want_split=False)
    for k in ("Js", "f", "h", "f_var"):
        assert sf.rel(got[k], ref[k]) < 1e-4, k


def test_curvature_of_a_class_token_model_matches_the_oracle_with_the_kernels_on_and_off(emulated, monkeypatch):
    """fails without the rules: "no VJP rule for method split" (and, behind it, "tensor indexing" for ``x[:, 0]``)"""
    got = sf.run_curvature_checks("cpu", _small_vit(), want_split=False)
    vjp = [s for s in emulated.seen if s[0] == "slice_vjp"]
    # the packed projection: three pieces of dim columns in rows of 3 dim; the class token: the first dim of T dim columns
    assert any(s[1] == (("f32", 16, 8), ("f32", 8, 8), ("f32", 0, 8)) and s[3] == 24 for s in vjp)
    assert any(s[1] == (("f32", 0, 8),) and s[3] == 5 * 8 for s in vjp)
    assert not any(s[0] == "slice_forward" for s in emulated.seen)  # (the NCHW sweep slices by view)
    emulated.seen.clear()
    monkeypatch.setattr(SeedBatchedSweep, "use_slice_kernels", False)
    ref = sf.run_curvature_checks("cpu", _small_vit(), want_split=False)
    assert not any(s[0].startswith("slice") for s in emulated.seen)
    for k in ("Js", "f", "h", "f_var"):
        assert sf.rel(got[k], ref[k]) < 1e-4, k


def test_the_workloads_are_served():
    """a tiny CSPNetSmall reaches ``split_reason is None`` on the emulation; ViTClassToken runs the NCHW walk with one
    weight-sharing factor on its packed projection.  Fails without the rules."""
    from laplace_amd.nets import CSPNetSmall, ViTClassToken
    from tests.emulated_slice_kernels import EmulatedSliceKernels

    K = EmulatedSliceKernels()
    m = CSPNetSmall(widths=(64, 128), depth=1).eval()
    sw = SplitSweep(m, _taps(m), kernels=lambda: K)
    assert sw.split_ok and sw.split_reason is None
    assert sum(r.kind == SPLIT for r in sw.rule.values()) == 2 and sum(r.kind == SLICE for r in sw.rule.values()) == 4
    full = CSPNetSmall()
    assert [s.mix[0].in_channels for s in full.layers if hasattr(s, "mix")] == [64, 128, 256]
    assert all(mod.in_channels % 32 == 0 and mod.out_channels % 32 == 0 for mod in full.modules()
               if isinstance(mod, nn.Conv2d) and mod.in_channels != 3)
    assert not any(p.requires_grad for mod in full.modules() if isinstance(mod, nn.BatchNorm2d) for p in mod.parameters())
    v = ViTClassToken(image=8, patch=4, dim=16, depth=2, heads=2).eval()
    assert not v.cls.requires_grad and v.pos.shape == (1, 5, 16) and v.blocks[0].qkv.out_features == 48
    sw = SplitSweep(v, _taps(v), kernels=lambda: K)
    assert not sw.split_ok and "scaled_dot_product_attention" in sw.split_reason
    x = torch.randn(2, 3, 8, 8)
    assert torch.allclose(sw.forward(x), v(x), rtol=1e-4, atol=1e-6)


# ---- 3. refusals of the rules ----------------------------------------------------------------------------------------------------------
def _node(target, args, kwargs=None, method=False):
    g = fx.Graph()
    x = g.placeholder("x")
    res = lambda a: x if isinstance(a, str) and a == "x" else a  # noqa: E731

    def deep(a):
        if isinstance(a, (list, tuple)):
            return type(a)(deep(v) for v in a)
        if isinstance(a, slice):
            return slice(deep(a.start), deep(a.stop), deep(a.step))
        return res(a)

    args = tuple(deep(a) for a in args)
    kwargs = {k: deep(v) for k, v in (kwargs or {}).items()}
    return (g.call_method(target, args, kwargs) if method else g.call_function(target, args, kwargs)), x


@pytest.mark.parametrize("target,args,kwargs,method,fragment", [
    ("chunk", ("x", 2), None, True, "along dim 0 (the batch dim"),  # (torch's default)
    (torch.chunk, ("x", 2, 0), None, False, "along dim 0 (the batch dim"),
    (torch.split, ("x", [1, 2]), {"dim": 0}, False, "along dim 0 (the batch dim"),
    ("narrow", ("x", 0, 0, 1), None, True, "along dim 0 (the batch dim"),
    (operator.getitem, ("x", 0), None, False, "slices dim 0 (the batch dim"),
    (operator.getitem, ("x", slice(1, 3)), None, False, "slices dim 0 (the batch dim"),
    (operator.getitem, ("x", (slice(None), slice(0, 4, 2))), None, False, "a step other than 1"),
    (operator.getitem, ("x", (slice(None), slice(None, None, -1))), None, False, "a step other than 1"),
    (operator.getitem, ("x", (slice(None), 0, slice(1, 2))), None, False, "index one dim at a time"),
    (operator.getitem, ("x", (slice(None), 0, 0)), None, False, "index one dim at a time"),
    (operator.getitem, ("x", (slice(None), torch.tensor([0, 1]))), None, False, "with a tensor index"),
    (operator.getitem, ("x", (slice(None), [0, 1])), None, False, "with a list index"),
    (operator.getitem, ("x", (slice(None), True)), None, False, "with a bool index"),
    (operator.getitem, ("x", (slice(None), None)), None, False, "with a None index"),
    (operator.getitem, ("x", (slice(None), "x")), None, False, "data-dependent index"),
    (operator.getitem, ("x", (slice(None), slice(0, "x"))), None, False, "data-dependent bounds"),
    (operator.getitem, ("x", (Ellipsis, 0, Ellipsis)), None, False, "more than one '...'"),
    ("split", ("x", "x", 1), None, True, "data-dependent split size"),
    (torch.split, ("x", [1, "x"], 1), None, False, "data-dependent section"),
    ("chunk", ("x", "x", 1), None, True, "data-dependent number of chunks"),
    ("chunk", ("x", 2), {"dim": "x"}, True, "data-dependent dim"),
    (torch.narrow, ("x", "x", 0, 1), None, False, "data-dependent dim"),
    (torch.narrow, ("x", 1, "x", 1), None, False, "data-dependent start"),
    ("narrow", ("x", 1, 0), {"length": "x"}, True, "data-dependent length"),
    (torch.unbind, ("x", 1), None, False, "no VJP rule for function unbind (unbind is out of scope"),
    ("unbind", ("x", 1), None, True, "no VJP rule for method unbind (unbind is out of scope"),
    (torch.tensor_split, ("x", 2, 1), None, False, "tensor_split is out of scope"),
    ("tensor_split", ("x", 2, 1), None, True, "tensor_split is out of scope"),
    (torch.stack, (["x", "x"], 1), None, False, "no VJP rule for function stack (stack is out of scope"),
], ids=lambda v: None)
def test_classify_refuses_by_name(target, args, kwargs, method, fragment):
    node, _ = _node(target, args, kwargs, method)
    with pytest.raises(SweepUnsupported, match=fragment.replace("(", r"\(").replace(".", r"\.")):
        classify(node, {})


def test_classify_accepts_the_spellings_and_keeps_non_tensor_getitem():
    node, x = _node(operator.getitem, ("x", (slice(None), slice(2, -1))))
    r = classify(node, {})
    assert isinstance(r, Rule) and r.kind == SLICE and r.src == (x,) and r.args == ("index", (slice(None), slice(2, -1)), 1)
    assert classify(_node(operator.getitem, ("x", (Ellipsis, -1)))[0], {}).args == ("index", (Ellipsis, -1), 1)
    assert classify(_node(operator.getitem, ("x", (slice(None), slice(0, None))))[0], {}).kind == IDENTITY
    assert classify(_node(torch.narrow, ("x", -1), {"start": -2, "length": 2})[0], {}).args == ("narrow", -1, -2, 2)
    assert classify(_node("split", ("x", (2, 3)), {"dim": 2}, True)[0], {}).args == ("split", (2, 3), 2)
    assert classify(_node(torch.split, ("x",), {"split_size_or_sections": 2, "dim": -1})[0], {}).args == ("split", 2, -1)
    # a getitem of a size() tuple keeps its kind and function
    g = fx.Graph()
    x = g.placeholder("x")
    size = g.call_method("size", (x,))
    r = classify(g.call_function(operator.getitem, (size, 0)), {})
    assert r.kind == "getitem" and r.fn is operator.getitem
    # a part of a split must be taken with a static integer; the tuple itself has no cotangent
    parts = g.call_method("chunk", (x, 2, 1))
    with pytest.raises(SweepUnsupported, match="one by one with a static integer index"):
        classify(g.call_function(operator.getitem, (parts, slice(0, 1))), {})


class _Refused(nn.Module):
    """what the rules refuse inside a model that is served but for that"""

    def __init__(self, how):
        super().__init__()
        self.how = how
        self.c0, self.c1, self.fc = nn.Conv2d(3, 4, 3, 1, 1), nn.Conv2d(2, 4, 1), nn.Linear(4, 3)

    def forward(self, x):
        how, h = self.how, torch.tanh(self.c0(x))
        if how == "step":
            h = h[:, ::2]
        elif how == "two-dims":
            h = h[:, :2, 1:]
        elif how == "none":
            h = h[:, :2, None].mean(2)
        elif how == "unbind":
            h = torch.cat(h.unbind(1)[:2], 1).view(-1, 2, 4, 4)
        elif how == "stack":
            h = torch.stack([h, h], 1)[:, 0, :2]
        elif how == "tensor_split":
            h = h.tensor_split(2, 1)[0]
        elif how == "whole-tuple":
            h = h.chunk(2, 1)[0:1][0]
        elif how == "batch-dim":  # dim -4 of a 4-D value is the batch dim: only the value tells
            h = h.narrow(-4, 0, 3).narrow(1, 0, 2)
        elif how == "ragged-sections":  # sections that do not sum to the dim: torch refuses them, and so does the value
            h = h.split([1, 2], 1)[1]
        else:
            h = h[:, :2]
        return self.fc(self.c1(h).mean((2, 3)))


REFUSALS = {"step": "a step other than 1", "two-dims": "index one dim at a time", "none": "with a None index",
            "unbind": "unbind is out of scope", "stack": "stack is out of scope", "tensor_split": "tensor_split is out of scope",
            "whole-tuple": "its parts must be taken one by one"}


def _tape_answers(model, X, fragment):
    """the backend falls to the tape with the refusal as its reason, and gives the oracle's numbers"""
    from laplace_amd import HipGGN
    from oracle import curvature_oracle as co
    from tests.emulated_slice_kernels import EmulatedSliceKernels

    prev = _lib.set_kernels_for_testing(EmulatedSliceKernels())
    try:
        backend = HipGGN(model, "classification")
        Js, f = backend.jacobians(X)
        assert fragment in backend._tape().sweep_reason
        y = torch.arange(X.shape[0]) % 3
        _, h = backend.diag(X, y)
    finally:
        _lib.set_kernels_for_testing(prev)
    m64 = copy.deepcopy(model).double()
    Js64, f64 = co.jacobians(m64, X.double())
    assert sf.rel(f, f64) < 1e-5 and sf.rel(Js, Js64) < 1e-4
    assert sf.rel(h, co.ggn_diag(Js64, co.functional_hessian(f64, "classification"))) < 1e-4


@pytest.mark.parametrize("how", sorted(REFUSALS))
def test_what_is_not_served_is_refused_at_construction_and_the_tape_answers(how):
    torch.manual_seed(1)
    model, X = _Refused(how).eval(), torch.randn(3, 3, 4, 4)
    with pytest.raises(SweepUnsupported, match=REFUSALS[how]):
        SeedBatchedSweep(model, _taps(model), kernels=None)
    _tape_answers(model, X, REFUSALS[how])


def test_what_only_the_value_tells_is_refused_in_the_forward_and_the_tape_answers():
    torch.manual_seed(1)
    X = torch.randn(3, 3, 4, 4)
    model = _Refused("batch-dim").eval()
    sweep = SeedBatchedSweep(model, _taps(model), kernels=None)  # (-4 is a static dim: `classify` lets it through)
    with pytest.raises(SweepUnsupported, match=r"narrow along dim -4 of a value with 4 dims \(the batch dim"):
        sweep.forward(X)
    _tape_answers(model, X, "the batch dim")
    served = _Refused("plain").eval()
    sweep = SeedBatchedSweep(served, _taps(served), kernels=None)
    assert torch.allclose(sweep.forward(X), served(X))


def test_sections_that_do_not_sum_to_the_dim_are_refused_on_the_value():
    model = _Refused("ragged-sections").eval()
    sweep = SeedBatchedSweep(model, _taps(model), kernels=None)
    with pytest.raises(SweepUnsupported, match="method split: split_with_sizes expects split_sizes to sum exactly to 4"):
        sweep.forward(torch.randn(2, 3, 4, 4))


def test_pinned_refusals_next_to_the_rules_stay():
    """`tensor * 2.0` stays "mul"; a batch-moving permute stays; the cross-attention model of tests/test_sweep_attn.py now gets past its
    ``q[:, :, :2]`` and is refused by the attention rule's own "Tq == Tk" """
    from tests.test_sweep_attn import _Attn

    class Mul(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = nn.Linear(4, 3)

        def forward(self, x):
            return self.fc(x[:, :4] * 2.0)

    with pytest.raises(SweepUnsupported, match="mul"):
        SeedBatchedSweep(Mul().eval(), {}, kernels=None)
    model = _Attn("cross").eval()
    sweep = SeedBatchedSweep(model, {n: m for n, m in model.named_modules() if isinstance(m, nn.Linear)}, kernels=None)
    assert sum(r.kind == SLICE for r in sweep.rule.values()) == 1
    with pytest.raises(SweepUnsupported, match="Tq == Tk"):
        sweep.forward(torch.randn(3, 4, 8))
    with pytest.raises(SweepUnsupported, match="moves the batch dim"):
        SeedBatchedSweep(_Attn("batch-permute").eval(), {}, kernels=None).forward(torch.randn(3, 4, 8))

    class Pool(nn.Module):
        def forward(self, x):
            return F.max_pool2d(x, 2, return_indices=True)[0].flatten(1)

    with pytest.raises(SweepUnsupported, match="max_pool2d"):
        SeedBatchedSweep(Pool().eval(), {}, kernels=None)


# ---- 4. the NHWC route: refusals and the kernel branch -----------------------------------------------------------------------------------
class _Map(nn.Module):
    """slices of feature maps the split sweep serves (``plain``) or leaves to the NCHW sweep"""

    def __init__(self, how):
        super().__init__()
        self.how = how
        cin = {"height": 64, "int": 32, "mixed": 32}.get(how, 32)
        self.c0, self.c1, self.fc = nn.Conv2d(3, 64, 3, 1, 1), nn.Conv2d(cin, 32, 3, 1, 1), nn.Linear(32, 3)
        if how == "mixed":
            self.l = nn.Linear(32 * 16, 32)

    def forward(self, x):
        how, a = self.how, torch.tanh(self.c0(x))
        if how == "height":
            h = self.c1(a[:, :, 1:3])
        elif how == "int":
            h = self.c1(a[:, :, 0].view(-1, 32, 2, 4))
        elif how == "mixed":
            b = a[:, 32:]
            return self.fc(torch.flatten(F.adaptive_avg_pool2d(self.c1(b), 1), 1) + self.l(b.flatten(1)))
        else:
            h = self.c1(a.narrow(1, 32, 32)) + a[:, :32]
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(h, 1), 1))


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


def test_eligibility_refusals_name_their_node_and_keep_the_nchw_route(emulated, monkeypatch):
    torch.manual_seed(2)
    assert _nchw_route(_Map("height").eval(), get_kernels) == \
        "getitem: indexing of tanh: slice of a feature map along dim 2 (H or W; the NHWC kernels slice channels: dim 1 of a 4-D map)"
    assert _nchw_route(_Map("int").eval(), get_kernels) == \
        "getitem: indexing of tanh: an int index on a feature map (the NHWC kernels slice channel ranges and keep the dim)"
    assert _nchw_route(_Map("mixed").eval(), get_kernels) == \
        "getitem: indexing of tanh: slice of a feature map mixed with consumers outside the feature maps"
    plain = _Map("plain").eval()
    assert SplitSweep(plain, _taps(plain), kernels=get_kernels).split_ok
    monkeypatch.setattr(SplitSweep, "nhwc_slice", False)
    assert _nchw_route(plain, get_kernels) == "narrow: method narrow has no NHWC rule"


@pytest.mark.parametrize("missing", ("slice_forward", "slice_vjp"))
def test_split_sweep_wants_both_entry_points(missing, emulated):
    def absent(self):
        raise AttributeError(missing)

    K = type("OneEntryPoint", (type(emulated),), {missing: property(absent)})()
    assert not hasattr(K, missing)
    assert _nchw_route(_Map("plain").eval(), lambda: K) == "narrow: kernels without the slicing entry points"


def test_the_concatenation_emulation_keeps_a_slicing_model_on_the_nchw_route_and_on_the_torch_sequence():
    from tests.emulated_cat_kernels import EmulatedCatKernels

    K = EmulatedCatKernels()
    assert "kernels without the slicing entry points" in _nchw_route(_Map("plain").eval(), lambda: K)


def test_the_kernel_branch_of_the_split_sweep_matches_float64_autograd(emulated):
    torch.manual_seed(7)
    m64 = _Map("plain").double().eval()
    model = copy.deepcopy(m64).float()
    taps = _taps(model)
    sw = SplitSweep(model, taps, kernels=get_kernels)
    assert sw.split_ok, sw.split_reason
    outs = {}
    inner = sw._run_slice
    sw._run_slice = lambda node, r, inp, *a, _i=inner: outs.setdefault(node, _i(node, r, inp, *a))
    X = torch.randn(3, 3, 4, 4, dtype=torch.float64)
    seeds = torch.randn(2, 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    f = sw.forward(X.float())
    grads = sw.backward(seeds.float())
    # layouts: NHWC memory in (a view, no copy), a contiguous NHWC map out, returned as the NCHW-logical view
    assert len(outs) == 2 and all(is_channels_last(o) and o.shape[1] == 32 for o in outs.values())
    assert [s for s in emulated.seen if s[0] == "slice_forward"] == [("slice_forward", 48, 64, 32, 32), ("slice_forward", 48, 64, 0, 32)]
    # ONE launch for the sliced map: the convolution's cotangent of channels [32, 64) as it lies and the fp32 map of [0, 32)
    vjp = [s for s in emulated.seen if s[0] == "slice_vjp"]
    assert len(vjp) == 1 and vjp[0][2:] == (2 * 48, 64, True)
    assert vjp[0][1] == (("f32", 0, 32), ("f32", 32, 32))
    f64, ins, want = autograd_reference(m64, _taps(m64), X, seeds)
    assert sf.rel(f, f64) < 1e-5
    for n in taps:
        assert sf.rel(sw.taps[n]["a"], ins[n]) < 1e-5, n
        assert grads[n].shape == want[n].shape and sf.rel(grads[n], want[n]) < 1e-4, (n, sf.rel(grads[n], want[n]))


def test_a_head_slice_takes_the_parent_math_on_the_split_sweep(emulated, monkeypatch):
    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.c0, self.l1, self.fc = nn.Conv2d(3, 32, 3, 1, 1), nn.Linear(16, 4), nn.Linear(20, 3)

        def forward(self, x):
            h = torch.flatten(F.adaptive_avg_pool2d(torch.relu(self.c0(x)), 1), 1)
            a, b = h.chunk(2, 1)
            return self.fc(torch.cat([a, torch.tanh(self.l1(b))], -1))

    monkeypatch.setattr(SeedBatchedSweep, "use_slice_kernels", False)
    torch.manual_seed(5)
    m64 = M().double().eval()
    model = copy.deepcopy(m64).float()
    taps = _taps(model)
    sw = SplitSweep(model, taps, kernels=get_kernels)
    assert sw.split_ok, sw.split_reason
    X, seeds = torch.randn(3, 3, 4, 4, dtype=torch.float64), torch.randn(2, 3, 3, dtype=torch.float64)
    f = sw.forward(X.float())
    grads = sw.backward(seeds.float())
    assert not [s for s in emulated.seen if s[0].startswith("slice")]  # (no kernel of lk_slice.hip: plain tensors, the torch sequence)
    f64, _, want = autograd_reference(m64, _taps(m64), X, seeds)
    assert sf.rel(f, f64) < 1e-5
    for n in taps:
        assert sf.rel(grads[n], want[n]) < 1e-4, n


def test_more_than_eight_pieces_take_a_further_launch(emulated):
    gen = torch.Generator().manual_seed(3)
    full = torch.randn(6, 8, generator=gen)
    halves = [torch.randn(6, 4, generator=gen) for _ in range(10)]
    pieces = [(full, 0, 8)] + [(h, 4 * (i % 2), 4) for i, h in enumerate(halves)]
    word = torch.zeros(1)
    got = SeedBatchedSweep.slice_vjp_launches(emulated, pieces, 6, 8, amax=word)
    assert torch.equal(got, sf.vjp_reference(pieces, 6, 8)) and float(word) == float(got.abs().max())
    seen = [s for s in emulated.seen if s[0] == "slice_vjp"]
    assert [len(s[1]) for s in seen] == [8, 4] and [s[4] for s in seen] == [False, True]  # (the word goes to the last launch)
    assert seen[1][1][0] == ("f32", 0, 8)


def test_an_inference_only_forward_keeps_nothing(emulated):
    m64, X, _ = _small_csp()
    model = copy.deepcopy(m64).float()
    sw = SplitSweep(model, sf.taps(model), kernels=get_kernels)
    f = sw.forward(X.float(), need_vjp=False)
    assert sw.saved == {} and sf.rel(f, m64(X).detach()) < 1e-5
