"""nn.MultiheadAttention and the stock transformer encoder in the seed-batched reverse sweep and on the autograd tape, on the CPU:
the module is served as the two nn.Linear layers around its attention core (`laplace_amd.mha.lift`), both 'linear' taps with the
real parameters' offsets; the curvature quantities match the fp64 oracle RUN ON THE TWIN (tests/mha_fixtures.py); every switch
and the hook route give the same values; what is not served is refused by name and the generic route still answers."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from laplace_amd import mha
from laplace_amd.capture import EXTRA_KINDS, Tape
from laplace_amd.sweep import SeedBatchedSweep, SweepUnsupported
from tests import mha_fixtures as mf
from tests.attn_fixtures import rel


@pytest.fixture
def emulated():
    from laplace_amd import _lib
    from tests.emulated_mha_kernels import EmulatedMhaKernels

    K = EmulatedMhaKernels()
    prev = _lib.set_kernels_for_testing(K)
    try:
        yield K
    finally:
        _lib.set_kernels_for_testing(prev)


# ---- the fixtures themselves --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mf.MODELS)
def test_the_twin_is_the_same_function(name):
    """same outputs to 1e-12 in fp64, the same parameter vector in the same order, and the same Jacobian"""
    from oracle import curvature_oracle as co

    model, twin, X = mf.make_model(name)
    m64, X = model.double(), X.double()
    with torch.no_grad():
        assert (m64(X) - twin(X)).abs().max().item() < 1e-12
    pm, pt = co.trainable_params(m64), co.trainable_params(twin)
    assert [tuple(p.shape) for p in pm] == [tuple(p.shape) for p in pt] and all(torch.equal(a, b) for a, b in zip(pm, pt))
    assert rel(co.jacobians(m64, X)[0], co.jacobians(twin, X)[0]) < 1e-12


def test_lift_holds_the_modules_own_parameters():
    m = nn.MultiheadAttention(8, 2, batch_first=True)
    a, b = mha.lift(m)
    assert a.weight is m.in_proj_weight and a.bias is m.in_proj_bias and b.weight is m.out_proj.weight and b.bias is m.out_proj.bias
    assert (a.in_features, a.out_features, b.in_features, b.out_features) == (8, 24, 8, 8)
    with torch.no_grad():
        m.in_proj_weight.mul_(2.0)
    assert a.weight._version == m.in_proj_weight._version and a.weight.data_ptr() == m.in_proj_weight.data_ptr()
    assert mha.lift(m)[0] is a and mha.lift(m)[1] is b  # (cached per module)
    m.in_proj_weight = nn.Parameter(torch.zeros(24, 8))  # (replaced: the views follow)
    assert mha.lift(m)[0] is not a and mha.lift(m)[0].weight is m.in_proj_weight
    x = torch.randn(3, 5, 8, dtype=torch.float64)
    m64 = nn.MultiheadAttention(8, 2, batch_first=True).double().eval()
    with torch.no_grad():
        m64.in_proj_bias.normal_(), m64.out_proj.bias.normal_()
        assert (mha.decomposed(m64, x)[0] - m64(x, x, x, need_weights=False)[0]).abs().max().item() < 1e-14
    import gc
    import weakref

    ref = weakref.ref(m64)
    mha.lift(m64)
    del m64
    gc.collect()
    assert ref() is None  # (the cache does not keep the module alive)


@pytest.mark.parametrize("name", mf.MODELS)
def test_the_tap_list(name):
    """names and order, offsets equal to the real parameters' offsets, nothing uncovered, and no new tap kind"""
    model, _, _ = mf.make_model(name)
    params = [p for p in model.parameters() if p.requires_grad]
    tape = Tape(model, params)
    assert [t.name for t in tape.taps] == mf.tap_names(name) and all(t.kind == "linear" for t in tape.taps)
    assert tape.uncovered == [] and EXTRA_KINDS == ("gconv", "norm", "embed", "param")
    off, offsets = 0, {}
    for p in params:
        offsets[id(p)] = off
        off += p.numel()
    mods = dict(model.named_modules())
    for t in tape.taps:
        if t.owner is None:
            assert t.module is mods[t.name]
            continue
        owner = mods[t.name.rsplit(".", 1)[0]]
        assert t.owner is owner and isinstance(owner, nn.MultiheadAttention)
        w, b = (owner.in_proj_weight, owner.in_proj_bias) if t.name.endswith("in_proj") else (owner.out_proj.weight, owner.out_proj.bias)
        assert t.module.weight is w and t.module.bias is b and (t.w_off, t.b_off) == (offsets[id(w)], offsets[id(b)])
    assert not any(t.module is m.out_proj for t in tape.taps for m in model.modules() if isinstance(m, nn.MultiheadAttention))


# ---- the sweep against one autograd pass per seed -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mf.MODELS)
def test_sweep_matches_autograd_on_the_twin(name):
    """fp64, torch math: the inputs and the output cotangents of every tap against autograd hooks on the twin's Linear layers"""
    from tests.norm_sweep_fixtures import autograd_reference

    model, twin, X = mf.make_model(name)
    m64, X = model.double(), X.double()
    tape = Tape(m64, [p for p in m64.parameters() if p.requires_grad])
    sweep = SeedBatchedSweep(m64, {t.name: t.module for t in tape.taps}, kernels=None)
    f = sweep.forward(X)
    torch.manual_seed(0)
    seeds = torch.randn(4, *f.shape, dtype=torch.float64)
    grads = sweep.backward(seeds)
    ttaps = {n: m for n, m in twin.named_modules() if isinstance(m, nn.Linear)}
    f_ref, ins, want = autograd_reference(twin, ttaps, X, seeds)
    assert rel(f, f_ref) < 1e-12 and len(ttaps) == len(tape.taps)
    for t, n in zip(tape.taps, ttaps):  # (the twin declares its layers in the model's order)
        assert rel(sweep.taps[t.name]["a"], ins[n]) < 1e-10, t.name
        assert rel(grads[t.name], want[n]) < 1e-10, t.name
    E, T = mf.E, mf.T
    assert grads[tape.taps[1].name].shape == (4, mf.B, T, 3 * E) and sweep.max_act_numel >= 3 * E * T


# ---- curvature on the emulation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lik", ["classification", "regression"])
@pytest.mark.parametrize("name", mf.MODELS)
def test_curvature_on_the_emulation_matches_the_oracle_on_the_twin(emulated, name, lik):
    mf.run_curvature_checks("cpu", name, lik)
    calls = {s[0] for s in emulated.seen}
    assert calls == {"forward_strided", "vjp_strided"}, calls  # (the strided entry points, and nothing else)
    E = mf.E
    for s in emulated.seen:  # the operands are the slices of ONE packed projection, the cotangents of ONE packed buffer
        if s[0] == "forward_strided":
            q, k, v = s[2]
            assert s[1] == 3 * E and (k - q, v - k) == (4 * E, 4 * E)
        else:
            dq, dk, dv = s[3][5:]
            assert (s[1], s[2]) == (3 * E, 3 * E) and (dk - dq, dv - dk) == (4 * E, 4 * E)


def _switch(**attrs):
    def configure(b):
        for k, v in attrs.items():
            setattr(b, k, v)
    return configure


@pytest.mark.parametrize("name", mf.MODELS)
def test_every_switch_and_the_hook_route_give_the_same_values(emulated, name):
    base = mf.run_curvature_checks("cpu", name, "classification")
    for attrs, calls in ((dict(use_strided_attn=False), {"forward", "vjp"}), (dict(use_attn_kernels=False), set()),
                         (dict(use_sweep=False), set())):
        del emulated.seen[:]
        got = mf.run_curvature_checks("cpu", name, "classification", _switch(**attrs), expect_sweep=attrs.get("use_sweep", True))
        assert {s[0] for s in emulated.seen} == calls, (attrs, {s[0] for s in emulated.seen})
        if calls:  # (contiguous copies in layout 1, not the slices)
            assert all(s[1] == 1 for s in emulated.seen)
        for key, want in base.items():
            pairs = zip(got[key], want) if key == "kfacs" else [(got[key], want)]
            for a, w in pairs:
                assert rel(a, w) < 2e-5, (attrs, key)


def test_hipggn_kron_on_a_tracked_multihead_attention(emulated):
    """before the module was lifted its ``out_proj`` was tapped as an nn.Linear that never runs: ``RuntimeError: attn.out_proj:
    module did not run in the forward pass``"""
    from laplace_amd import HipGGN
    from oracle import curvature_oracle as co

    model, twin, X = mf.make_model("mha")
    torch.manual_seed(11)
    y = torch.randint(3, (mf.B,))
    for use_sweep in (True, False):
        backend = HipGGN(model, "classification")
        backend.use_sweep = use_sweep
        loss, kron = backend.kron(X, y, N=mf.B)
        loss64, want = co.kfac_ggn(twin, X.double(), y, mf.B, "classification")
        assert abs(loss.item() - loss64.item()) < 1e-5 * abs(loss64.item()) and len(kron.kfacs) == len(want) == 8
        for F_, G_ in zip(kron.kfacs, want):
            for a, w in zip(F_, G_):
                assert rel(a, w) < 1e-4


def test_the_replaced_output_equals_the_modules_own(emulated):
    """the autograd-tape route returns the decomposition's value as the module's output: exact in fp64, rel < 1e-6 in fp32"""
    for dtype, bar in ((torch.float64, 1e-14), (torch.float32, 1e-6)):
        model, _, X = mf.make_model("mha", need_weights=True)
        model, X = model.to(dtype), X.to(dtype)
        with torch.no_grad():
            want = model(X)
        tape = Tape(model, [p for p in model.parameters() if p.requires_grad])
        f = tape.forward(X)
        assert rel(f, want) < bar
        assert all(t.a is not None and t.out is not None for t in tape.taps)
        assert tape.taps[1].a.shape == (mf.B, mf.T, mf.E) and tape.taps[2].a.shape == (mf.B, mf.T, mf.E)


def test_a_module_applied_twice_raises_the_existing_message():
    class Twice(mf.MhaBlock):
        def forward(self, x):
            x = self.embed(x)
            x = x + self.attn(x, x, x, need_weights=False)[0]
            return self.head((x + self.attn(x, x, x, need_weights=False)[0]).mean(1))

    torch.manual_seed(0)
    model = Twice().eval()
    tape = Tape(model, list(model.parameters()))
    with pytest.raises(NotImplementedError, match="attn: module is applied more than once per forward"):
        tape.forward(torch.randn(2, 6, 5))
    with pytest.raises(SweepUnsupported, match="attn.in_proj: module is applied more than once per forward"):
        SeedBatchedSweep(model, {t.name: t.module for t in tape.taps}).forward(torch.randn(2, 6, 5))


def test_a_head_dim_that_is_no_multiple_of_4_falls_to_the_torch_math(emulated):
    from laplace_amd import HipGGN
    from oracle import curvature_oracle as co

    class Odd(nn.Module):
        def __init__(self):
            super().__init__()
            self.attn = nn.MultiheadAttention(6, 2, batch_first=True)  # (head dim 3)
            self.head = nn.Linear(6, 3)

        def forward(self, x):
            return self.head(self.attn(x, x, x)[0].mean(1))

    torch.manual_seed(2)
    model, X = Odd().eval(), torch.randn(4, 5, 6)
    backend = HipGGN(model, "classification")
    Js, f = backend.jacobians(X)
    import copy

    Js64, f64 = co.jacobians(copy.deepcopy(model).double(), X.double())
    assert rel(f, f64) < 1e-5 and rel(Js, Js64) < 1e-4
    tape = backend._tape()
    assert tape.sweep_reason is None if hasattr(tape, "sweep_reason") else True
    assert emulated.seen == [] and tape.sweeps[frozenset()] is not False and tape.uncovered == []


def test_split_reason_names_the_module(emulated):
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep_nhwc import SplitSweep

    for name, target in (("mha", "attn"), ("pre-norm", "layer.self_attn"), ("encoder", "encoder.layers.0.self_attn")):
        model, _, X = mf.make_model(name)
        tape = Tape(model, [p for p in model.parameters() if p.requires_grad])
        s = SplitSweep(model, {t.name: t.module for t in tape.taps}, kernels=get_kernels)
        assert not s.split_ok and s.split_reason == f"{target}: MultiheadAttention has no NHWC rule"
        f = s.forward(X)  # (the model runs the NCHW walk)
        assert set(s.backward(torch.randn(2, *f.shape))) == set(mf.tap_names(name))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
MODULE_REFUSALS = {
    "kdim": (dict(kdim=4, vdim=4), "kdim / vdim"),
    "bias_kv": (dict(add_bias_kv=True), "bias_k / bias_v"),
    "zero_attn": (dict(add_zero_attn=True), "add_zero_attn"),
    "seq_first": (dict(batch_first=False), "batch_first=False"),
    "dropout": (dict(dropout=0.1), "dropout > 0 in training mode"),
}


@pytest.mark.parametrize("how", sorted(MODULE_REFUSALS))
def test_module_refusals_by_name(how):
    """the module is not lifted, its four parameters stay uncovered and its ``out_proj`` is not tapped as a module that never runs"""
    kw, fragment = MODULE_REFUSALS[how]
    m = nn.MultiheadAttention(8, 2, **{"batch_first": True, **kw})
    m.train(how == "dropout")
    assert fragment in mha.refusal(m)
    with pytest.raises(NotImplementedError, match=fragment):
        mha.lift(m)
    holder = nn.Sequential()
    holder.add_module("attn", m)
    holder.add_module("head", nn.Linear(8, 3))
    tape = Tape(holder, list(holder.parameters()))
    assert [t.name for t in tape.taps] == ["head"] and fragment in tape.mha_refused["attn"]
    assert {id(p) for p in tape.uncovered} == {id(p) for p in m.parameters()}
    if how == "dropout":
        m.eval()
        assert mha.refusal(m) is None


class _Call(nn.Module):
    """a tracked nn.MultiheadAttention called in one of the ways that are not served"""

    def __init__(self, how):
        super().__init__()
        self.how = how
        self.embed = nn.Linear(5, 8)
        if how in ("cross", "key-is-not-value"):
            self.other = nn.Linear(5, 8)
        self.attn = nn.MultiheadAttention(8, 2, batch_first=True)
        self.head = nn.Linear(8, 3)
        self.register_buffer("mask", torch.zeros(6, 6).masked_fill(torch.ones(6, 6).triu(1).bool(), float("-inf")))
        self.register_buffer("pad", torch.zeros(9, 6, dtype=torch.bool))
        self.pad[:, -1] = True

    def forward(self, x):
        h, how = self.embed(x), self.how
        if how == "cross":
            o = self.other(x)
            a = self.attn(h, o, o, need_weights=False)[0]
        elif how == "key-is-not-value":
            a = self.attn(h, h, self.other(x), need_weights=False)[0]
        elif how == "attn_mask":
            a = self.attn(h, h, h, attn_mask=self.mask, need_weights=False)[0]
        elif how == "key_padding_mask":
            a = self.attn(h, h, h, key_padding_mask=self.pad, need_weights=False)[0]
        elif how == "is_causal":
            a = self.attn(h, h, h, attn_mask=self.mask, is_causal=True, need_weights=False)[0]
        else:  # the attention weights are consumed
            a, w = self.attn(h, h, h)
            a = a + w @ h
        return self.head((h + a).mean(1))


CALL_REFUSALS = {"cross": "cross-attention", "key-is-not-value": "cross-attention", "attn_mask": "attn_mask",
                 "key_padding_mask": "key_padding_mask", "is_causal": "attn_mask", "weights": "attention weights are consumed"}


@pytest.mark.parametrize("how", sorted(CALL_REFUSALS))
def test_call_refusals_by_name_and_the_generic_route_still_answers(emulated, how):
    """the sweep names the argument; the tape meets the call, drops the module's taps (its parameters are uncovered from then on)
    and the backend answers through the route it had before - inside the bars of the curvature checks"""
    import copy

    from laplace_amd import HipGGN
    from oracle import curvature_oracle as co

    torch.manual_seed(4)
    model, X = _Call(how).eval(), torch.randn(9, 6, 5)
    tape = Tape(model, list(model.parameters()))
    rest = ["embed"] + ["other"] * hasattr(model, "other")
    assert [t.name for t in tape.taps] == rest + ["attn.in_proj", "attn.out_proj", "head"]
    with pytest.raises(SweepUnsupported, match="attn: nn.MultiheadAttention.*" + CALL_REFUSALS[how]):
        SeedBatchedSweep(model, {t.name: t.module for t in tape.taps})
    backend = HipGGN(model, "classification")
    Js64, f64 = co.jacobians(copy.deepcopy(model).double(), X.double())
    if how == "weights":  # (the tape cannot see a consumer before the reverse pass: it names it there)
        with pytest.raises(NotImplementedError, match="attn: nn.MultiheadAttention whose attention weights are consumed"):
            backend.jacobians(X)
        return
    Js, f = backend.jacobians(X)
    assert rel(f, f64) < 1e-5 and rel(Js, Js64) < 1e-4
    tape = backend._tape()
    assert [t.name for t in tape.taps] == rest + ["head"] and CALL_REFUSALS[how] in tape.mha_refused["attn"]
    assert {id(p) for p in tape.uncovered} == {id(p) for p in model.attn.parameters()}
    torch.manual_seed(11)
    y = torch.randint(3, (9,))
    _, Hf = backend.full(X, y)
    assert rel(Hf, co.ggn_full(Js64, co.functional_hessian(f64, "classification"))) < 1e-4
    with pytest.raises(NotImplementedError, match="KFAC supports nn.Linear / nn.Conv2d parameters only"):
        backend.kron(X, y, N=9)


class _Enc(nn.Module):
    """a stock encoder (layer) called or built in one of the ways that the rewrite refuses"""

    def __init__(self, how):
        super().__init__()
        self.how = how
        self.embed = nn.Linear(5, 8)
        act = {"activation": F.silu, "activation-module": nn.GELU()}.get(how, "relu")
        layer = nn.TransformerEncoderLayer(8, 2, 16, 0.0, act, batch_first=how != "seq_first")
        self.layer = nn.TransformerEncoder(layer, 1, enable_nested_tensor=False) if how.startswith("encoder") else layer
        self.head = nn.Linear(8, 3)
        self.register_buffer("mask", torch.zeros(6, 6).masked_fill(torch.ones(6, 6).triu(1).bool(), float("-inf")))
        self.register_buffer("pad", torch.zeros(9, 6, dtype=torch.bool))
        self.pad[:, -1] = True
        for m in self.modules():  # (KFAC refuses tracked LayerNorm affines: frozen, as in the fixtures)
            if isinstance(m, nn.LayerNorm):
                m.weight.requires_grad_(False), m.bias.requires_grad_(False)

    def forward(self, x):
        h, how = self.embed(x), self.how
        if how == "src_mask":
            h = self.layer(h, src_mask=self.mask)
        elif how == "encoder-mask":
            h = self.layer(h, mask=self.mask)
        elif how in ("src_key_padding_mask", "encoder-src_key_padding_mask"):
            h = self.layer(h, src_key_padding_mask=self.pad)
        elif how == "is_causal":
            h = self.layer(h, src_mask=self.mask, is_causal=True)
        elif how == "seq_first":
            h = self.layer(h.transpose(0, 1)).transpose(0, 1)
        else:
            h = self.layer(h)
        return self.head(h.mean(1))


ENCODER_REFUSALS = {"src_mask": "src_mask", "src_key_padding_mask": "src_key_padding_mask", "is_causal": "src_mask",
                    "encoder-mask": "with mask", "encoder-src_key_padding_mask": "src_key_padding_mask",
                    "activation": "activation silu", "activation-module": "activation GELU", "seq_first": "batch_first=False"}


@pytest.mark.parametrize("how", sorted(ENCODER_REFUSALS))
def test_encoder_refusals_by_name_and_the_tape_still_answers(emulated, how):
    import copy

    from laplace_amd import HipGGN
    from oracle import curvature_oracle as co

    torch.manual_seed(4)
    model, X = _Enc(how).eval(), torch.randn(9, 6, 5)
    tape = Tape(model, [p for p in model.parameters() if p.requires_grad])
    with pytest.raises(SweepUnsupported, match="nn.TransformerEncoder.*" + ENCODER_REFUSALS[how]):
        SeedBatchedSweep(model, {t.name: t.module for t in tape.taps})
    backend = HipGGN(model, "classification")
    Js64, f64 = co.jacobians(copy.deepcopy(model).double(), X.double())
    Js, f = backend.jacobians(X)
    assert rel(f, f64) < 1e-5 and rel(Js, Js64) < 1e-4
    tape = backend._tape()
    if how == "seq_first":  # (the module itself is refused: never lifted, its parameters take the generic route without a sweep)
        assert "batch_first=False" in tape.mha_refused["layer.self_attn"]
        assert {id(p) for p in tape.uncovered} == {id(p) for p in model.layer.self_attn.parameters()}
        return
    assert ENCODER_REFUSALS[how] in tape.sweep_reason
    served = how.startswith("activation")  # (another activation: the layer's own forward calls its sub-modules, the tape serves it)
    assert any(t.owner is not None for t in tape.taps) == served


def test_an_encoder_activation_given_as_a_function_is_served(emulated):
    """``F.relu`` / ``F.gelu`` as callables are what the strings resolve to"""
    torch.manual_seed(0)
    for act in (F.relu, F.gelu):
        model = nn.Sequential(nn.TransformerEncoderLayer(8, 2, 16, 0.0, act, batch_first=True, norm_first=True)).eval()
        tape = Tape(model, [p for p in model.parameters() if p.dim() > 1])
        sweep = SeedBatchedSweep(model, {t.name: t.module for t in tape.taps})
        X = torch.randn(2, 6, 8)
        with torch.no_grad():
            assert rel(sweep.forward(X), model(X)) < 1e-5


def test_vitstock_is_swept_with_every_linear_tapped(emulated):
    """`nets.ViTStock` at small sizes: the stock encoder is rewritten into its sub-modules, each layer's attention is two 'linear'
    taps, nothing is uncovered and the KFAC factors are the twin-free oracle's blocks in number (4 Linear layers per block)"""
    from laplace_amd import HipGGN
    from laplace_amd.nets import ViTStock

    torch.manual_seed(0)
    model = ViTStock(num_classes=3, image=8, patch=4, dim=16, depth=2, heads=2).eval()
    X, y = torch.randn(5, 3, 8, 8), torch.randint(3, (5,))
    backend = HipGGN(model, "classification")
    _, kron = backend.kron(X, y, N=5)
    tape = backend._tape()
    assert tape.sweep_reason is None if hasattr(tape, "sweep_reason") else True
    assert tape.sweeps[frozenset()] not in (None, False) and tape.uncovered == []
    assert len(tape.taps) == 2 + 4 * 2 and len(kron.kfacs) == 2 * len(tape.taps)
    slow = HipGGN(model, "classification")
    slow.use_sweep = False
    for F_, G_ in zip(kron.kfacs, slow.kron(X, y, N=5)[1].kfacs):
        for a, w in zip(F_, G_):
            assert rel(a, w) < 1e-4
