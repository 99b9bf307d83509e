"""The ATTN / PERMUTE / CONST rules of the seed-batched reverse sweep (laplace_amd/sweep.py) on the CPU: a pre-LN transformer
block goes through ONE sweep for all seeds and matches one autograd pass per seed; the curvature quantities built on it match the
fp64 oracle; what the rules do not serve is refused by name and the backend answers through the tape."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from laplace_amd.sweep import ATTN, CONST, PERMUTE, SeedBatchedSweep, SweepUnsupported, attn_forward_math, attn_vjp_math
from tests import attn_fixtures as af
from tests.norm_sweep_fixtures import autograd_reference


def _taps(model):
    return {n: m for n, m in model.named_modules() if isinstance(m, (nn.Linear, nn.Conv2d))}


@pytest.mark.parametrize("name", af.MODELS)
def test_sweep_matches_one_autograd_pass_per_seed(name):
    _, m64, X = af.make_model(name)
    X = X.double()
    taps = _taps(m64)
    sweep = SeedBatchedSweep(m64, taps, kernels=None)
    kinds = {r.kind for r in sweep.rule.values()}
    assert {ATTN, PERMUTE} <= kinds and (CONST in kinds) == name.startswith("attnseq")
    f = sweep.forward(X)
    torch.manual_seed(0)
    seeds = torch.randn(4, *f.shape, dtype=torch.float64)
    grads = sweep.backward(seeds)
    f_ref, ins, want = autograd_reference(m64, taps, X, seeds)
    assert af.rel(f, f_ref) < 1e-12
    for n in taps:
        assert af.rel(sweep.taps[n]["a"], ins[n]) < 1e-10, n
        assert af.rel(grads[n], want[n]) < 1e-10, n
    H, T = 2, 4
    assert sweep.max_act_numel >= H * T * T  # (the [B, H, T, T] probabilities of the torch math count as an activation)


def test_vjp_math_is_chunked_over_seeds_with_the_same_result():
    c = af._case(5, 2, 3, 7, 8, causal=True)
    q, k, v, go = (t.double() for t in af.make_operands(c, seed=5))
    o, p = attn_forward_math(q, k, v, 0.3, True)
    whole = attn_vjp_math(go, q, k, v, o, p, 5, 0.3)
    one_seed = 3 * 2 * 3 * 7 * 7 * 8
    for budget in (one_seed, 2 * one_seed + 1, 1):
        for a, b in zip(attn_vjp_math(go, q, k, v, o, p, 5, 0.3, max_bytes=budget), whole):
            assert torch.equal(a, b)
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = F.scaled_dot_product_attention(qr, kr, vr, is_causal=True, scale=0.3)
    for s in range(5):
        want = torch.autograd.grad(out, (qr, kr, vr), go.reshape(5, 2, 3, 7, 8)[s], retain_graph=True)
        for a, w in zip(whole, want):
            assert af.rel(a.reshape(5, 2, 3, 7, 8)[s], w) < 1e-12


@pytest.mark.parametrize("lik", ["classification", "regression"])
@pytest.mark.parametrize("name", af.MODELS)
def test_curvature_on_the_emulation_matches_the_oracle(name, lik):
    from laplace_amd import _lib
    from tests.emulated_kernels import EmulatedKernels

    prev = _lib.set_kernels_for_testing(EmulatedKernels())
    try:
        af.run_curvature_checks("cpu", name, lik)
    finally:
        _lib.set_kernels_for_testing(prev)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
class _Attn(nn.Module):
    def __init__(self, how):
        super().__init__()
        self.how = how
        self.l = nn.Linear(8, 8)
        self.head = nn.Linear(8, 3)
        self.register_buffer("mask", torch.zeros(4, 4))
        self.register_buffer("wide", torch.zeros(2, 4, 8))
        if how == "trainable-attr":
            self.free = nn.Parameter(torch.zeros(1, 4, 8))

    def forward(self, x):
        how = self.how
        h = self.l(x)
        if how == "trainable-attr":
            h = h + self.free
        if how == "reducing-broadcast":
            h = h.mean(1, keepdim=True) + self.wide[:1]
        q = h.view(x.size(0), x.size(1), 2, -1).transpose(1, 2)
        kv = q[:, :, :2] if how == "cross" else q
        if how == "mask":
            a = F.scaled_dot_product_attention(q, q, q, attn_mask=self.mask)
        elif how == "dropout":
            a = F.scaled_dot_product_attention(q, q, q, dropout_p=0.1)
        elif how == "gqa":
            a = F.scaled_dot_product_attention(q, q, q, enable_gqa=True)
        elif how == "batch-permute":
            a = F.scaled_dot_product_attention(q, q, q).permute(2, 1, 0, 3).permute(2, 1, 0, 3)
        elif how == "batch-transpose":
            a = F.scaled_dot_product_attention(q, q, q).transpose(0, 2).transpose(0, 2)
        else:
            a = F.scaled_dot_product_attention(q, kv, kv)
        return self.head(a.transpose(1, 2).reshape(x.size(0), x.size(1), -1).mean(1))


REFUSALS = {"mask": "attn_mask", "dropout": "dropout_p", "gqa": "enable_gqa", "cross": "Tq == Tk",
            "trainable-attr": "graph reads attributes directly", "batch-permute": "moves the batch dim",
            "batch-transpose": "moves the batch dim", "reducing-broadcast": "needs a reduction"}


@pytest.mark.parametrize("how", sorted(REFUSALS))
def test_what_is_not_served_is_refused_by_name_and_the_tape_answers(how):
    torch.manual_seed(1)
    model = _Attn(how).eval()
    X = torch.randn(3, 4, 8)
    if how == "cross":
        # (tensor indexing is refused earlier; the cross-attention refusal is the rule's own, asked directly)
        sweep = SeedBatchedSweep(_Attn("plain").eval(), {}, kernels=None)
        r = next(r for r in sweep.rule.values() if r.kind == ATTN)
        with pytest.raises(SweepUnsupported, match="Tq == Tk"):
            sweep._run_attn(r, torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 3, 4), torch.zeros(1, 2, 3, 4))
    else:
        with pytest.raises(SweepUnsupported, match=REFUSALS[how]):
            SeedBatchedSweep(model, _taps(model), kernels=None).forward(X)
    if how == "dropout":
        return  # (its tape would draw a mask per pass even in eval mode: nothing to compare)
    from laplace_amd import HipGGN, _lib
    from oracle import curvature_oracle as co
    from tests.emulated_kernels import EmulatedKernels

    prev = _lib.set_kernels_for_testing(EmulatedKernels())
    try:
        backend = HipGGN(model, "classification")
        Js, f = backend.jacobians(X)
        # (a free parameter takes the backend's generic route as a whole, which asks no sweep)
        assert how in ("cross", "trainable-attr") or REFUSALS[how] in backend._tape().sweep_reason
    finally:
        _lib.set_kernels_for_testing(prev)
    import copy

    Js64, f64 = co.jacobians(copy.deepcopy(model).double(), X.double())
    assert af.rel(f, f64) < 1e-5 and af.rel(Js, Js64) < 1e-4


def test_split_sweep_names_the_attention_node():
    from laplace_amd.sweep_nhwc import SplitSweep
    from tests.emulated_kernels import EmulatedKernels

    for name in af.MODELS:
        model, _, X = af.make_model(name)
        K = EmulatedKernels()
        sweep = SplitSweep(model, _taps(model), kernels=lambda: K)
        assert not sweep.split_ok and "scaled_dot_product_attention" in sweep.split_reason
        f = sweep.forward(X)  # (the NCHW walk)
        assert af.rel(f, model(X)) < 1e-5


def test_frozen_parameter_is_a_constant_and_drops_its_cotangent():
    model, m64, X = af.make_model("attnseq")
    sweep = SeedBatchedSweep(m64, _taps(m64), kernels=None)
    consts = [r for r in sweep.rule.values() if r.kind == CONST]
    assert len(consts) == 1 and consts[0].args == ("pos",)


# ---- the kernel branch of the rule on the CPU ------------------------------------------------------------------------------------
def test_kernel_branch_detects_layouts_copies_nothing_and_matches_the_math():
    from tests.emulated_attn_kernels import EmulatedAttnKernels

    K = EmulatedAttnKernels()
    model, _, X = af.make_model("attnseq-causal")
    taps = _taps(model)
    ker = SeedBatchedSweep(model, taps, kernels=lambda: K)
    ref = SeedBatchedSweep(model, taps, kernels=lambda: K)
    ref.use_attn_kernels = False
    f, f_ref = ker.forward(X), ref.forward(X)
    assert [s[0] for s in K.seen] == ["forward"] and K.seen[0][1] == 1  # (Linear -> view -> transpose: layout 1, as it lies)
    node = next(n for n, r in ker.rule.items() if r.kind == ATTN)
    saved = ker.saved[node]
    assert saved[0] is K and ref.saved[next(n for n, r in ref.rule.items() if r.kind == ATTN)][0] is None
    assert af.rel(f, f_ref) < 1e-5
    torch.manual_seed(2)
    seeds = torch.randn(3, *f.shape)
    g, g_ref = ker.backward(seeds), ref.backward(seeds)
    assert [s[0] for s in K.seen] == ["forward", "vjp"] and K.seen[1][1] == 1
    assert K.seen[1][2][1:4] == K.seen[0][2]  # (the VJP read the very operands the forward read: no copy in between)
    for n in taps:
        assert af.rel(g[n], g_ref[n]) < 1e-4, n


@pytest.mark.parametrize("layout", ["contiguous", "transposed", "foreign", "mixed"])
def test_operand_layouts_of_the_kernel_branch(layout):
    from laplace_amd.sweep import attn_layout, attn_operands
    from tests.emulated_attn_kernels import EmulatedAttnKernels

    K = EmulatedAttnKernels()
    torch.manual_seed(4)
    B, H, T, D, S = 2, 3, 5, 4, 2
    base = [torch.randn(B, H, T, D) for _ in range(3)]
    if layout == "contiguous":
        ops, want = base, 0
    elif layout == "transposed":
        ops, want = [af.in_layout(t, 1) for t in base], 1
    elif layout == "foreign":  # [B][H][D][T] memory: neither layout
        ops, want = [t.transpose(2, 3).contiguous().transpose(2, 3) for t in base], 0
    else:
        ops, want = [base[0], af.in_layout(base[1], 1), base[2]], 0
    got_layout, used = attn_operands(*ops)
    assert got_layout == want
    same = [u.data_ptr() == t.data_ptr() for u, t in zip(used, ops)]
    assert all(same) if layout in ("contiguous", "transposed") else not all(same)
    o, lse = K.attn_forward(*ops, 0.5, False)
    assert tuple(o.shape) == (B, H, T, D) and attn_layout(o) == want
    o_ref, p = attn_forward_math(*base, 0.5, False)
    assert af.rel(o, o_ref) < 1e-5
    go = af.in_layout(torch.randn(S * B, H, T, D), want)
    got = K.attn_vjp(go, *ops, o, lse, S, 0.5, False)
    for a, w in zip(got, attn_vjp_math(go, *base, o_ref, p, S, 0.5)):
        assert tuple(a.shape) == (S * B, H, T, D) and attn_layout(a) == want
        assert af.rel(a, w) < 1e-5
    if want == 1:  # the transpose and view VJPs behind the node stay views
        back = got[0].permute(0, 2, 1, 3)
        assert back.is_contiguous() and back.reshape(S * B, T, H * D).data_ptr() == got[0].data_ptr()


def test_rule_sends_a_shape_outside_the_contract_to_the_math():
    from tests.emulated_attn_kernels import EmulatedAttnKernels

    K = EmulatedAttnKernels()
    sweep = SeedBatchedSweep(_Attn("plain").eval(), {}, kernels=lambda: K)
    assert sweep._attn_kernels(torch.zeros(1, 2, 4, 8), False) is K
    assert sweep._attn_kernels(torch.zeros(1, 2, 4, 6), False) is None  # odd head dim
    assert sweep._attn_kernels(torch.zeros(1, 2, 4, 132), False) is None  # D > 128
    assert sweep._attn_kernels(torch.zeros(1, 2, 4, 8, dtype=torch.float64), False) is None
    sweep.use_attn_kernels = False
    assert sweep._attn_kernels(torch.zeros(1, 2, 4, 8), False) is None
