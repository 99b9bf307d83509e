"""nn.MultiheadAttention and the stock transformer encoder on the device (-m gpu): the strided entry points of csrc/lk_attn.hip
(lk_attn_fwd_strided_f32, lk_attn_vjp_strided_f32) through the C ABI on every shape of tests/attn_fixtures.CASES, and the
fixture models of tests/mha_fixtures.py end to end.

The strided entry points run the kernels of the layout-1 entry points on the same plan, so every output must be BIT-equal to
lk_attn_fwd_f32 / lk_attn_vjp_f32 with ``layout = 1`` on contiguous copies of the operands; tests/test_gpu_attn.py holds those to
their analytic error bounds, which bit equality inherits - no tolerance appears here.  The operands lie packed as
``[B, T, 3, H, D]`` (what ``in_proj`` leaves), the cotangents go into one NaN-filled ``[S, B, T, 3, H, D]`` buffer (what
``in_proj``'s VJP reads), both inside NaN guard bands."""
import ctypes

import pytest
import torch

from tests import attn_fixtures as af
from tests import mha_fixtures as mf

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64


def _layout1_cases():
    """every case of the table in layout 1: those that are, and the shapes of the others re-run in layout 1"""
    seen, out = set(), []
    for c in af.CASES:
        c1 = {**c, "layout": 1}
        key = tuple(sorted(c1.items()))
        if key not in seen:
            seen.add(key)
            out.append(c1)
    return out


CASES1 = _layout1_cases()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


class _Banded:
    """``rows`` rows of ``ld`` floats (all NaN) between NaN guard bands of ``PAD`` floats"""

    def __init__(self, rows, ld):
        self.buf = torch.full((2 * PAD + rows * ld,), float("nan"), device=DEV)
        self.t = self.buf[PAD:PAD + rows * ld].view(rows, ld)

    def bands_intact(self):
        return bool(self.buf[:PAD].isnan().all()) and bool(self.buf[-PAD:].isnan().all())


def _layout1(K, c, q, k, v, go):
    """the layout-1 entry points on contiguous ``[N, T, H, D]`` operands -> o, lse, dq, dk, dv"""
    S, B, H, T, D = c["S"], c["B"], c["H"], c["T"], c["D"]
    scale, causal = af.scale_of(c), int(c["causal"])
    st = K._stream(q.device)
    o, lse = torch.full_like(q, float("nan")), torch.full((B, H, T), float("nan"), device=DEV)
    assert K.lib.lk_attn_fwd_f32(_p(q), _p(k), _p(v), B, H, T, D, 1, scale, causal, _p(o), _p(lse), st) == 0, K.lib.lk_last_error()
    need = int(K.lib.lk_attn_vjp_workspace_bytes(S, B, H, T, D))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
    dq, dk, dv = (torch.full_like(go, float("nan")) for _ in range(3))
    rc = K.lib.lk_attn_vjp_f32(_p(go), _p(q), _p(k), _p(v), _p(o), _p(lse), S, B, H, T, D, 1, scale, causal, _p(dq), _p(dk), _p(dv),
                               _p(ws), need, st)
    assert rc == 0, K.lib.lk_last_error()
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)


def _strided(K, c, q, k, v, go, ldq, ldd, packed=True):
    """the strided entry points: operands packed into rows of ``ldq`` floats (``q | k | v | padding``; ``packed = False``: three
    buffers of their own), cotangents into rows of ``ldd`` floats -> the outputs as contiguous tensors, the banded buffers"""
    S, B, H, T, D = c["S"], c["B"], c["H"], c["T"], c["D"]
    E = H * D
    scale, causal = af.scale_of(c), int(c["causal"])
    st = K._stream(q.device)
    if packed:
        src = _Banded(B * T, ldq)
        ins = [src.t[:, i * E:(i + 1) * E] for i in range(3)]
        outb = _Banded(S * B * T, ldd)
        outs = [outb.t[:, i * E:(i + 1) * E] for i in range(3)]
        bufs = [src, outb]
    else:
        srcs, outbs = [_Banded(B * T, ldq) for _ in range(3)], [_Banded(S * B * T, ldd) for _ in range(3)]
        ins, outs = [b.t[:, :E] for b in srcs], [b.t[:, :E] for b in outbs]
        bufs = srcs + outbs
    for dst, t in zip(ins, (q, k, v)):
        dst.copy_(t.reshape(B * T, E))
    before = [b.buf.clone() for b in bufs]
    ob, lb, wsb = _Banded(B * T, E), _Banded(B * H, T), None
    rc = K.lib.lk_attn_fwd_strided_f32(_p(ins[0]), _p(ins[1]), _p(ins[2]), ldq, B, H, T, D, scale, causal, _p(ob.t), _p(lb.t), st)
    assert rc == 0, K.lib.lk_last_error()
    need = int(K.lib.lk_attn_vjp_workspace_bytes(S, B, H, T, D))
    wsb = _Banded(1, max(need // 4, 4))
    rc = K.lib.lk_attn_vjp_strided_f32(_p(go), _p(ins[0]), _p(ins[1]), _p(ins[2]), ldq, _p(ob.t), _p(lb.t), S, B, H, T, D, scale, causal,
                                       _p(outs[0]), _p(outs[1]), _p(outs[2]), ldd, _p(wsb.t), need, st)
    assert rc == 0, K.lib.lk_last_error()
    for b in (ob, lb, wsb, *bufs):
        assert b.bands_intact(), "written outside an extent"
    n_in = 1 if packed else 3
    for b, was in zip(bufs[:n_in], before[:n_in]):  # (NaN == NaN is false: compare the bits)
        assert torch.equal(b.buf.view(torch.int32), was.view(torch.int32)), "an input changed"
    for b in bufs[n_in:]:  # the columns past the last output of a row are still NaN
        used = 3 * E if packed else E
        assert bool(b.t[:, used:].isnan().all()), "a padding column was written"
    got = dict(o=ob.t.view(B, T, H, D), lse=lb.t.view(B, H, T), **{n: t.reshape(S * B, T, H, D) for n, t in zip(("dq", "dk", "dv"), outs)})
    for n, t in got.items():
        assert not t.isnan().any(), f"{n}: an element was not written"
    return {n: t.clone() for n, t in got.items()}


def _operands(c):
    """contiguous ``[N, T, H, D]`` device operands of a layout-1 case"""
    return tuple(t.transpose(1, 2).contiguous().to(DEV) for t in af.make_operands(c))


@pytest.mark.parametrize("c", CASES1, ids=af.case_id)
def test_packed_operands_are_bit_equal_to_layout_1(c):
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    ops = _operands(c)
    E = c["H"] * c["D"]
    want = _layout1(K, c, *ops)
    got = _strided(K, c, *ops, 3 * E, 3 * E)
    again = _strided(K, c, *ops, 3 * E, 3 * E)
    for n in af.OUTPUTS:
        assert torch.equal(got[n], want[n]), f"{n} differs from the layout-1 entry point"
        assert torch.equal(got[n], again[n]), f"{n}: two equal calls differ"


PADDED = [c for c in CASES1 if (c["T"], c["D"]) in ((1, 4), (33, 20), (65, 8), (257, 64), (129, 64), (16, 8))]


@pytest.mark.parametrize("c", PADDED, ids=af.case_id)
def test_padded_rows_and_the_layout_1_strides(c):
    """``ldq > 3 E`` and ``ldd > 3 E`` (the padding columns stay NaN), different paddings of the two; and ``ldq = ldd = H D`` on
    three buffers of their own, which is layout 1 itself"""
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    ops = _operands(c)
    E = c["H"] * c["D"]
    want = _layout1(K, c, *ops)
    for ldq, ldd, packed in ((3 * E + 8, 3 * E + 4, True), (3 * E, 3 * E + 12, True), (E, E, False), (E + 4, E, False)):
        got = _strided(K, c, *ops, ldq, ldd, packed)
        for n in af.OUTPUTS:
            assert torch.equal(got[n], want[n]), f"{n} differs at ldq={ldq}, ldd={ldd}"


def test_the_wrappers_take_views_of_a_packed_projection():
    """`attn_forward_strided` / `attn_vjp_strided` on ``qkv.view(B, T, 3, H, D).unbind(2)``: no copy, the values of layout 1"""
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    c = dict(S=3, B=2, H=3, T=33, D=8, layout=1, causal=False, big=False)
    q, k, v, go = _operands(c)
    S, B, H, T, D = 3, 2, 3, 33, 8
    qkv = torch.stack((q, k, v), 2).contiguous()  # [B, T, 3, H, D]
    o, lse = K.attn_forward_strided(*qkv.unbind(2), af.scale_of(c), False)
    dqkv = torch.full((S * B, T, 3, H, D), float("nan"), device=DEV)
    K.attn_vjp_strided(go, *qkv.unbind(2), o, lse, S, af.scale_of(c), False, *dqkv.unbind(2))
    want = _layout1(K, c, q, k, v, go)
    assert torch.equal(o, want["o"]) and torch.equal(lse, want["lse"])
    for i, n in enumerate(("dq", "dk", "dv")):
        assert torch.equal(dqkv[:, :, i], want[n])
    from laplace_amd._lib import LaplaceHipError

    with pytest.raises(LaplaceHipError, match="share one row stride"):
        K.attn_forward_strided(qkv[:, :, 0], qkv[:, :, 1], v, 1.0, False)


# ---- the fixture models end to end ---------------------------------------------------------------------------------------------------
SWITCHES = {"strided": {}, "copies": dict(use_strided_attn=False), "math": dict(use_attn_kernels=False), "tape": dict(use_sweep=False)}
_BASE = {}


@pytest.mark.parametrize("how", list(SWITCHES))
@pytest.mark.parametrize("name", mf.MODELS)
def test_fixture_models_against_the_oracle_on_the_twin(name, how):
    """jacobians, diag, full, a two-minibatch kron fit, the Kron and the diagonal predictive of every fixture model against the
    fp64 oracle run on the twin, with both switches on and off and on the autograd tape; every route gives the values of the
    first (each is within 1e-4 of the oracle: two routes differ by rounding only)"""
    attrs = SWITCHES[how]

    def configure(b):
        for k, v in attrs.items():
            setattr(b, k, v)

    got = mf.run_curvature_checks(DEV, name, "classification", configure, expect_sweep=how != "tape")
    base = _BASE.setdefault(name, got)
    for key, want in base.items():
        for a, w in (zip(got[key], want) if key == "kfacs" else [(got[key], want)]):
            assert mf.rel(a, w) < 2e-4, (how, key)


def test_the_sweep_of_a_fixture_model_calls_the_strided_entry_points(monkeypatch):
    from laplace_amd import HipGGN
    from laplace_amd._lib import HipKernels

    calls = []
    for fn in ("attn_forward_strided", "attn_vjp_strided", "attn_forward", "attn_vjp"):
        real = getattr(HipKernels, fn)
        monkeypatch.setattr(HipKernels, fn, lambda self, *a, _fn=fn, _real=real, **kw: (calls.append(_fn), _real(self, *a, **kw))[1])
    model, _, X = mf.make_model("encoder")
    backend = HipGGN(model.to(DEV), "classification")
    backend.jacobians(X.to(DEV))
    assert calls == ["attn_forward_strided"] * 2 + ["attn_vjp_strided"] * 2
    del calls[:]
    backend.use_strided_attn = False
    backend.jacobians(X.to(DEV))
    assert calls == ["attn_forward"] * 2 + ["attn_vjp"] * 2
