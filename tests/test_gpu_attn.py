"""Scaled dot-product attention in the seed-batched reverse sweep, on the device (-m gpu): the kernels alone (csrc/lk_attn.hip
through the C ABI) on every case of tests/attn_fixtures.CASES against float64 evaluated from the same fp32 operands, inside the
fixtures' analytic bounds (tests/test_attn_fixtures.py shows on the CPU that the table reaches every launch form, that fp32
restatements sit below the bounds and that the mutants leave them); then the fixture models and a small ``nets.ViTSmall`` through
``HipGGN`` / ``HipLaplace`` against the fp64 oracle, with the kernels and with ``use_attn_kernels = False``.

The VJP is fed the forward's own ``o`` and ``lse``, as the sweep feeds it; its bounds include the forward's error."""
import ctypes

import pytest
import torch

from tests import attn_fixtures as af

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64
WORST = {}


@pytest.fixture(autouse=True, scope="module")
def _report():
    """the worst error / bound per output, printed when the module is done (pytest -s): what profiles/attn_instances.md records"""
    yield
    for key, (r, name) in sorted(WORST.items()):
        print(f"\n{key:4s} worst error / bound {r:.4f}  ({name})", end="")


class _Banded:
    """a ``[N, H, T, D]`` tensor in memory layout 0 or 1 (or any plain shape) inside NaN guard bands of ``PAD`` floats"""

    def __init__(self, shape, layout=0, init=None):
        phys = (shape[0], shape[2], shape[1], shape[3]) if layout == 1 else tuple(shape)
        n = 1
        for d in phys:
            n *= d
        self.buf = torch.full((2 * PAD + n,), float("nan"), device=DEV)
        self.lo, self.hi = PAD, PAD + n
        inner = self.buf[self.lo:self.hi].view(*phys)
        self.t = inner.transpose(1, 2) if layout == 1 else inner
        if init is not None:
            self.t.copy_(init)

    def bands_intact(self):
        return bool(self.buf[:self.lo].isnan().all()) and bool(self.buf[self.hi:].isnan().all())


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _run_case(K, c, ops):
    """forward and VJP of one case through the C ABI -> (outputs by name, their buffers, the input buffers)"""
    S, B, H, T, D, layout = c["S"], c["B"], c["H"], c["T"], c["D"], c["layout"]
    scale, causal = af.scale_of(c), int(c["causal"])
    q, k, v = (_Banded((B, H, T, D), layout, t) for t in ops[:3])
    go = _Banded((S * B, H, T, D), layout, ops[3])
    o, lse = _Banded((B, H, T, D), layout), _Banded((B, H, T))
    st = K._stream(q.t.device)
    rc = K.lib.lk_attn_fwd_f32(_p(q.t), _p(k.t), _p(v.t), B, H, T, D, layout, scale, causal, _p(o.t), _p(lse.t), st)
    assert rc == 0, K.lib.lk_last_error()
    need = int(K.lib.lk_attn_vjp_workspace_bytes(S, B, H, T, D))
    assert need >= 4 * S * B * H * T
    ws = _Banded((need // 4,))
    dq, dk, dv = (_Banded((S * B, H, T, D), layout) for _ in range(3))
    rc = K.lib.lk_attn_vjp_f32(_p(go.t), _p(q.t), _p(k.t), _p(v.t), _p(o.t), _p(lse.t), S, B, H, T, D, layout, scale, causal,
                               _p(dq.t), _p(dk.t), _p(dv.t), _p(ws.t), need, st)
    assert rc == 0, K.lib.lk_last_error()
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv, ws=ws), (q, k, v, go)


@pytest.mark.parametrize("c", af.CASES, ids=af.case_id)
def test_kernels_against_float64(c):
    """every output element within its bound; inputs unchanged; the NaN guard bands round every output and the workspace intact
    and no NaN left inside an output; a second call gives the same bits"""
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    ops = af.make_operands(c)
    ref = af.reference(c, *ops)
    dev_ops = tuple(t.to(DEV) for t in ops)
    out, ins = _run_case(K, c, dev_ops)
    for buf, src in zip(ins, dev_ops):
        assert torch.equal(buf.t, src) and buf.bands_intact(), "an input changed"
    got = {n: out[n].t for n in af.OUTPUTS}
    for n in af.OUTPUTS + ("ws",):
        assert out[n].bands_intact(), f"{n}: written outside its extent"
    for n in af.OUTPUTS:
        assert not got[n].isnan().any(), f"{n}: an element was not written"
    worst = af.ratios(ref, got)
    print(f"{af.case_id(c)}: worst |err| / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    for n, r in worst.items():
        if r > WORST.get(n, (0.0, ""))[0]:
            WORST[n] = (r, af.case_id(c))
    for n, r in worst.items():
        assert r <= 1.0, f"{n}: error is {r:.3f} of its bound"
    again, _ = _run_case(K, c, dev_ops)
    for n in af.OUTPUTS:
        assert torch.equal(out[n].t, again[n].t), f"{n}: two equal calls differ"


def test_one_position_is_exact():
    """T = 1: the only probability is 1, so dq = dk = 0 and dv = go exactly"""
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    for c in (c for c in af.CASES if c["T"] == 1):
        ops = tuple(t.to(DEV) for t in af.make_operands(c))
        out, _ = _run_case(K, c, ops)
        assert torch.equal(out["o"].t, ops[2]), af.case_id(c)
        assert not out["dq"].t.any() and not out["dk"].t.any(), af.case_id(c)
        assert torch.equal(out["dv"].t, ops[3]), af.case_id(c)


def test_binding_allocates_and_keeps_the_operands_layout():
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep import attn_layout

    K = get_kernels()
    c = af._case(3, 2, 3, 21, 12, 1, True)
    q, k, v, go = (t.to(DEV) for t in af.make_operands(c, seed=9))
    ref = af.reference(c, q.cpu(), k.cpu(), v.cpu(), go.cpu())
    o, lse = K.attn_forward(q, k, v, af.scale_of(c), True)
    dq, dk, dv = K.attn_vjp(go, q, k, v, o, lse, 3, af.scale_of(c), True)
    assert all(attn_layout(t) == 1 for t in (o, dq, dk, dv))
    assert max(af.ratios(ref, dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)).values()) <= 1.0
    # operands in different layouts are made contiguous: the same values within the bounds, layout 0 back
    o0, lse0 = K.attn_forward(q.contiguous(), k, v, af.scale_of(c), True)
    assert attn_layout(o0) == 0 and max(af.ratios(ref, dict(o=o0, lse=lse0)).values()) <= 1.0
    dq0, _, _ = K.attn_vjp(go, q.contiguous(), k.contiguous(), v.contiguous(), o0, lse0, 3, af.scale_of(c), True)
    assert attn_layout(dq0) == 0 and af.bound_ratio(dq0, ref["dq"], ref["b_dq"]) <= 1.0


def _route(on):
    def configure(backend):
        backend.use_attn_kernels = on

    return configure


@pytest.mark.parametrize("name", af.MODELS)
def test_fixture_models_with_and_without_the_kernels(name):
    """the `_run` body of tests/test_weight_sharing.py against the fp64 oracle, once per route; then the routes against each other"""
    on = af.run_curvature_checks(DEV, name, "classification", _route(True))
    off = af.run_curvature_checks(DEV, name, "classification", _route(False))
    for key in ("Js", "f", "h", "H", "f_var", "f_var_d"):
        assert af.rel(on[key], off[key]) < 1e-4, key
    for a, b in zip(on["kfacs"], off["kfacs"]):
        assert af.rel(a, b) < 1e-4
    af.run_curvature_checks(DEV, name, "regression", _route(True))


def test_the_kernels_serve_the_node_on_the_device():
    """the kernel object of the device has the entry points and the rule takes them (not the math) for an fp32 model"""
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep import ATTN, SeedBatchedSweep

    model, _, X = af.make_model("attnseq")
    model, X = model.to(DEV), X.to(DEV)
    sweep = SeedBatchedSweep(model, {"head": model.head}, kernels=get_kernels)
    sweep.forward(X)
    node = next(n for n, r in sweep.rule.items() if r.kind == ATTN)
    assert sweep.saved[node][0] is get_kernels()


def test_small_vit_kron_and_predictive():
    """nets.ViTSmall(dim=32, depth=2, heads=2) at batch 4 on 32 x 32 inputs (T = 64): kron factors and the Kron predictive
    against the oracle"""
    import copy

    from laplace_amd import nets
    from laplace_amd.laplace import HipLaplace
    from oracle import curvature_oracle as co

    torch.manual_seed(0)
    model = nets.ViTSmall(dim=32, depth=2, heads=2).to(DEV).eval()
    X = torch.randn(4, 3, 32, 32, device=DEV)
    y = torch.randint(10, (4,), device=DEV)
    m64 = copy.deepcopy(model).double().cpu()
    loader = af._Loader([(X, y)])
    loader.dataset = range(4)
    la = HipLaplace(model, "classification", "all", "kron", prior_precision=0.5)
    la.fit(loader)
    tape = la.backend._tape()
    assert getattr(tape, "sweep_reason", None) is None and tape.sweep not in (None, False)
    _, want = co.kfac_ggn(m64, X.double().cpu(), y.cpu(), 4, "classification")
    for F_, G_ in zip(la.H_facs.kfacs, want):
        for a_, w_ in zip(F_, G_):
            assert af.rel(a_, w_) < 1e-4
    _, f_var = la._glm_predictive_distribution(X)
    Js64, _ = co.jacobians(m64, X.double().cpu())
    Qs, ls = co.kron_decompose(want)
    assert af.rel(f_var, co.functional_variance_kron(Js64, Qs, ls, 0.5)) < 1e-4
