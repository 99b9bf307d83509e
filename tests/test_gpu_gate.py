"""The squeeze-and-excitation gate kernels (csrc/lk_gate.hip) and the NHWC walk that uses them (``SplitSweep.nhwc_mul``) on the
device.  ``LK_TEST_DEVICE=cpu`` rehearses the file on the emulation (tests/emulated_gate_kernels.py).

1. Every runnable case of tests/gate_fixtures.CASES through the C ABI on banded buffers (NaN / -0.0 guard bands, compared by bit
   pattern; outputs start as NaN), against the derived criteria of `gate_fixtures.violations`: the VJP without ``r`` is the fp32
   product bit for bit, with ``r`` within ``2^-23 (|g gate| + |r|)`` of the fp64 value, the reduce within
   ``(P + 1) 2^-24 sum_p |g x|``; the amax word holds the bit pattern of max|dx| of the kernel's own output; a second equal call
   gives the same bits; a split cotangent and its fp32 reconstruction give the same bits.
2. The two small SE networks through ``SplitSweep`` (taps against float64 autograd), ``HipGGN.jacobians`` / ``kron``, and the Kron
   GLM predictive against the fp64 oracle, at 1e-4 relative per block - the tolerance tests/test_gpu_cat.py and
   tests/test_gpu_slice.py hold on the split sweep - with ``split_ok`` true; the same models with the switch off (the NCHW
   sweep) agree with the switched-on results at that tolerance.
"""
import copy
import ctypes
import os

import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from oracle import curvature_oracle as co
from tests import gate_fixtures as gf
from tests.cat_fixtures import functional_variance_kron

pytestmark = pytest.mark.gpu
DEV = os.environ.get("LK_TEST_DEVICE", "cuda")
PAD = 64


@pytest.fixture(autouse=True, scope="module")
def _kernels():
    if DEV != "cpu":
        yield
        return
    from laplace_amd import _lib
    from tests.emulated_gate_kernels import EmulatedGateKernels

    prev = _lib.set_kernels_for_testing(EmulatedGateKernels())
    yield
    _lib.set_kernels_for_testing(prev)


def rel(a, b):
    from tests.parity_log import record_error

    a, b = a.double().cpu(), b.double().cpu()
    return record_error((a - b).abs().max().item() / (b.abs().max().item() + 1e-300))


def check(got, want, tol=1e-4, what=""):
    e = rel(got, want)
    print(f"{what}: {e:.3e}")
    assert e < tol, f"{what}: rel err {e:.3e}"


# ---- 1. the kernels alone ---------------------------------------------------------------------------------------------------------
class _Banded:
    """``numel`` elements inside guard bands of ``PAD`` elements filled with ``fill`` (NaN or -0.0: compared by bit pattern);
    ``off``: the interior starts one element past an aligned address (4 bytes past 16 for fp32, 2 bytes past 8 for the planes);
    the interior starts as NaN unless ``init`` is given"""

    def __init__(self, shape, off, dtype=torch.float32, init=None, fill=float("nan")):
        n = 1
        for d in shape:
            n *= d
        self.buf = torch.full((2 * PAD + n + 8,), fill, dtype=dtype, device=DEV)
        self.lo, self.hi = PAD + off, PAD + off + n
        self.t = self.buf[self.lo:self.hi].view(*shape)
        if n:
            self.t.fill_(float("nan"))
        self.bands = self._bits(torch.cat([self.buf[:self.lo], self.buf[self.hi:]])).clone()
        if init is not None and n:
            self.t.copy_(init)

    @staticmethod
    def _bits(t):
        return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)

    def ptr(self):
        """address of the interior (of the allocation plus the offset: an empty view reports a null data_ptr)"""
        return ctypes.c_void_p(self.buf.data_ptr() + self.lo * self.buf.element_size())

    def bands_intact(self):
        return torch.equal(self._bits(torch.cat([self.buf[:self.lo], self.buf[self.hi:]])), self.bands)


class _Operands:
    """the inputs of a case in banded device buffers; ``g`` in the case's own form and - for a split case - also as the fp32
    reconstruction of its planes"""

    def __init__(self, c, inp):
        S, B, P, C, off = c["S"], c["B"], c["P"], c["C"], c["off"]
        self.c = c
        self.g32 = _Banded((S * B, P, 1, C), off, init=inp["g"].reshape(S * B, P, 1, C), fill=-0.0)
        self.planes = None
        if c["split"]:
            pl = inp["g_split"].planes
            self.planes = (_Banded((S * B, P, 1, C), off, torch.float16, init=pl[0]),
                           _Banded((S * B, P, 1, C), off, torch.float16, init=pl[1], fill=-0.0))
            self.sexp = inp["g_split"].sexp.to(DEV)
        if c["kind"] == "reduce":
            self.x = _Banded((B, P, 1, C), off, init=inp["x"].reshape(B, P, 1, C))
        else:
            self.gate = _Banded((B, C), off, init=inp["gate"], fill=-0.0)
            self.r = None if inp["r"] is None else _Banded((S * B, C), off, init=inp["r"].reshape(S * B, C))

    def all(self):
        return [b for b in (self.g32, *(self.planes or ()), getattr(self, "x", None), getattr(self, "gate", None), getattr(self, "r", None))
                if b is not None]


def _run(ops, out, amax, as_split):
    """one call of the case's entry point through the C ABI (the emulation's method when rehearsing on the CPU)"""
    from laplace_amd._lib import SplitTensor, get_kernels

    K, c = get_kernels(), ops.c
    S, B, P, C = c["S"], c["B"], c["P"], c["C"]
    if DEV == "cpu":
        if not B:
            return
        g = SplitTensor(torch.stack([ops.planes[0].t, ops.planes[1].t]), ops.sexp) if as_split else ops.g32.t.contiguous()
        if c["kind"] == "reduce":
            out.t.copy_(K.gate_reduce(g, ops.x.t.contiguous(), S))
        else:
            out.t.copy_(K.gate_vjp(g, ops.gate.t.contiguous(), None if ops.r is None else ops.r.t.contiguous(), S, amax=amax))
        return
    gp = (None, ops.planes[0].ptr(), ops.planes[1].ptr(), ctypes.c_void_p(ops.sexp.data_ptr())) if as_split else (ops.g32.ptr(), None, None, None)
    st = K._stream(out.buf.device)
    if c["kind"] == "reduce":
        rc = K.lib.lk_gate_reduce_nhwc_f32(*gp, ops.x.ptr(), S, B, P, C, out.ptr(), st)
    else:
        rc = K.lib.lk_gate_vjp_nhwc_f32(*gp, ops.gate.ptr(), None if ops.r is None else ops.r.ptr(), S, B, P, C, out.ptr(),
                                        None if amax is None else ctypes.c_void_p(amax.data_ptr()), st)
    assert rc == 0, K.lib.lk_last_error()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("c", [c for c in gf.CASES if not c["wide"]], ids=gf.case_id)
def test_kernels_against_the_criteria(c):
    from tests.parity_log import record_error

    inp = gf.make_inputs(c, torch.Generator().manual_seed(100 + gf.CASES.index(c)))
    ref = gf.reference(c, inp)
    ops = _Operands(c, inp)
    S, B, P, C = c["S"], c["B"], c["P"], c["C"]
    shape = (S * B, C) if c["kind"] == "reduce" else (S * B, P, 1, C)

    def call(as_split, with_amax):
        out = _Banded(shape, c["off"], fill=-0.0 if as_split else float("nan"))
        amax = torch.zeros(1, device=DEV) if with_amax else None
        _run(ops, out, amax, as_split)
        assert out.bands_intact(), "the output: written outside its extent"
        return out, amax

    out, amax = call(c["split"], c["amax"])
    assert bool(torch.isfinite(out.t).all()), "the output: an element was not written"
    bad = gf.violations(c, out.t, ref, inp)
    print(f"{gf.case_id(c)}: worst error / bound {record_error(gf.worst_ratio(c, out.t, ref, inp)):.3f}")
    assert not bad, bad
    if amax is not None:
        want = out.t.abs().max().reshape(1) if out.t.numel() else torch.zeros(1, device=DEV)
        assert torch.equal(amax.view(torch.int32), want.view(torch.int32)), "amax is not the bit pattern of max|dx| of the output"
    out2, amax2 = call(c["split"], c["amax"])
    assert torch.equal(_bits(out.t), _bits(out2.t)), "two equal calls differ"
    assert amax is None or torch.equal(amax, amax2)
    if c["kind"] == "vjp":  # (with and without the amax word: the same dx)
        out3, _ = call(c["split"], not c["amax"])
        assert torch.equal(_bits(out.t), _bits(out3.t)), "the amax word changes dx"
    if c["split"]:
        out4, _ = call(False, c["amax"])
        assert torch.equal(_bits(out.t), _bits(out4.t)), "a split g and its fp32 reconstruction give different bits"
    assert all(b.bands_intact() for b in ops.all()), "an input was written"


def test_the_bindings():
    """the Python bindings allocate what the C ABI takes and refuse what does not belong together"""
    from laplace_amd._lib import LaplaceHipError, SplitTensor, get_kernels

    K = get_kernels()
    c = dict(kind="vjp", S=3, B=2, P=12, C=20, split=True, off=0, r=True, amax=True, wide=False)
    inp = gf.make_inputs(c, torch.Generator().manual_seed(9))
    gs = SplitTensor(inp["g_split"].planes.reshape(2, 6, 3, 4, 20).to(DEV), inp["g_split"].sexp.to(DEV))
    g32 = inp["g"].reshape(6, 3, 4, 20).to(DEV)
    gate, r = inp["gate"].to(DEV), inp["r"].reshape(6, 20).to(DEV)
    word = torch.zeros(1, device=DEV)
    dx = K.gate_vjp(gs, gate, r, 3, amax=word)
    assert tuple(dx.shape) == (6, 3, 4, 20) and not gf.violations(c, dx, gf.reference(c, inp), inp)
    assert torch.equal(word, dx.abs().max().reshape(1)) and torch.equal(K.gate_vjp(g32, gate, r, 3), dx)
    assert torch.equal(K.gate_vjp(g32, gate, None, 3).cpu(), (inp["g"] * inp["gate"][None, :, None, :]).reshape(6, 3, 4, 20))
    cr = dict(c, kind="reduce")
    x = gf.full_mantissa((2, 3, 4, 20), torch.Generator().manual_seed(10))
    ds = K.gate_reduce(gs, x.to(DEV), 3)
    inr = dict(g=inp["g"], x=x.reshape(2, 12, 20))
    assert tuple(ds.shape) == (6, 20) and not gf.violations(cr, ds, gf.reference(cr, inr), inr)
    assert torch.equal(K.gate_reduce(g32, x.to(DEV), 3), ds)
    if DEV != "cpu":
        with pytest.raises(LaplaceHipError):
            K.gate_reduce(g32, x.to(DEV), 2)  # (six maps are not two seeds of two samples)
        with pytest.raises(LaplaceHipError):
            K.gate_vjp(g32, gate[:, :19].contiguous(), None, 3)
        with pytest.raises(LaplaceHipError):
            K.gate_vjp(g32, gate, r[:5], 3)
        with pytest.raises(LaplaceHipError):
            K.gate_vjp(g32, gate, r, 3, amax=torch.zeros(2, device=DEV))
        with pytest.raises(LaplaceHipError):  # (one scale per image is a forward operand)
            K.gate_reduce(SplitTensor(gs.planes, torch.zeros(6, dtype=torch.int32, device=DEV)), x.to(DEV), 3)
        with pytest.raises(LaplaceHipError):
            K.gate_vjp(SplitTensor(gs.planes, gs.sexp, chunked=True), gate, r, 3)  # (chunk-major planes are no NHWC map)
        with pytest.raises(LaplaceHipError, match="dx overlaps"):
            K._rc(K.lib.lk_gate_vjp_nhwc_f32(g32.data_ptr(), None, None, None, gate.data_ptr(), None, 3, 2, 12, 20, g32.data_ptr(), None,
                                             None), "lk_gate_vjp_nhwc_f32")


# ---- 2. the small networks -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["se", "linear-gate"])
def e2e(request):
    """(fp64 CPU model, X, y, seeds, fp64 per-tap inputs and cotangents, oracle Jacobians, factors and predictive variance) -
    computed once per fixture and left unchanged"""
    from tests.norm_sweep_fixtures import autograd_reference

    kind = request.param
    m64, X, y = gf.se_net() if kind == "se" else gf.linear_gate_net()
    seeds = torch.randn(4, X.shape[0], gf.E2E_CLASSES, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    f, ins, grads = autograd_reference(m64, gf.taps(m64), X, seeds)
    Js, _ = co.jacobians(m64, X)
    loss, kf = co.kfac_ggn(m64, X, y, X.shape[0], "classification")
    Qs, ls = co.kron_decompose(kf)
    f_var = functional_variance_kron(Js, Qs, ls, 0.5)
    Hl = co.functional_hessian(f.detach(), "classification")
    return dict(kind=kind, m64=m64, X=X, y=y, seeds=seeds, f=f.detach(), ins=ins, grads=grads, Js=Js, loss=loss, kf=kf, f_var=f_var,
                h=co.ggn_diag(Js, Hl))


@pytest.mark.parametrize("on", (True, False), ids=("nhwc_mul", "default"))
def test_e2e_taps_of_the_sweep_against_float64_autograd(e2e, on, monkeypatch):
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep_nhwc import SplitSweep

    monkeypatch.setattr(SplitSweep, "nhwc_mul", on)
    model = copy.deepcopy(e2e["m64"]).float().to(DEV)
    taps = gf.taps(model)
    sw = SplitSweep(model, taps, kernels=get_kernels)
    assert sw.split_ok == on, sw.split_reason
    assert on or sw.split_reason == "mul has no NHWC rule"
    f = sw.forward(e2e["X"].float().to(DEV))
    grads = sw.backward(e2e["seeds"].float().to(DEV))
    check(f, e2e["f"], what="f")
    for n in taps:
        check(sw.taps[n]["a"], e2e["ins"][n], what=f"{n}: a")
        assert tuple(grads[n].shape) == tuple(e2e["grads"][n].shape), n
        check(grads[n], e2e["grads"][n], what=f"{n}: cotangent")


def _backend_checks(e2e, what, want_split):
    from laplace_amd import HipGGN
    from laplace_amd.laplace import HipLaplace
    from laplace_amd.sweep_nhwc import SplitSweep

    m64, X, y = e2e["m64"], e2e["X"], e2e["y"]
    model = copy.deepcopy(m64).float().to(DEV)
    Xd, yd = X.float().to(DEV), y.to(DEV)
    b = HipGGN(model, "classification")
    Js, f = b.jacobians(Xd)
    check(f, e2e["f"], what=f"{what}: f")
    check(Js, e2e["Js"], what=f"{what}: jacobians")
    _, h = b.diag(Xd, yd)
    check(h, e2e["h"], what=f"{what}: diag")
    loss, kron = b.kron(Xd, yd, N=X.shape[0])
    tape = b._tape()
    assert not getattr(tape, "sweep_reason", None), tape.sweep_reason
    assert isinstance(tape.sweep, SplitSweep) and tape.sweep.split_ok == want_split, getattr(tape.sweep, "split_reason", None)
    check(loss, e2e["loss"], what=f"{what}: loss")
    facs = [a for F_ in kron.kfacs for a in F_]
    for i, (a, ref) in enumerate(zip(facs, [r for G_ in e2e["kf"] for r in G_])):
        check(a, ref, what=f"{what}: kron factor {i}")
    la = HipLaplace(model, "classification", "all", "kron", prior_precision=0.5)
    la.fit(DataLoader(TensorDataset(Xd, yd), batch_size=X.shape[0]))
    _, f_var = la._glm_predictive_distribution(Xd)
    check(f_var, e2e["f_var"], what=f"{what}: Kron GLM predictive variance")
    return dict(Js=Js, h=h, f_var=f_var, facs=facs)


def test_e2e_curvature_against_the_oracle_with_the_switch_on_and_off(e2e, monkeypatch):
    from laplace_amd.sweep_nhwc import SplitSweep

    monkeypatch.setattr(SplitSweep, "nhwc_mul", True)
    on = _backend_checks(e2e, f"{e2e['kind']} (nhwc_mul)", want_split=True)
    monkeypatch.setattr(SplitSweep, "nhwc_mul", False)
    off = _backend_checks(e2e, f"{e2e['kind']} (default)", want_split=False)
    for k in ("Js", "h", "f_var"):
        check(off[k], on[k], what=f"{e2e['kind']}: default against nhwc_mul: {k}")
    for i, (a, b) in enumerate(zip(off["facs"], on["facs"])):
        check(a, b, what=f"{e2e['kind']}: default against nhwc_mul: kron factor {i}")
