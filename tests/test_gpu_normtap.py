"""Tracked BatchNorm and GroupNorm parameters on the NHWC split-fp16 sweep, on the device (-m gpu): the norm-tap Jacobian kernel alone
(csrc/lk_normtap.hip through the C ABI) against float64 torch on the CPU evaluated from the same fp16 planes and the same fp32
``x``, ``mu``, ``rstd``, and small networks with every normalisation parameter tracked through ``SplitSweep`` and ``HipGGN`` with
``nhwc_norm_taps`` on against float64 autograd.

Kernel level.  The shape table is tests/normtap_fixtures.CASES (tests/test_normtap_fixtures.py proves on the CPU that it reaches every
launch path and that the references tell the three mutants apart).  Full-mantissa operands: ``|Jw - ref| <= (L + 8) 2^-24 sum_l
|g| |xhat|`` and ``|Jb - ref| <= (L + 2) 2^-24 sum_l |g|`` element-wise (at most four roundings per term plus any summation order).
Integer-valued planes with a zero low plane and integer ``x`` come out equal to the integer result bit for bit, whatever the seed
split.  ``Js`` is filled with a sentinel that every column outside the two blocks keeps, guard bands of 64 elements round every
buffer keep their fill, and a second run gives the same bits.

End to end: tests/normtap_fixtures.E2E at the project's 1e-4 relative per block: 3 x 8 x 8 inputs, 4 samples
in two batches of 2, 3 classes.  The golden model ``normbn`` has 4-channel convolutions, which the implicit-GEMM kernels do not
cover: it stays on the NCHW sweep whatever the switch says and is held against its goldens on that route; ``bnres32`` is the same
architecture at 32 channels.  ``LK_TEST_DEVICE=cpu`` rehearses this file's host logic on the kernel emulation.
"""
import copy
import ctypes
import os

import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from oracle import curvature_oracle as co
from tests import normtap_fixtures as nf

pytestmark = pytest.mark.gpu
DEV = os.environ.get("LK_TEST_DEVICE", "cuda")
PAD = 64
SENTINEL = -7.25
PRIOR_PREC = 0.5


@pytest.fixture(autouse=True, scope="module")
def _kernels():
    if DEV != "cpu":
        yield
        return
    from laplace_amd import _lib
    from tests.emulated_normtap_kernels import EmulatedNormtapKernels

    prev = _lib.set_kernels_for_testing(EmulatedNormtapKernels())
    yield
    _lib.set_kernels_for_testing(prev)


@pytest.fixture(autouse=True)
def _norm_tap_route(monkeypatch):
    """the route under test is opt-in (``HipGGN.nhwc_norm_taps`` is off by default: DESIGN.md section 3)"""
    from laplace_amd.backend import _HipCurvatureMixin

    assert _HipCurvatureMixin.nhwc_norm_taps is False
    monkeypatch.setattr(_HipCurvatureMixin, "nhwc_norm_taps", True)


def rel(a, b):
    from tests.parity_log import record_error

    a, b = a.double().cpu(), b.double().cpu()
    return record_error((a - b).abs().max().item() / (b.abs().max().item() + 1e-300))


def check(got, want, tol=1e-4, what=""):
    e = rel(got, want)
    print(f"{what}: {e:.3e}")
    assert e < tol, f"{what}: rel err {e:.3e}"


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------------
class _Banded:
    """``numel`` elements inside guard bands of ``PAD`` elements; ``off``: the interior starts one element past an aligned address
    (4 bytes past 16 for fp32, 2 bytes past 16 for the fp16 planes)"""

    def __init__(self, shape, off, dtype=torch.float32, init=None, fill=7.5):
        n = 1
        for d in shape:
            n *= d
        self.fill = fill
        self.buf = torch.full((2 * PAD + n + 8,), fill, dtype=dtype, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.lo, self.hi = PAD + off, PAD + off + n
        self.t = self.buf[self.lo:self.hi].view(*shape)
        if init is not None:
            self.t.copy_(init)

    def bands_intact(self):
        return bool((self.buf[:self.lo] == self.fill).all()) and bool((self.buf[self.hi:] == self.fill).all())


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _launch(c, gh, gl, sexp, x, mu, rstd, Js):
    from laplace_amd._lib import SplitTensor, get_kernels

    K = get_kernels()
    P, w0, b0 = nf.columns(c)
    if DEV == "cpu":
        g = SplitTensor(torch.stack([gh.t, gl.t]).reshape(2, c["S"] * c["B"], c["L"], c["Ch"]), sexp)
        out = Js.t.clone()
        K.jac_norm_affine_nhwc(g, x.t.contiguous(), None if mu is None else mu.t.contiguous(),
                               None if rstd is None else rstd.t.contiguous(), c["S"], out, w0, b0, aligned=not c["off"])
        Js.t.copy_(out)
        return
    rc = K.lib.lk_jac_norm_affine_nhwc_f16x2(_p(gh.t), _p(gl.t), _p(sexp), _p(x.t), _p(None if mu is None else mu.t),
                                             _p(None if rstd is None else rstd.t), c["S"], c["B"], c["L"], c["Ch"], _p(Js.t), P, w0,
                                             b0, K._stream(Js.t.device))
    assert rc == 0, K.lib.lk_last_error()


def _within(got, want, bound, what):
    err = (got.double().cpu() - want).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    excess = (err - bound).max().item()
    print(f"{what}: worst |err| / bound {ratio:.3f}")
    assert excess <= 0.0, f"{what}: error exceeds the bound by {excess:.3e} ({ratio:.3f} of it)"


def _operands(c, g0, x0, mu0, rstd0):
    off, gshape = c["off"], (c["S"], c["B"], c["L"], c["Ch"])
    gh = _Banded(gshape, off, torch.float16, init=g0.planes[0].reshape(gshape))
    gl = _Banded(gshape, off, torch.float16, init=g0.planes[1].reshape(gshape))
    x = _Banded(x0.shape, off, init=x0)
    mu = None if mu0 is None else _Banded(mu0.shape, off, init=mu0)
    rstd = None if rstd0 is None else _Banded(rstd0.shape, off, init=rstd0)
    return gh, gl, g0.sexp.to(DEV), x, mu, rstd


@pytest.mark.parametrize("c", nf.CASES, ids=nf.case_id)
def test_kernel_against_float64(c):
    gen = torch.Generator().manual_seed(53 + nf.CASES.index(c))
    P, w0, b0 = nf.columns(c)
    Ch, off = c["Ch"], c["off"]
    gh, gl, sexp, x, mu, rstd = _operands(c, *nf.make_inputs(c, gen))
    if DEV != "cpu":  # the variant query names the launch this case takes on THESE addresses
        from laplace_amd._lib import get_kernels

        v = get_kernels().normtap_variant(c["S"], c["B"], c["L"], Ch, c["affine"], aligned=not off)
        assert v["vec"] == nf.plan(Ch, off)[0] and (gh.t.data_ptr() % 16 == 0) == (not off)
    Js = _Banded((c["B"], c["S"], P), off, fill=SENTINEL)
    _launch(c, gh, gl, sexp, x, mu, rstd, Js)
    Jw, Jb, bw, bb = nf.reference(c, torch.stack([gh.t, gl.t]), sexp, x.t, None if mu is None else mu.t,
                                  None if rstd is None else rstd.t)
    assert Js.bands_intact(), "Js: written outside its extent"
    assert all(b.bands_intact() for b in (gh, gl, x) + (() if mu is None else (mu, rstd))), "an operand was written"
    keep = torch.ones(P, dtype=torch.bool)
    if w0 >= 0:
        keep[w0:w0 + Ch] = False
        _within(Js.t[..., w0:w0 + Ch], Jw, bw, "weight columns")
    if b0 >= 0:
        keep[b0:b0 + Ch] = False
        _within(Js.t[..., b0:b0 + Ch], Jb, bb, "bias columns")
    assert bool((Js.t[..., keep.to(DEV)] == SENTINEL).all()), "a column outside the two blocks lost the sentinel"
    Js2 = _Banded((c["B"], c["S"], P), off, fill=SENTINEL)
    _launch(c, gh, gl, sexp, x, mu, rstd, Js2)
    assert torch.equal(Js.buf, Js2.buf), "two runs on the same input differ"

    # integers: every product and partial sum is exact, so the result is the integer result whatever the order and the seed split
    gh, gl, sexp, x, mu, rstd = _operands(c, *nf.make_integer_inputs(c, gen))
    Ji = _Banded((c["B"], c["S"], P), off, fill=SENTINEL)
    _launch(c, gh, gl, sexp, x, mu, rstd, Ji)
    Jw, Jb, _, _ = nf.reference(c, torch.stack([gh.t, gl.t]), sexp, x.t, None if mu is None else mu.t,
                                None if rstd is None else rstd.t)
    assert Ji.bands_intact()
    if w0 >= 0:
        assert torch.equal(Ji.t[..., w0:w0 + Ch].double().cpu(), Jw), "integer operands: weight columns are not exact"
    if b0 >= 0:
        assert torch.equal(Ji.t[..., b0:b0 + Ch].double().cpu(), Jb), "integer operands: bias columns are not exact"


def test_the_binding_checks_and_refuses():
    """the Python binding takes NHWC maps of any rank, refuses split tensors with one scale per image or chunk-major planes by
    name, non-contiguous operands and shapes that do not belong together, and hands a refusal of the C ABI to the caller"""
    from laplace_amd._lib import LaplaceHipError, SplitTensor, get_kernels

    K = get_kernels()
    c = dict(Ch=16, L=12, S=3, B=2, off=0, sexp=12, affine=True, wcol=True, bcol=True)
    g, x, mu, rstd = nf.make_inputs(c, torch.Generator().manual_seed(4))
    P, w0, b0 = nf.columns(c)
    gd = SplitTensor(g.planes.reshape(2, 6, 3, 4, 16).to(DEV), g.sexp.to(DEV))  # [S*B, H, W, C]
    xd, mud, rsd = x.reshape(2, 3, 4, 16).to(DEV), mu.to(DEV), rstd.to(DEV)
    Js = torch.zeros(2, 3, P, device=DEV)
    K.jac_norm_affine_nhwc(gd, xd, mud, rsd, 3, Js, w0, b0)
    Jw, Jb, bw, bb = nf.reference(c, g.planes, g.sexp, x, mu, rstd)
    _within(Js[..., w0:w0 + 16], Jw, bw, "weight columns")
    _within(Js[..., b0:b0 + 16], Jb, bb, "bias columns")
    per_image = SplitTensor(gd.planes, gd.sexp.expand(6).contiguous())
    with pytest.raises(LaplaceHipError, match="one scale per image"):
        K.jac_norm_affine_nhwc(per_image, xd, mud, rsd, 3, Js, w0, b0)
    chunked = SplitTensor(gd.planes, gd.sexp, chunked=True)
    with pytest.raises(LaplaceHipError, match="chunk-major"):
        K.jac_norm_affine_nhwc(chunked, xd, mud, rsd, 3, Js, w0, b0)
    with pytest.raises(LaplaceHipError, match="contiguous"):
        K.jac_norm_affine_nhwc(gd, xd.permute(0, 2, 1, 3), mud, rsd, 3, Js, w0, b0)
    if DEV != "cpu":
        with pytest.raises(LaplaceHipError, match="do not match"):
            K.jac_norm_affine_nhwc(gd, xd[:1], mud, rsd, 3, Js, w0, b0)
        with pytest.raises(LaplaceHipError, match="together"):
            K.jac_norm_affine_nhwc(gd, xd, mud, None, 3, Js, w0, b0)
        with pytest.raises(LaplaceHipError, match="columns overlap"):  # (the C ABI's own refusal reaches the caller)
            K.jac_norm_affine_nhwc(gd, xd, mud, rsd, 3, Js, 0, 8)


# ---- 2. networks with every normalisation parameter tracked -----------------------------------------------------------------------------
@pytest.fixture(scope="module", params=nf.E2E)
def e2e(request):
    """(name, fp64 CPU model, X, y, seeds, fp64 per-tap inputs and cotangents, oracle Jacobians, diagonal and the diagonal GLM
    predictive's variance) - computed once per fixture and left unchanged"""
    from tests.norm_sweep_fixtures import autograd_reference

    name = request.param
    m64, X, y = nf.e2e_fixture(name)
    seeds = torch.randn(4, X.shape[0], nf.E2E_CLASSES, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    f, ins, grads = autograd_reference(m64, nf.e2e_taps(m64), X, seeds)
    Js, _ = co.jacobians(m64, X)
    diag = co.ggn_diag(Js, co.functional_hessian(f.detach(), "classification"))
    f_var = torch.einsum("ncp,p,nkp->nck", Js, 1.0 / (diag + PRIOR_PREC), Js)
    return dict(name=name, m64=m64, X=X, y=y, seeds=seeds, f=f.detach(), ins=ins, grads=grads, Js=Js, diag=diag, f_var=f_var)


def _norm_sweep(b):
    """the sweep the backend built with the norm layers tapped: a ``SplitSweep`` that took the NHWC walk"""
    from laplace_amd.sweep_nhwc import SplitSweep

    tape = b._tape()
    sweep = tape.sweeps.get(frozenset({"norm"}))
    assert isinstance(sweep, SplitSweep), getattr(tape, "sweep_reason", None)
    assert sweep.split_ok and sweep.split_reason is None, sweep.split_reason
    return sweep


def test_e2e_taps_of_the_split_sweep_against_float64_autograd(e2e):
    from laplace_amd._lib import SplitTensor, get_kernels
    from laplace_amd.sweep_nhwc import NhwcNormGrad, SplitSweep

    model = copy.deepcopy(e2e["m64"]).float().to(DEV)
    taps = nf.e2e_taps(model)
    sw = SplitSweep(model, taps, kernels=get_kernels, nhwc_norm_taps=True)
    assert sw.split_ok and sw.split_reason is None, sw.split_reason
    f = sw.forward(e2e["X"].float().to(DEV))
    S, B = e2e["seeds"].shape[:2]
    grads = sw.backward(e2e["seeds"].float().to(DEV))
    assert sw.grad_scale == {}
    check(f, e2e["f"], what="f")
    for n, mod in taps.items():
        check(sw.taps[n]["a"], e2e["ins"][n], what=f"{n}: a")
        g = grads[n]
        if isinstance(mod, nf.NORMS):
            assert isinstance(g, (SplitTensor, NhwcNormGrad)), (n, type(g))
            g = SplitSweep.norm_grad_nchw(g, S, B)
        assert tuple(g.shape) == tuple(e2e["grads"][n].shape), n
        check(g, e2e["grads"][n], what=f"{n}: cotangent")


def _in_two_batches(b, Xd, yd):
    """``(Js, f, diagonal)`` over two batches of 2, the diagonal summed as a fit does"""
    parts = [(*b.jacobians(Xd[i:i + 2]), b.diag(Xd[i:i + 2], yd[i:i + 2])[1]) for i in range(0, Xd.shape[0], 2)]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), sum(p[2] for p in parts)


def test_e2e_jacobians_diag_and_the_diagonal_predictive(e2e):
    from laplace_amd import HipGGN
    from laplace_amd.laplace import HipLaplace

    model = copy.deepcopy(e2e["m64"]).float().to(DEV)
    Xd, yd = e2e["X"].float().to(DEV), e2e["y"].to(DEV)
    b = HipGGN(model, "classification")
    Js, f, h = _in_two_batches(b, Xd, yd)
    _norm_sweep(b)
    check(f, e2e["f"], what="f")
    for n, lo, hi in nf.blocks(model):
        check(Js[..., lo:hi], e2e["Js"][..., lo:hi], what=f"jacobians: {n}")
        check(h[lo:hi], e2e["diag"][lo:hi], what=f"diag: {n}")
    la = HipLaplace(model, "classification", "all", "diag", prior_precision=PRIOR_PREC)
    la.fit(DataLoader(TensorDataset(Xd, yd), batch_size=2))
    _norm_sweep(la.backend)
    _, f_var = la._glm_predictive_distribution(Xd)
    _norm_sweep(la.backend)
    check(f_var, e2e["f_var"], what="diagonal GLM predictive variance")


@pytest.mark.parametrize("lik", ("classification", "regression"))
def test_the_golden_model_keeps_its_numbers_with_the_switch_on(lik):
    from laplace_amd import HipGGN
    from tests.norm_fixtures import golden_model, load_golden

    g = load_golden("normbn", lik)
    model, X, y = golden_model("normbn", g, device=DEV)
    b = HipGGN(model, lik)
    Js, f = b.jacobians(X)
    _, h = b.diag(X, y)
    sweep = b._tape().sweeps[frozenset({"norm"})]
    assert not sweep.split_ok and sweep.split_reason == "0: convolution outside the implicit-GEMM kernel's coverage"
    check(Js, torch.as_tensor(g["Js"]), what="jacobians")
    check(h, torch.as_tensor(g["h_ggn"]), what="diag GGN")


def test_resnet18_norm_columns_with_the_switch_on_equal_those_with_it_off():
    """``nets.ResNet18`` with tracked BatchNorm at batch 2 (tanh: two separately executed passes are compared)"""
    from laplace_amd import HipGGN
    from laplace_amd.sweep_nhwc import SplitSweep

    m, X, y = nf.resnet18_fixture()
    Xd, yd = X.to(DEV), y.to(DEV)
    on = HipGGN(copy.deepcopy(m).to(DEV), "classification")
    Js, _ = on.jacobians(Xd)
    _, h = on.diag(Xd, yd)
    _norm_sweep(on)
    off = HipGGN(copy.deepcopy(m).to(DEV), "classification")
    off.nhwc_norm_taps = False
    Js0, _ = off.jacobians(Xd)
    _, h0 = off.diag(Xd, yd)
    sweep = off._tape().sweeps[frozenset({"norm"})]
    assert isinstance(sweep, SplitSweep) and not sweep.split_ok and "tapped BatchNorm" in sweep.split_reason
    names = set(nf.norm_names(m))
    n_norm = 0
    for n, lo, hi in nf.blocks(m):
        if n.rsplit(".", 1)[0] in names:
            check(Js[..., lo:hi], Js0[..., lo:hi], what=f"jacobians, on against off: {n}")
            check(h[lo:hi], h0[lo:hi], what=f"diag, on against off: {n}")
            n_norm += 1
    assert n_norm == 40
