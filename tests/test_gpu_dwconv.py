"""Depthwise convolutions of the NHWC split-fp16 sweep on the device (-m gpu): the kernels alone (csrc/lk_dwconv.hip through the C
ABI) against float64 torch on the CPU evaluated from the same fp32 operands and the same fp16 planes, and three small
depthwise-separable networks through ``SplitSweep``, ``HipGGN`` and the Kron GLM predictive against float64 autograd and the oracle.

Kernel level.  The shape table is tests/dwconv_fixtures.CASES (tests/test_dwconv_fixtures.py proves on the CPU that it reaches
every launch path and that the references tell a correlation from a transposed convolution and a dropped divisibility test).
Forward and backward: ``|got - ref| <= gamma(T + 2) sum |w| |operand| + T 2^-126`` (derived in tests/dwconv_fixtures.py; it holds
for any summation order, with or without FMA).  Guard bands of 64 elements round ``y`` and ``dx`` keep their fill, ``amax`` is
``max|dx|`` bit for bit, and a second run gives the same bits.

End to end: tests/dwconv_fixtures.E2E at the project's 1e-4 relative per block: 3 x 16 x 16 inputs, 8 samples in
two batches of 4, 10 classes.  ``LK_TEST_DEVICE=cpu`` rehearses this file's host logic on the kernel emulation.
"""
import copy
import ctypes
import os

import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from oracle import curvature_oracle as co
from tests import dwconv_fixtures as df

pytestmark = pytest.mark.gpu
DEV = os.environ.get("LK_TEST_DEVICE", "cuda")
PAD = 64
PRIOR_PREC = 0.5


@pytest.fixture(autouse=True, scope="module")
def _kernels():
    if DEV != "cpu":
        yield
        return
    from laplace_amd import _lib
    from tests.emulated_dwconv_kernels import EmulatedDwconvKernels

    prev = _lib.set_kernels_for_testing(EmulatedDwconvKernels())
    yield
    _lib.set_kernels_for_testing(prev)


@pytest.fixture(autouse=True)
def _depthwise_route(monkeypatch):
    """the route under test is opt-in (``SplitSweep.nhwc_depthwise`` is off by default: DESIGN.md section 3)"""
    from laplace_amd.sweep_nhwc import SplitSweep

    monkeypatch.setattr(SplitSweep, "nhwc_depthwise", True)


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
    """``numel`` elements inside guard bands of ``PAD`` elements; ``off``: the interior starts one element past an aligned address
    (4 bytes past 16 for fp32, 2 bytes past 8 for the fp16 planes)"""

    def __init__(self, shape, off, dtype=torch.float32, init=None):
        n = 1
        for d in shape:
            n *= d
        self.fill = 7.5
        self.buf = torch.full((2 * PAD + n + 4,), self.fill, dtype=dtype, device=DEV)
        self.lo, self.hi = PAD + off, PAD + off + n
        self.t = self.buf[self.lo:self.hi].view(*shape)
        if init is not None:
            self.t.copy_(init)

    def bands_intact(self):
        return bool((self.buf[:self.lo] == self.fill).all()) and bool((self.buf[self.hi:] == self.fill).all())


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _forward(c, x, w, b, y):
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    if DEV == "cpu":
        y.t.copy_(K.dwconv_forward(x.t, w.t, None if b is None else b.t, c["k"], c["s"], c["p"]))
        return
    rc = K.lib.lk_dwconv_fwd_nhwc_f32(_p(x.t), _p(w.t), _p(None if b is None else b.t), c["B"], c["H"], c["W"], c["C"], *c["k"],
                                      *c["s"], *c["p"], _p(y.t), K._stream(x.t.device))
    assert rc == 0, K.lib.lk_last_error()


def _backward(c, gh, gl, sexp, w, dx, amax):
    from laplace_amd._lib import SplitTensor, get_kernels

    K = get_kernels()
    if DEV == "cpu":
        g = SplitTensor(torch.stack([gh.t, gl.t]).reshape(2, c["S"] * c["B"], *gh.t.shape[2:]), sexp)
        dx.t.copy_(K.dwconv_backward(g, w.t, c["S"], (c["H"], c["W"]), c["k"], c["s"], c["p"], amax=amax).reshape(dx.t.shape))
        return
    rc = K.lib.lk_dwconv_bwd_nhwc_f16x2(_p(gh.t), _p(gl.t), _p(sexp), _p(w.t), c["S"], c["B"], c["H"], c["W"], c["C"], *c["k"],
                                        *c["s"], *c["p"], _p(dx.t), _p(amax), K._stream(dx.t.device))
    assert rc == 0, K.lib.lk_last_error()


def _within(got, want, bound, what):
    err = (got.double().cpu() - want).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    excess = (err - bound).max().item()
    print(f"{what}: worst |err| / bound {ratio:.3f}")
    assert excess <= 0.0, f"{what}: error exceeds the bound by {excess:.3e} ({ratio:.3f} of it)"


@pytest.mark.parametrize("c", df.CASES, ids=df.case_id)
def test_kernels_against_float64(c):
    gen = torch.Generator().manual_seed(31 + df.CASES.index(c))
    off, (OH, OW), T = c["off"], df.out_hw(c), df.taps(c)
    x0, w0, b0, g0 = df.make_inputs(c, gen)
    x, w = _Banded(x0.shape, off, init=x0), _Banded(w0.shape, off, init=w0)
    b = None if b0 is None else _Banded(b0.shape, off, init=b0)
    y = _Banded((c["B"], OH, OW, c["C"]), off)
    _forward(c, x, w, b, y)
    ref, bound = df.forward_reference(c, x.t, w.t, None if b is None else b.t)
    assert y.bands_intact(), "y: written outside its extent"
    _within(y.t, ref, bound, "y")

    gshape = (c["S"], c["B"], OH, OW, c["C"])
    gh = _Banded(gshape, off, torch.float16, init=g0.planes[0].reshape(gshape))
    gl = _Banded(gshape, off, torch.float16, init=g0.planes[1].reshape(gshape))
    sexp = g0.sexp.to(DEV)
    dshape = (c["S"], c["B"], c["H"], c["W"], c["C"])
    dx, amax = _Banded(dshape, off), torch.zeros(1, device=DEV)
    _backward(c, gh, gl, sexp, w, dx, amax)
    want, bound = df.backward_reference(c, torch.stack([gh.t, gl.t]), sexp, w.t)
    assert dx.bands_intact(), "dx: written outside its extent"
    _within(dx.t, want, bound, "dx")
    # the last window ends (H + 2 ph - kh) % sh rows short of the padded map: past the padding, those rows receive no tap
    if (c["H"] + 2 * c["p"][0] - c["k"][0]) % c["s"][0] > c["p"][0]:
        assert bool((dx.t[:, :, -1] == 0).all()), "a row no window reaches must be zero"
    if (c["W"] + 2 * c["p"][1] - c["k"][1]) % c["s"][1] > c["p"][1]:
        assert bool((dx.t[:, :, :, -1] == 0).all()), "a column no window reaches must be zero"
    assert torch.equal(amax.view(torch.int32), dx.t.abs().max().reshape(1).view(torch.int32)), "amax is not max|dx|"
    dx2, amax2 = _Banded(dshape, off), torch.zeros(1, device=DEV)
    _backward(c, gh, gl, sexp, w, dx2, amax2)
    assert torch.equal(dx.buf, dx2.buf) and torch.equal(amax, amax2), "two runs on the same input differ"


def test_the_binding_allocates_checks_and_refuses():
    """``amax = None``; the Python binding allocates what the C ABI takes, refuses shapes that do not belong together and split
    tensors with one scale per image, and hands a refusal of the C ABI to the caller"""
    from laplace_amd._lib import LaplaceHipError, SplitTensor, get_kernels

    K = get_kernels()
    c = next(c for c in df.CASES if c["k"] == (3, 3) and c["s"] == (2, 2) and c["H"] == 8 and c["C"] == 8 and not c["off"])
    x, w, b, g = df.make_inputs(c, torch.Generator().manual_seed(2))
    g = SplitTensor(g.planes.to(DEV), g.sexp.to(DEV))
    y = K.dwconv_forward(x.to(DEV), w.to(DEV), None, c["k"], c["s"], c["p"])
    ref, bound = df.forward_reference(c, x, w, None)
    _within(y, ref, bound, "y")
    dx = K.dwconv_backward(g, w.to(DEV), c["S"], (c["H"], c["W"]), c["k"], c["s"], c["p"])
    want, bound = df.backward_reference(c, g.planes, g.sexp, w)
    _within(dx.reshape(want.shape), want, bound, "dx")
    per_image = SplitTensor(g.planes, g.sexp.expand(g.planes.shape[1]).contiguous())
    with pytest.raises(LaplaceHipError):
        K.dwconv_backward(per_image, w.to(DEV), c["S"], (c["H"], c["W"]), c["k"], c["s"], c["p"])
    if DEV != "cpu":
        with pytest.raises(LaplaceHipError):
            K.dwconv_backward(g, w.to(DEV), c["S"], (c["H"] + 2, c["W"]), c["k"], c["s"], c["p"])
        with pytest.raises(LaplaceHipError, match="amax is one 32-bit device word"):
            K.dwconv_backward(g, w.to(DEV), c["S"], (c["H"], c["W"]), c["k"], c["s"], c["p"], amax=torch.zeros(2, device=DEV))
        with pytest.raises(LaplaceHipError, match="g must be a split tensor"):  # (chunk-major planes are no NHWC map)
            K.dwconv_backward(SplitTensor(g.planes, g.sexp, chunked=True), w.to(DEV), c["S"], (c["H"], c["W"]), c["k"], c["s"], c["p"])
        with pytest.raises(LaplaceHipError):
            K.dwconv_forward(x.to(DEV), w.to(DEV)[:4], None, c["k"], c["s"], c["p"])
        with pytest.raises(LaplaceHipError):
            K.dwconv_forward(x.to(DEV), w.to(DEV), None, c["k"], 9, c["p"])  # (the C ABI's own refusal reaches the caller)


# ---- 2. the depthwise-separable networks, small --------------------------------------------------------------------------------------
def _loader(X, y):
    return DataLoader(TensorDataset(X, y), batch_size=4)


@pytest.fixture(scope="module", params=df.E2E)
def e2e(request):
    """(name, fp64 CPU models, X, y, seeds, fp64 per-tap inputs and cotangents, oracle Jacobians, diagonal and factors) - computed
    once per fixture and left unchanged.  ``m64``: the depthwise weights tracked; ``m64f``: the same network with them frozen."""
    from tests.norm_sweep_fixtures import autograd_reference

    name = request.param
    m64, X, y = df.e2e_fixture(name)
    m64f, _, _ = df.e2e_fixture(name, freeze_depthwise=True)
    seeds = torch.randn(4, X.shape[0], df.E2E_CLASSES, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    f, ins, grads = autograd_reference(m64, df.e2e_taps(m64), X, seeds)
    Js, _ = co.jacobians(m64, X)
    diag = co.ggn_diag(Js, co.functional_hessian(f.detach(), "classification"))
    # (freezing the depthwise weights removes their columns and changes nothing else)
    tracked = {n for n, p in m64f.named_parameters() if p.requires_grad}
    keep = torch.cat([torch.arange(lo, hi) for n, lo, hi in _blocks(m64) if n in tracked])
    Jsf = Js[..., keep]
    loss, kf = None, None
    for i in range(0, X.shape[0], 4):  # (two batches of 4, accumulated as a fit does)
        l_, k_ = co.kfac_ggn(m64f, X[i:i + 4], y[i:i + 4], X.shape[0], "classification")
        loss, kf = (l_, k_) if kf is None else (loss + l_, co.kron_add(kf, k_))
    Qs, ls = co.kron_decompose(kf)
    f_var = co.krondecomposed_inv_square_form_blocks(Qs, ls, PRIOR_PREC, Jsf)  # (the oracle's form without the dense P x P matrix)
    return dict(name=name, m64=m64, m64f=m64f, X=X, y=y, seeds=seeds, f=f.detach(), ins=ins, grads=grads, Js=Js, diag=diag,
                loss=loss, kf=kf, f_var=f_var)


def _split_sweeps(b):
    """the sweeps the backend built: each of them must be a ``SplitSweep`` that took the NHWC walk"""
    from laplace_amd.sweep_nhwc import SplitSweep

    tape = b._tape()
    sweeps = [s for s in tape.sweeps.values() if s]
    assert sweeps, getattr(tape, "sweep_reason", None)
    for s in sweeps:
        assert isinstance(s, SplitSweep) and s.split_reason is None, getattr(s, "split_reason", None)
    return sweeps


def test_e2e_taps_of_the_split_sweep_against_float64_autograd(e2e):
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep_nhwc import SplitSweep

    model = copy.deepcopy(e2e["m64"]).float().to(DEV)
    taps = df.e2e_taps(model)
    sw = SplitSweep(model, taps, kernels=get_kernels)
    assert isinstance(sw, SplitSweep) and sw.split_reason is None, sw.split_reason
    f = sw.forward(e2e["X"].float().to(DEV))
    grads = sw.backward(e2e["seeds"].float().to(DEV))
    check(f, e2e["f"], what="f")
    for n in taps:
        check(sw.taps[n]["a"], e2e["ins"][n], what=f"{n}: a")
        assert tuple(grads[n].shape) == tuple(e2e["grads"][n].shape), n
        check(grads[n], e2e["grads"][n], what=f"{n}: cotangent")


def _blocks(model):
    """(name, first column, one past the last) of every tracked parameter in the order of the Jacobian's columns"""
    out, at = [], 0
    for n, p in model.named_parameters():
        if p.requires_grad:
            out.append((n, at, at + p.numel()))
            at += p.numel()
    return out


def test_e2e_jacobians_and_diag_with_the_depthwise_weights_tracked(e2e):
    from laplace_amd import HipGGN

    model = copy.deepcopy(e2e["m64"]).float().to(DEV)
    Xd, yd = e2e["X"].float().to(DEV), e2e["y"].to(DEV)
    b = HipGGN(model, "classification")
    Js, f, h = _in_two_batches(b, Xd, yd)
    _split_sweeps(b)
    check(f, e2e["f"], what="f")
    for n, lo, hi in _blocks(model):
        check(Js[..., lo:hi], e2e["Js"][..., lo:hi], what=f"jacobians: {n}")
        check(h[lo:hi], e2e["diag"][lo:hi], what=f"diag: {n}")


def _in_two_batches(b, Xd, yd):
    """``(Js, f, diagonal)`` over two batches of 4, the diagonal summed as a fit does"""
    parts = [(*b.jacobians(Xd[i:i + 4]), b.diag(Xd[i:i + 4], yd[i:i + 4])[1]) for i in range(0, Xd.shape[0], 4)]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), sum(p[2] for p in parts)


def _factors(kron, kf_ref, what):
    for i, (F_, G_) in enumerate(zip(kron.kfacs, kf_ref)):
        for j, (a, ref) in enumerate(zip(F_, G_)):
            check(a, ref, what=f"{what}: block {i} factor {j}")


def test_e2e_kron_and_the_predictive_with_the_depthwise_weights_frozen(e2e):
    from laplace_amd import HipGGN
    from laplace_amd.laplace import HipLaplace

    model = copy.deepcopy(e2e["m64f"]).float().to(DEV)
    Xd, yd = e2e["X"].float().to(DEV), e2e["y"].to(DEV)
    b = HipGGN(model, "classification")
    loss, kron = b.kron(Xd[:4], yd[:4], N=Xd.shape[0])
    loss2, kron2 = b.kron(Xd[4:], yd[4:], N=Xd.shape[0])
    _split_sweeps(b)
    check(loss + loss2, e2e["loss"], what="loss")
    _factors(kron + kron2, e2e["kf"], "kron")
    la = HipLaplace(model, "classification", "all", "kron", prior_precision=PRIOR_PREC)
    la.fit(_loader(Xd, yd))
    _split_sweeps(la.backend)
    _, f_var = la._glm_predictive_distribution(Xd)
    check(f_var, e2e["f_var"], what="Kron GLM predictive variance")


def test_e2e_kron_refuses_a_tracked_depthwise_layer_by_name(e2e):
    from laplace_amd import HipGGN

    model = copy.deepcopy(e2e["m64"]).float().to(DEV)
    first = df.depthwise_names(model)[0]
    with pytest.raises(NotImplementedError, match=rf"^{first}: KFAC has no rule for a grouped convolution"):
        HipGGN(model, "classification").kron(e2e["X"][:4].float().to(DEV), e2e["y"][:4].to(DEV), N=8)


def test_the_switch_gives_the_default_results(e2e, monkeypatch):
    """``SplitSweep.nhwc_depthwise = False`` (the NCHW sweep, the route of these models before lk_dwconv.hip) against the same
    oracle at the same tolerance as the default route above"""
    from laplace_amd import HipGGN
    from laplace_amd.sweep_nhwc import SplitSweep

    model = copy.deepcopy(e2e["m64"]).float().to(DEV)
    Xd, yd = e2e["X"].float().to(DEV), e2e["y"].to(DEV)
    b = HipGGN(model, "classification")
    Js, _, _ = _in_two_batches(b, Xd, yd)
    _split_sweeps(b)
    monkeypatch.setattr(SplitSweep, "nhwc_depthwise", False)
    old = HipGGN(copy.deepcopy(e2e["m64"]).float().to(DEV), "classification")
    Js_old, f_old, h_old = _in_two_batches(old, Xd, yd)
    sweep = old._tape().sweeps[frozenset({"gconv"})]
    assert isinstance(sweep, SplitSweep) and not sweep.split_ok and "foreign to the NHWC kernels" in sweep.split_reason
    check(f_old, e2e["f"], what="f (nhwc_depthwise = False)")
    for n, lo, hi in _blocks(model):
        check(Js_old[..., lo:hi], e2e["Js"][..., lo:hi], what=f"jacobians (nhwc_depthwise = False): {n}")
        check(h_old[lo:hi], e2e["diag"][lo:hi], what=f"diag (nhwc_depthwise = False): {n}")
        check(Js[..., lo:hi], Js_old[..., lo:hi], what=f"jacobians, default against the switch: {n}")
