"""GroupNorm and LayerNorm in the seed-batched reverse sweep, on the device (-m gpu): the forward and VJP kernels alone
(csrc/lk_normvjp.hip through the C ABI) against float64 evaluated from the same fp32 inputs, and the sweeps, ``HipGGN`` and the
Kron predictive on models with these layers against float64 autograd, the goldens of the unmodified reference and the oracle.

The kernel bounds hold for ANY summation order.  With u = 2^-24, A = mean_row|x|, dmu = (N + 2) u A:
    |d xhat| <= rstd dmu + 2 u rstd |x - mu| + |xhat| ((N/2 + 8) u + (rstd dmu)^2 / 2)
    |d rstd| <= rstd ((N/2 + 8) u + (rstd dmu)^2 / 2)
    |d y|    <= |w| bound(xhat) + u (2 |w xhat| + |y|)
    |d dx|   <= u rstd (4 |t| + (N + 6) mean_row|t| + (N + 8) |xhat| mean_row|t xhat|)
(tests/norm_sweep_fixtures.py states them in code; tests/test_norm_sweep_fixtures.py shows on the CPU that fp32 two-pass forms sit
below them and ``E[x^2] - mu^2`` far above).  The shape table is tests/norm_sweep_fixtures.CASES; the same CPU file proves that it
reaches every launch variant.  ``LK_TEST_DEVICE=cpu`` rehearses this file's host logic on the kernel emulation.
"""
import copy
import ctypes
import os

import pytest
import torch
from torch import nn
from torch.utils.data import DataLoader, TensorDataset

from oracle import curvature_oracle as co
from tests import norm_sweep_fixtures as nf
from tests.norm_fixtures import golden_model, load_golden, rel

pytestmark = pytest.mark.gpu
DEV = os.environ.get("LK_TEST_DEVICE", "cuda")
PAD, FILL, EPS = 64, 7.5, 1e-5


@pytest.fixture(autouse=True, scope="module")
def _kernels():
    if DEV != "cpu":
        yield
        return
    from laplace_amd import _lib
    from tests.emulated_normvjp_kernels import EmulatedNormVjpKernels

    prev = _lib.set_kernels_for_testing(EmulatedNormVjpKernels())
    yield
    _lib.set_kernels_for_testing(prev)


# ---- 1. the kernels alone ---------------------------------------------------------------------------------------------------------
class _Banded:
    """``numel`` floats inside guard bands of ``PAD`` floats; ``off``: the interior starts one float past a 16-byte boundary"""

    def __init__(self, shape, off, init=None):
        n = 1
        for d in shape:
            n *= d
        self.buf = torch.full((2 * PAD + n + 4,), FILL, device=DEV)
        self.lo, self.hi = PAD + off, PAD + off + n
        self.t = self.buf[self.lo:self.hi].view(*shape)
        if init is not None:
            self.t.copy_(init)

    def bands_intact(self):
        return bool((self.buf[:self.lo] == FILL).all()) and bool((self.buf[self.hi:] == FILL).all())


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _forward(c, x, w, b, y, xhat, rstd):
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    if DEV == "cpu":
        for dst, src in zip((y, xhat, rstd), K.norm_forward(x.t, w, b, c["G"], c["layout"], EPS)):
            dst.t.copy_(src)
        return
    rc = K.lib.lk_norm_fwd_f32(_p(x.t), _p(w), _p(b), c["B"], c["L"], c["Ch"], c["G"], c["layout"], EPS, _p(y.t), _p(xhat.t),
                               _p(rstd.t), K._stream(x.t.device))
    assert rc == 0, K.lib.lk_last_error()


def _vjp(c, g, xhat, rstd, w, dx, amax):
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    if DEV == "cpu":
        dx.t.copy_(K.norm_vjp(g.t.reshape(c["S"] * c["B"], *g.t.shape[2:]), xhat.t, rstd.t, w, c["S"], c["G"], c["layout"],
                              amax=amax).reshape(dx.t.shape))
        return
    rc = K.lib.lk_norm_vjp_f32(_p(g.t), _p(xhat.t), _p(rstd.t), _p(w), c["S"], c["B"], c["L"], c["Ch"], c["G"], c["layout"],
                               _p(dx.t), _p(amax), K._stream(g.t.device))
    assert rc == 0, K.lib.lk_last_error()


def _ratio(got, want, bound):
    err = (got.double() - want).abs()
    return (err / bound.clamp_min(1e-300)).max().item(), (err - bound).max().item()


@pytest.mark.parametrize("c", nf.CASES, ids=nf.case_id)
def test_kernels_against_float64(c):
    """forward on inputs with mean 100 and unit spread, then the VJP on the forward's own fp32 ``xhat`` and ``rstd``: every
    element within its bound; the guard bands around ``y``, ``xhat``, ``rstd`` and ``dx`` keep their fill; ``amax`` is
    ``max|dx|`` bit for bit; a second run gives the same bits."""
    gen = torch.Generator(device=DEV).manual_seed(c["S"] + 10 * c["B"] + 1000 * c["L"] + 7 * c["Ch"] + c["G"])
    shape, off, G, layout = nf.shape_of(c), c["off"], c["G"], c["layout"]
    x = _Banded(shape, off, torch.randn(*shape, generator=gen, device=DEV) + 100.0)
    w, b = nf.make_affine(c, gen, DEV)
    y, xhat, rstd = _Banded(shape, off), _Banded(shape, off), _Banded((c["B"], G), off)
    _forward(c, x, w, b, y, xhat, rstd)
    ref = nf.forward_reference(x.t, w, b, c, EPS)
    worst = {}
    for name, got in (("y", y), ("xhat", xhat)):
        worst[name], excess = _ratio(nf.to_rows(got.t, G, layout), ref[name], ref["b_" + name])
        assert excess <= 0.0, f"{name}: error exceeds the bound by {excess:.3e} ({worst[name]:.3f} of it)"
        assert got.bands_intact(), f"{name}: written outside its extent"
    worst["rstd"], excess = _ratio(rstd.t.reshape(c["B"], G, 1), ref["rstd"], ref["b_rstd"])
    assert excess <= 0.0, f"rstd: error exceeds the bound by {excess:.3e} ({worst['rstd']:.3f} of it)"
    assert rstd.bands_intact()

    g = _Banded((c["S"],) + shape, off, torch.randn(c["S"], *shape, generator=gen, device=DEV))
    dx, amax = _Banded((c["S"],) + shape, off), torch.zeros(1, device=DEV)
    _vjp(c, g, xhat, rstd, w, dx, amax)
    want, bound = nf.vjp_reference(g.t, xhat.t, rstd.t, w, c)
    worst["dx"], excess = _ratio(nf.to_rows(dx.t, G, layout), want, bound)
    print(f"{nf.case_id(c)}: worst |err| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert excess <= 0.0, f"dx: error exceeds the bound by {excess:.3e} ({worst['dx']:.3f} of it)"
    assert dx.bands_intact(), "dx: written outside its extent"
    assert torch.equal(amax.view(torch.int32), dx.t.abs().max().reshape(1).view(torch.int32)), "amax is not max|dx|"
    dx2, amax2 = _Banded((c["S"],) + shape, off), torch.zeros(1, device=DEV)
    _vjp(c, g, xhat, rstd, w, dx2, amax2)
    assert torch.equal(dx.buf, dx2.buf) and torch.equal(amax, amax2), "two runs on the same input differ"


def test_vjp_without_an_amax_word_and_the_binding():
    """``amax = null``; the Python binding allocates what the C ABI takes"""
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    c = dict(S=3, B=2, L=16, Ch=64, G=32, layout=1, w="rand", off=0)
    gen = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(*nf.shape_of(c), generator=gen, device=DEV)
    w, b = nf.make_affine(c, gen, DEV)
    y, xhat, rstd = K.norm_forward(x, w, b, 32, 1, EPS)
    g = torch.randn(3 * 2, 16, 64, generator=gen, device=DEV)
    dx = K.norm_vjp(g, xhat, rstd, w, 3, 32, 1)
    want, bound = nf.vjp_reference(g.reshape(3, 2, 16, 64), xhat, rstd, w, c)
    assert _ratio(nf.to_rows(dx.reshape(3, 2, 16, 64), 32, 1), want, bound)[1] <= 0.0
    assert rel(y, torch.nn.functional.group_norm(x.movedim(-1, 1).double(), 32, w.double(), b.double(), EPS).movedim(1, -1)) < 1e-5
    if DEV != "cpu":
        from laplace_amd._lib import LaplaceHipError

        with pytest.raises(LaplaceHipError, match="amax is one 32-bit device word"):
            K.norm_vjp(g, xhat, rstd, w, 3, 32, 1, amax=torch.zeros(2, device=DEV))


# ---- 2. the backend against the goldens of the reference --------------------------------------------------------------------------
def check(got, want, tol=1e-4, what=""):
    e = rel(got, want)
    print(f"{what}: {e:.3e}")
    assert e < tol, f"{what}: rel err {e:.3e}"


@pytest.mark.parametrize("lik", ("classification", "regression"))
@pytest.mark.parametrize("name", ("normgn", "normln"))
def test_backend_on_the_sweep_against_reference_golden(monkeypatch, name, lik):
    from laplace_amd import HipGGN
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep import SeedBatchedSweep

    K, calls = get_kernels(), []
    inner = K.norm_vjp
    monkeypatch.setattr(K, "norm_vjp", lambda *a, **kw: (calls.append(1), inner(*a, **kw))[1], raising=False)
    real, passes = torch.autograd.grad, []
    g = load_golden(name, lik)
    model, X, y = golden_model(name, g, device=DEV)
    b = HipGGN(model, lik)
    monkeypatch.setattr(torch.autograd, "grad", lambda *a, **kw: (passes.append(1), real(*a, **kw))[1])
    Js, f = b.jacobians(X)
    loss, h = b.diag(X, y)
    monkeypatch.setattr(torch.autograd, "grad", real)
    tape = b._tape()
    # the route: the seed-batched sweep with the norm layers tapped, one VJP launch per norm node and call, no autograd pass
    assert isinstance(tape.sweeps.get(frozenset({"norm"})), SeedBatchedSweep), getattr(tape, "sweep_reason", None)
    assert len(calls) == 2 and not passes, (calls, passes)
    check(Js, g["Js"], what="jacobians")
    check(f, g["f"], what="f")
    check(h, g["h_ggn"], what="diag GGN")
    check(loss, g["loss"], what="loss")


# ---- 3. a small ResNet with GroupNorm -----------------------------------------------------------------------------------------------
class _GNResNet(nn.Module):
    def __init__(self, act=torch.tanh):
        super().__init__()
        from laplace_amd.nets import BasicBlock

        self.act = act
        self.conv1 = nn.Conv2d(3, 32, 3, 1, 1, bias=False)
        self.bn1 = nn.GroupNorm(32, 32)
        self.layers = nn.Sequential(BasicBlock(32, 32, 1, act, "gn"), BasicBlock(32, 64, 2, act, "gn"))
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(64, 5)

    def forward(self, x):
        x = self.act(self.bn1(self.conv1(x)))
        return self.fc(torch.flatten(self.pool(self.layers(x)), 1))


def _gn_resnet_reference(seed, act=torch.tanh):
    torch.manual_seed(seed)
    m64 = _GNResNet(act).double().eval()
    for mod in m64.modules():
        if isinstance(mod, nn.GroupNorm):
            mod.weight.data.uniform_(0.5, 1.5), mod.bias.data.normal_(0.0, 0.2)
            mod.weight.requires_grad_(False), mod.bias.requires_grad_(False)
    X, y, seeds = torch.randn(4, 3, 8, 8, dtype=torch.float64), torch.randint(5, (4,)), torch.randn(4, 4, 5, dtype=torch.float64)
    taps = {n: m for n, m in m64.named_modules() if isinstance(m, (nn.Conv2d, nn.Linear))}
    f, ins, grads = nf.autograd_reference(m64, taps, X, seeds)
    return m64, X, y, seeds, f.detach(), ins, grads


@pytest.fixture(scope="module")
def gn_resnet():
    """(fp64 CPU model, X, y, seeds, fp64 per-tap inputs and cotangents) - computed once"""
    return _gn_resnet_reference(5)


RELU_MARGIN = 1e-5  # fp32 moves a pre-activation of this net (values of order 1) by a few 1e-7: none can change sides


@pytest.fixture(scope="module")
def gn_relu_resnet():
    """the same net with ReLU behind every GroupNorm, as ``ResNet18(norm="gn")`` has it: the mask is a bool over an NCHW-logical
    view of NHWC memory and the next convolution splits its input itself.  A ReLU mask is a step function of the
    pre-activation, so a per-element comparison of two separately executed passes needs every float64 pre-activation
    to stay clear of zero; the reference is checked for that (it is a property of the seed, not of the code under test)."""
    margin = [float("inf")]

    def noting_relu(z):
        margin[0] = min(margin[0], z.detach().abs().min().item())
        return torch.relu(z)

    ref = _gn_resnet_reference(6, noting_relu)
    assert margin[0] > RELU_MARGIN, f"a float64 pre-activation lies {margin[0]:.2e} from zero: take another seed"
    for mod in ref[0].modules():  # (the sweeps trace the stock function)
        if getattr(mod, "act", None) is noting_relu:
            mod.act = torch.relu
    return ref


@pytest.mark.parametrize("split", (False, True))
def test_gn_resnet_taps_of_both_sweeps_against_float64_autograd(gn_resnet, split):
    _taps_of_both_sweeps(gn_resnet, split)


@pytest.mark.parametrize("split", (False, True))
def test_gn_relu_resnet_taps_of_both_sweeps_against_float64_autograd(gn_relu_resnet, split):
    _taps_of_both_sweeps(gn_relu_resnet, split)


def _taps_of_both_sweeps(reference, split):
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep import SeedBatchedSweep
    from laplace_amd.sweep_nhwc import SplitSweep

    m64, X, y, seeds, f64, ins, want = reference
    model = copy.deepcopy(m64).float().to(DEV)
    taps = {n: m for n, m in model.named_modules() if isinstance(m, (nn.Conv2d, nn.Linear))}
    sw = (SplitSweep if split else SeedBatchedSweep)(model, taps, kernels=get_kernels)
    if split:
        assert sw.split_ok, sw.split_reason
    f = sw.forward(X.float().to(DEV))
    grads = sw.backward(seeds.float().to(DEV))
    check(f, f64, what="f")
    for n in taps:
        check(sw.taps[n]["a"], ins[n], what=f"{n}: a")
        assert tuple(grads[n].shape) == tuple(want[n].shape), n
        check(grads[n], want[n], what=f"{n}: cotangent")


def test_gn_resnet_kron_and_predictive_against_the_oracle(gn_resnet):
    from laplace_amd import HipGGN
    from laplace_amd.laplace import HipLaplace
    from laplace_amd.sweep_nhwc import SplitSweep

    m64, X, y, _, _, _, _ = gn_resnet
    model = copy.deepcopy(m64).float().to(DEV)
    Xd, yd = X.float().to(DEV), y.to(DEV)
    b = HipGGN(model, "classification")
    loss, kron = b.kron(Xd, yd, N=4)
    sweep = b._tape().sweep
    assert isinstance(sweep, SplitSweep) and sweep.split_ok, getattr(sweep, "split_reason", None)
    loss_ref, kf_ref = co.kfac_ggn(m64, X, y, 4, "classification")
    check(loss, loss_ref, what="loss")
    for i, (F_, G_) in enumerate(zip(kron.kfacs, kf_ref)):
        for j, (a, ref) in enumerate(zip(F_, G_)):
            err = (a.double().cpu() - ref).abs()
            rel(a, ref)  # (recorded in the parity log)
            excess = (err - (1e-4 * ref.abs() + 1e-6 * ref.abs().max())).max().item()
            assert excess <= 0.0, f"factor {i}.{j}: exceeds 1e-4 |b| + 1e-6 max|b| by {excess:.3e}"
    la = HipLaplace(model, "classification", "all", "kron", prior_precision=0.5)
    la.fit(DataLoader(TensorDataset(Xd, yd), batch_size=4))
    _, f_var = la._glm_predictive_distribution(Xd)
    Qs, ls = co.kron_decompose(kf_ref)
    check(f_var, co.functional_variance_kron(co.jacobians(m64, X)[0], Qs, ls, 0.5), what="Kron GLM predictive variance")
