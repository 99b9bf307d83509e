"""Parameters of BatchNorm / LayerNorm / GroupNorm layers on the device (-m gpu): the norm kernel alone (csrc/lk_norm.hip
through the C ABI), the backend and the Laplace classes against the goldens of the unmodified reference
(tools/make_norm_golden.py), the route check, and a ResNet-18 with unfrozen BatchNorm.

Tolerance of the golden comparisons: 1e-4 max-normalised (BASELINE.json north_star), as every golden test here.
``LK_TEST_DEVICE=cpu`` rehearses this file's host logic on the kernel emulation, as tests/test_gpu_backend.py does.
"""
import os

import pytest
import torch
from torch import nn
from torch.utils.data import DataLoader, TensorDataset

from oracle.make_golden import PRIOR_PREC, SIGMA_NOISE
from tests.norm_fixtures import NORM_FIXTURES, ef_gradients_from_golden, golden_model, load_golden, rel, route_check

pytestmark = pytest.mark.gpu
DEV = os.environ.get("LK_TEST_DEVICE", "cuda")
LIKS = ("classification", "regression")
CASES = [(n, l) for n in NORM_FIXTURES for l in LIKS]


@pytest.fixture(autouse=True, scope="module")
def _kernels():
    if DEV != "cpu":
        yield
        return
    from laplace_amd import _lib
    from tests.emulated_norm_kernels import EmulatedNormKernels

    prev = _lib.set_kernels_for_testing(EmulatedNormKernels())
    yield
    _lib.set_kernels_for_testing(prev)


def check(got, want, tol=1e-4, what=""):
    e = rel(got, want)
    print(f"{what}: {e:.3e}")
    assert e < tol, f"{what}: rel err {e:.3e}"


# ---- 1. the kernel alone ----------------------------------------------------------------------------------------------
# (S, B, Ch, L): L in {1, 4, 49, 1024}, Ch in {3, 8, 64, 100, 512}, S in {1, 9}, B in {1, 10, 128}; the largest cotangent is the
# 302 MB of the c4 network's 64-channel 32 x 32 layers; Ch not a multiple of 4 and S * B = 1 included
KERNEL_SHAPES = [
    (1, 1, 3, 1024), (1, 1, 8, 1), (1, 1, 100, 49), (9, 1, 64, 1024), (9, 10, 3, 4), (9, 10, 100, 49), (1, 10, 512, 4),
    (9, 10, 512, 4), (1, 10, 100, 1024), (9, 128, 512, 1), (1, 128, 8, 49), (9, 128, 8, 4), (1, 128, 64, 1), (9, 10, 64, 49),
    (9, 128, 64, 1024),
]


def _kernel_case(S, B, Ch, L, layout, cols):
    """runs the kernel on seeded inputs; returns (Js, float64 reference block, bound, column map)"""
    from laplace_amd._lib import get_kernels

    gen = torch.Generator(device=DEV).manual_seed(1000 * L + 10 * Ch + S + B)
    shape = (B, Ch, L) if layout == 0 else (B, L, Ch)
    g = torch.randn(S, *shape, generator=gen, device=DEV)
    xhat = torch.randn(*shape, generator=gen, device=DEV)
    P = 2 * Ch + 7
    wcol0 = 3 if "w" in cols else -1
    bcol0 = (Ch + 5 if "w" in cols else 2) if "b" in cols else -1
    Js = torch.full((B, S, P), 7.5, device=DEV)
    get_kernels().jac_norm_affine(g, xhat, Ch, layout, Js, wcol0, bcol0)
    red = 2 if layout == 0 else 1  # the reduced dim of xhat
    bounds, wants = {}, {}
    eps = (L + 2) * 2.0 ** -24
    # per seed, so that the float64 copies stay the size of one seed's cotangent
    want_w = torch.empty(B, S, Ch, dtype=torch.float64, device=DEV)
    want_b, bnd_w, bnd_b = torch.empty_like(want_w), torch.empty_like(want_w), torch.empty_like(want_w)
    x64 = xhat.double()
    for s in range(S):
        g64 = g[s].double()
        prod = g64 * x64
        want_w[:, s], bnd_w[:, s] = prod.sum(red), prod.abs().sum(red) * eps
        want_b[:, s], bnd_b[:, s] = g64.sum(red), g64.abs().sum(red) * eps
    if wcol0 >= 0:
        wants[wcol0], bounds[wcol0] = want_w, bnd_w
    if bcol0 >= 0:
        wants[bcol0], bounds[bcol0] = want_b, bnd_b
    return g, xhat, Js, wants, bounds, (wcol0, bcol0)


@pytest.mark.parametrize("layout", (0, 1))
@pytest.mark.parametrize("S,B,Ch,L", KERNEL_SHAPES)
def test_norm_kernel_against_float64(S, B, Ch, L, layout):
    """every output within ``(L + 2) * 2^-24 * sum_l |g_l * xhat_l|`` of a float64 evaluation of the same inputs - the fp32
    bound of a length-L dot product that holds for ANY summation order (bias columns: ``xhat = 1``); the other columns of
    ``Js`` keep what they held; a second run gives the same bits."""
    from laplace_amd._lib import get_kernels

    g, xhat, Js, wants, bounds, (wcol0, bcol0) = _kernel_case(S, B, Ch, L, layout, "wb")
    touched = torch.zeros(Js.shape[-1], dtype=torch.bool, device=DEV)
    for col0, want in wants.items():
        got = Js[:, :, col0:col0 + Ch].double()
        excess = ((got - want).abs() - bounds[col0]).max().item()
        ratio = ((got - want).abs() / bounds[col0].clamp_min(1e-300)).max().item()
        print(f"S={S} B={B} Ch={Ch} L={L} layout={layout} col0={col0}: worst |err| / bound = {ratio:.3f}")
        assert excess <= 0.0, f"column block at {col0}: error exceeds the bound by {excess:.3e} (ratio {ratio:.3f})"
        touched[col0:col0 + Ch] = True
    assert bool((Js[:, :, ~touched] == 7.5).all()), "columns outside the layer's were written"
    again = torch.full_like(Js, 7.5)
    get_kernels().jac_norm_affine(g, xhat, Ch, layout, again, wcol0, bcol0)
    assert torch.equal(Js, again), "two runs on the same input differ"


@pytest.mark.parametrize("cols", ("w", "b"))
@pytest.mark.parametrize("layout", (0, 1))
@pytest.mark.parametrize("S,B,Ch,L", [(9, 10, 100, 49), (1, 1, 8, 1), (9, 10, 64, 1024)])
def test_norm_kernel_weight_only_and_bias_only(S, B, Ch, L, layout, cols):
    g, xhat, Js, wants, bounds, _ = _kernel_case(S, B, Ch, L, layout, cols)
    assert len(wants) == 1
    (col0, want), = wants.items()
    got = Js[:, :, col0:col0 + Ch].double()
    assert ((got - want).abs() - bounds[col0]).max().item() <= 0.0
    keep = torch.ones(Js.shape[-1], dtype=torch.bool, device=DEV)
    keep[col0:col0 + Ch] = False
    assert bool((Js[:, :, keep] == 7.5).all()), "columns outside the requested block were written"


# ---- 2. the backend against the goldens -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lik", CASES)
def test_ggn_against_reference_golden(name, lik):
    from laplace_amd import HipGGN

    g = load_golden(name, lik)
    model, X, y = golden_model(name, g, device=DEV)
    b = HipGGN(model, lik)
    assert b._supported()
    Js, f = b.jacobians(X)
    check(Js, g["Js"], what="jacobians")
    check(f, g["f"], what="f")
    loss, H = b.full(X, y)
    check(H, g["H_ggn"], what="full GGN")
    check(loss, g["loss"], what="loss")
    loss, h = b.diag(X, y)
    check(h, g["h_ggn"], what="diag GGN")
    check(loss, g["loss"], what="loss")
    h2 = b.diag(X[:5], y[:5])[1] + b.diag(X[5:], y[5:])[1]
    check(h2, g["h_ggn"], what="diag additivity")


@pytest.mark.parametrize("name,lik", CASES)
def test_ef_against_reference_golden(name, lik):
    from laplace_amd import HipEF

    g = load_golden(name, lik)
    model, X, y = golden_model(name, g, device=DEV)
    b = HipEF(model, lik)
    assert b._supported()
    loss, H = b.full(X, y)
    check(H, g["H_ef"], what="full EF")
    check(loss, g["loss_ef"], what="EF loss")
    check(b.diag(X, y)[1], g["h_ef"], what="diag EF")
    Gs, _ = b.gradients(X, y)
    check(Gs, ef_gradients_from_golden(g, lik), what="EF gradients")


# ---- 3. the Laplace classes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hs", ("diag", "full"))
@pytest.mark.parametrize("name,lik", CASES)
def test_laplace_all_against_reference_golden(name, lik, hs):
    from laplace_amd.laplace import HipLaplace

    g = load_golden(name, lik)
    model, X, y = golden_model(name, g, device=DEV)
    la = HipLaplace(model, lik, "all", hs, prior_precision=PRIOR_PREC,
                    sigma_noise=SIGMA_NOISE if lik == "regression" else 1.0)
    la.fit(DataLoader(TensorDataset(X, y), batch_size=5))
    tag = f"la.all.{hs}"
    check(la.loss, g[f"{tag}.loss"], what="loss")
    check(la.H, g[f"{tag}.H"], what="accumulated H")
    f_mu, f_var = la._glm_predictive_distribution(X)
    check(f_mu, g[f"{tag}.f_mu"], what="f_mu")
    check(f_var, g[f"{tag}.f_var"], what="f_var")
    check(la.log_marginal_likelihood(), g[f"{tag}.marglik"], what="marglik")


def test_route_check_generic_route_forbidden(monkeypatch):
    """fails on a backend without the norm route: there every one of these calls goes through ``jacrev`` / ``grad``"""
    route_check(monkeypatch, DEV)


# ---- 4. ResNet-18 with unfrozen BatchNorm -------------------------------------------------------------------------------
def test_resnet18_unfrozen_batchnorm_diag_against_its_own_jacobians():
    """``diag(X, y)[1]`` against ``sum_n diag(J_n^T Lambda_n J_n)`` formed in float64 on the host from ``jacobians(X)``, for
    ALL normalisation columns and a seeded sample of 4 096 others (tanh: see the docstring of nets.ResNet18)."""
    from laplace_amd import HipGGN
    from laplace_amd.nets import ResNet18
    from laplace_amd.sweep_nhwc import SplitSweep

    torch.manual_seed(11)
    model = ResNet18(freeze_bn=False, act=torch.tanh)
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0.0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0.0, 0.1)
    model = model.to(DEV).eval()
    nb = 1 if DEV == "cpu" else 4
    X = torch.randn(nb, 3, 32, 32, device=DEV)
    y = torch.randint(10, (nb,), device=DEV)
    b = HipGGN(model, "classification")
    tape = b._tape()
    assert len(tape.norm_taps) == 20 and not tape.unserved and b._supported()
    norm_cols = torch.cat([torch.arange(o, o + t.module.num_features) for t in tape.norm_taps for o in (t.w_off, t.b_off)])
    assert norm_cols.numel() == 9600
    gen = torch.Generator().manual_seed(5)
    is_norm = torch.zeros(tape.n_params, dtype=torch.bool)
    is_norm[norm_cols] = True
    others = torch.nonzero(~is_norm).flatten()
    other_cols = others[torch.randperm(others.numel(), generator=gen)[:4096]]

    _, h = b.diag(X, y)
    sweep = tape.sweeps[frozenset({"norm"})]
    # which sweep served the model: the NCHW rules of the parent class (a tapped BatchNorm makes the split sweep ineligible)
    assert isinstance(sweep, SplitSweep) and not sweep.split_ok and "tapped BatchNorm" in sweep.split_reason
    print(f"sweep: {type(sweep).__name__}, split_ok={sweep.split_ok}, split_reason={sweep.split_reason!r}")
    Js, f = b.jacobians(X)
    assert Js.shape == (nb, 10, tape.n_params)
    p = torch.softmax(f.double().cpu(), -1)
    Lam = torch.diag_embed(p) - p[:, :, None] * p[:, None, :]
    for what, cols in (("norm columns", norm_cols), ("other columns", other_cols)):
        J = Js[:, :, cols.to(Js.device)].double().cpu()
        want = torch.einsum("ncp,nck,nkp->p", J, Lam, J)
        check(h[cols.to(h.device)], want, what=f"diag of {what}")
