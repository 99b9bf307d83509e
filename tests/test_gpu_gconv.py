"""Weights of grouped / depthwise convolutions on the device (-m gpu): the kernel alone (csrc/lk_gconv.hip through the C
ABI), the backend and the Laplace classes against the goldens of the unmodified reference (tools/make_gconv_golden.py), the
route check, and a reduced-width MobileNetV2-style network.

Tolerance of the golden comparisons: 1e-4 max-normalised (BASELINE.json north_star), as every golden test here.
``LK_TEST_DEVICE=cpu`` rehearses this file's host logic on the kernel emulation, as tests/test_gpu_backend.py does.
"""
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn
from torch.utils.data import DataLoader, TensorDataset

from oracle.make_golden import PRIOR_PREC, SIGMA_NOISE
from tests.gconv_fixtures import GCONV_FIXTURES, ef_gradients_from_golden, golden_model, load_golden, rel, route_check

pytestmark = pytest.mark.gpu
DEV = os.environ.get("LK_TEST_DEVICE", "cuda")
LIKS = ("classification", "regression")
CASES = [(n, l) for n in GCONV_FIXTURES for l in LIKS]


@pytest.fixture(autouse=True, scope="module")
def _kernels():
    if DEV != "cpu":
        yield
        return
    from laplace_amd import _lib
    from tests.emulated_gconv_kernels import EmulatedGConvKernels

    prev = _lib.set_kernels_for_testing(EmulatedGConvKernels())
    yield
    _lib.set_kernels_for_testing(prev)


def check(got, want, tol=1e-4, what=""):
    e = rel(got, want)
    print(f"{what}: {e:.3e}")
    assert e < tol, f"{what}: rel err {e:.3e}"


# ---- 1. the kernel alone ----------------------------------------------------------------------------------------------
# (S, B, Cin, groups, Do, H, W, k, stride, pad, dil)
KERNEL_SHAPES = [
    (1, 1, 3, 3, 3, 5, 5, 3, 1, 1, 1),
    (9, 10, 4, 4, 8, 7, 7, 3, 2, 1, 1),          # depthwise, channel multiplier 2, stride 2
    (3, 2, 5, 5, 5, 9, 9, 7, 1, 3, 1),           # 49 taps
    (2, 3, 4, 4, 4, 8, 6, 5, 2, 2, 1),           # 25 taps, stride 2, rectangular map
    (1, 2, 2, 2, 2, 33, 33, 3, 1, 1, 1),         # L = 1089 crosses any tile
    (9, 4, 100, 100, 100, 4, 4, 3, 1, 1, 1),     # 16-byte loads (OW = 4)
    (1, 1, 8, 8, 8, 1, 1, 1, 1, 0, 1),           # L = 1
    (2, 3, 6, 2, 4, 6, 6, 3, 1, 2, 2),           # two groups, dilated: the tile path
    (9, 2, 32, 4, 32, 6, 6, 3, 1, 1, 1),         # Dkg = 72
    (2, 2, 64, 2, 64, 5, 5, 3, 1, 1, 1),         # Dkg = 288
    (3, 2, 6, 3, 6, 5, 7, (1, 3), (2, 1), (0, 1), 1),
    (2, 2, 6, 1, 4, 5, 5, 3, 1, 1, 1),           # groups = 1: the contract of lk_jac_conv_f32
    (9, 128, 64, 64, 64, 16, 16, 3, 1, 1, 1),    # the largest case
]
_CASE_CACHE = {}


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _kernel_inputs(shape):
    """seeded inputs and, computed once per shape, the float64 value and the bound of every weight / bias entry"""
    if shape in _CASE_CACHE:
        return _CASE_CACHE[shape]
    _CASE_CACHE.clear()  # (one shape's tensors at a time)
    S, B, Cin, groups, Do, H, W, k, st, pd, dl = shape
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = _pair(k), _pair(st), _pair(pd), _pair(dl)
    OH = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1
    OW = (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    L, Cig, Dog = OH * OW, Cin // groups, Do // groups
    Dkg = Cig * kh * kw
    gen = torch.Generator(device=DEV).manual_seed(1000 * H + 10 * Do + S + B)
    x = torch.randn(B, Cin, H, W, generator=gen, device=DEV)
    g = torch.randn(S, B, Do, OH, OW, generator=gen, device=DEV)
    eps = (L + 2) * 2.0 ** -24
    cols = F.unfold(x.double(), (kh, kw), dilation=(dh, dw), padding=(ph, pw), stride=(sh, sw)).reshape(B, groups, Dkg, L)
    cabs = cols.abs()
    want_w = torch.empty(B, S, Do * Dkg, dtype=torch.float64, device=DEV)
    bnd_w = torch.empty_like(want_w)
    want_b = torch.empty(B, S, Do, dtype=torch.float64, device=DEV)
    bnd_b = torch.empty_like(want_b)
    for s in range(S):  # per seed, so that the float64 copies stay the size of one seed's cotangent
        g64 = g[s].double().reshape(B, groups, Dog, L)
        want_w[:, s] = torch.einsum("bqol,bqkl->bqok", g64, cols).reshape(B, -1)
        bnd_w[:, s] = torch.einsum("bqol,bqkl->bqok", g64.abs(), cabs).reshape(B, -1) * eps
        want_b[:, s] = g64.sum(-1).reshape(B, Do)
        bnd_b[:, s] = g64.abs().sum(-1).reshape(B, Do) * eps
    out = (x, g, (kh, kw), (sh, sw), (ph, pw), (dh, dw), groups, Do, Dkg, want_w, bnd_w, want_b, bnd_b)
    _CASE_CACHE[shape] = out
    return out


def _columns(cols, Do, Dkg):
    """(P, col0, bcol0): "wb" bias columns after the weight's, "bw" before them, "w" no bias; gaps on every side"""
    width = Do * Dkg
    if cols == "wb":
        return width + Do + 7, 3, 3 + width + 2
    if cols == "bw":
        return width + Do + 7, 2 + Do + 3, 2
    return width + 7, 3, -1


def _within(got, want, bnd, what):
    err = (got.double() - want).abs()
    excess = (err - bnd).max().item()
    ratio = (err / bnd.clamp_min(1e-300)).max().item()
    print(f"{what}: worst |err| / bound = {ratio:.3f}")
    assert excess <= 0.0, f"{what}: error exceeds the bound by {excess:.3e} (ratio {ratio:.3f})"


@pytest.mark.parametrize("cols", ("wb", "bw", "w"))
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "-".join(str(v).replace(" ", "") for v in s))
def test_gconv_kernel_against_float64(shape, cols):
    """every output within ``(L + 2) * 2^-24 * sum_l |g_l * patch_l|`` of a float64 evaluation of the same inputs - the fp32
    bound of a length-L dot product that holds for ANY summation order (bias columns: ``patch = 1``); the other columns of
    ``Js`` keep what they held; a second run gives the same bits."""
    from laplace_amd._lib import get_kernels

    x, g, ks, st, pd, dl, groups, Do, Dkg, want_w, bnd_w, want_b, bnd_b = _kernel_inputs(shape)
    S, B = g.shape[:2]
    P, col0, bcol0 = _columns(cols, Do, Dkg)
    Js = torch.full((B, S, P), 7.5, device=DEV)
    get_kernels().jac_gconv(x, g, ks, st, pd, dl, groups, Js, col0, bcol0)
    touched = torch.zeros(P, dtype=torch.bool, device=DEV)
    _within(Js[:, :, col0:col0 + Do * Dkg], want_w, bnd_w, f"{shape} {cols} weight")
    touched[col0:col0 + Do * Dkg] = True
    if bcol0 >= 0:
        _within(Js[:, :, bcol0:bcol0 + Do], want_b, bnd_b, f"{shape} {cols} bias")
        touched[bcol0:bcol0 + Do] = True
    assert bool((Js[:, :, ~touched] == 7.5).all()), "columns outside the layer's were written"
    again = torch.full_like(Js, 7.5)
    get_kernels().jac_gconv(x, g, ks, st, pd, dl, groups, again, col0, bcol0)
    assert torch.equal(Js, again), "two runs on the same input differ"


def test_groups_1_is_the_contract_of_jac_conv():
    from laplace_amd._lib import get_kernels

    shape = (2, 2, 6, 1, 4, 5, 5, 3, 1, 1, 1)
    x, g, ks, st, pd, dl, groups, Do, Dkg, want_w, bnd_w, want_b, bnd_b = _kernel_inputs(shape)
    P, col0, bcol0 = _columns("wb", Do, Dkg)
    Js = torch.full((2, 2, P), 7.5, device=DEV)
    get_kernels().jac_conv(x, g, ks, st, pd, dl, Js, col0, bcol0)
    _within(Js[:, :, col0:col0 + Do * Dkg], want_w, bnd_w, "lk_jac_conv_f32 weight")
    _within(Js[:, :, bcol0:bcol0 + Do], want_b, bnd_b, "lk_jac_conv_f32 bias")


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
    """fails on a backend without the grouped-convolution route: there ``_tape()`` raises"""
    route_check(monkeypatch, DEV)


# ---- 4. a MobileNetV2-style network -------------------------------------------------------------------------------------
def test_mobilenet_diag_against_its_own_jacobians():
    """``diag(X, y)[1]`` against ``sum_n diag(J_n^T Lambda_n J_n)`` formed in float64 on the host from ``jacobians(X)``, for
    ALL depthwise columns and a seeded sample of 4 096 others (a smooth activation: see the docstring of nets.ResNet18)."""
    from laplace_amd import HipGGN
    from laplace_amd.nets import MobileNetV2Small

    torch.manual_seed(11)
    model = MobileNetV2Small(width=0.25, act=nn.Tanh)
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0.0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0.0, 0.1)
    model = model.to(DEV).eval()
    nb = 2 if DEV == "cpu" else 4
    X = torch.randn(nb, 3, 16, 16, device=DEV)
    y = torch.randint(10, (nb,), device=DEV)
    b = HipGGN(model, "classification")
    tape = b._tape()
    assert len(tape.gconv_taps) == 9 and all(t.module.groups == t.module.in_channels for t in tape.gconv_taps)
    assert b._supported()
    dw_cols = torch.cat([torch.arange(t.w_off, t.w_off + t.module.weight.numel()) for t in tape.gconv_taps])
    gen = torch.Generator().manual_seed(5)
    is_dw = torch.zeros(tape.n_params, dtype=torch.bool)
    is_dw[dw_cols] = True
    others = torch.nonzero(~is_dw).flatten()
    other_cols = others[torch.randperm(others.numel(), generator=gen)[:4096]]

    _, h = b.diag(X, y)
    sweep = tape.sweeps[frozenset({"gconv", "norm"})]
    assert sweep, getattr(tape, "sweep_reason", None)  # (one seed-batched reverse pass, not one autograd pass per seed)
    Js, f = b.jacobians(X)
    assert Js.shape == (nb, 10, tape.n_params)
    p = torch.softmax(f.double().cpu(), -1)
    Lam = torch.diag_embed(p) - p[:, :, None] * p[:, None, :]
    for what, cols in (("depthwise columns", dw_cols), ("other columns", other_cols)):
        J = Js[:, :, cols.to(Js.device)].double().cpu()
        want = torch.einsum("ncp,nck,nkp->p", J, Lam, J)
        check(h[cols.to(h.device)], want, what=f"diag of {what}")
