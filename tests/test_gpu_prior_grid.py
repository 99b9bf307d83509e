"""Batched prior-precision grid on the MI355X: the three grid kernels (csrc/lk_grid.hip) against fp64 torch and against G
calls of the single-delta kernels, the grid predictives against the fp64 oracle, and the batched search end to end
against the per-point loop."""
import copy
from math import pi

import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from tests.conftest import golden_model, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
DELTAS = torch.logspace(-4, 4, 9)


def K():
    from laplace_amd._lib import get_kernels

    return get_kernels()


def relerr(got, want):
    """elementwise relative error (every entry here is a positive sum)"""
    got, want = got.double().cpu(), want.double().cpu()
    return ((got - want).abs() / want.abs().clamp_min(1e-30)).max().item()


def weights64(w0, w1, d, mode, Do, Di):
    d = d.double().reshape(-1, 1, 1)
    if mode == 0:
        return 1.0 / (torch.outer(w0.double(), w1.double())[None] + d)
    if mode == 1:
        sd = d.sqrt()
        return 1.0 / ((w0.double()[None, :, None] + sd) * (w1.double()[None, None, :] + sd))
    return 1.0 / (w0.double().reshape(1, Do, Di) + d)


def operands(mode, Do, Di, gen):
    if mode == 2:
        return torch.rand(Do, Di, generator=gen) * 3, None
    return torch.rand(Do, generator=gen) * 2 + 0.01, torch.rand(Di, generator=gen) * 2 + 0.01


@pytest.mark.parametrize("C", [1, 2, 10, 37, 100])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_linear_grid_kernel(C, mode):
    gen = torch.Generator().manual_seed(C * 7 + mode)
    B, Do, Di = 5, 13, 67
    u, v = torch.randn(C, B, Do, generator=gen), torch.randn(B, Di, generator=gen)
    ub, wb = torch.randn(C, B, Do, generator=gen), torch.rand(Do, generator=gen) + 0.1
    w0, w1 = operands(mode, Do, Di, gen)
    dev = lambda t: None if t is None else t.to(DEV).contiguous()  # noqa: E731
    var = torch.zeros(len(DELTAS), B, C, device=DEV)
    K().quadform_linear_grid(dev(u), dev(v), dev(w0.reshape(-1) if mode == 2 else w0), dev(w1), dev(DELTAS), mode, var,
                             dev(ub), dev(wb))
    W = weights64(w0, w1, DELTAS, mode, Do, Di)
    want = torch.einsum("cno,ni,goi->gnc", u.double() ** 2, v.double() ** 2, W)
    want += torch.einsum("cno,go->gnc", ub.double() ** 2, 1.0 / (wb.double()[None] + DELTAS.double()[:, None]))
    assert relerr(var, want) < 1e-5
    if mode == 0:  # G calls of the single-delta kernel
        for g, d in enumerate(DELTAS):
            fv = torch.zeros(B, C, C, device=DEV)
            K().kron_quadform_linear(dev(u), dev(v), dev(w0), dev(w1), d.reshape(1).to(DEV), fv, dev(ub), dev(wb),
                                     d.reshape(1).to(DEV))
            assert relerr(var[g], torch.diagonal(fv, dim1=1, dim2=2)) < 1e-5


@pytest.mark.parametrize("C", [1, 2, 10, 37, 100])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("L", [9, 16])
@pytest.mark.parametrize("seed_major", [False, True])
def test_shared_grid_kernel(C, mode, L, seed_major):
    gen = torch.Generator().manual_seed(C * 13 + mode + L)
    B, Do, Dk = 3, 33, 135
    u, v = torch.randn(B, C, Do, L, generator=gen), torch.randn(B, Dk, L, generator=gen)
    w0, w1 = operands(mode, Do, Dk, gen)
    dev = lambda t: None if t is None else t.to(DEV).contiguous()  # noqa: E731
    var = torch.zeros(len(DELTAS), B, C, device=DEV)
    uu = u.permute(1, 0, 2, 3) if seed_major else u
    K().quadform_shared_grid(dev(uu), dev(v), dev(w0), dev(w1), dev(DELTAS), mode, var, seed_major=seed_major)
    M = torch.einsum("ncol,nil->ncoi", u.double(), v.double())
    want = torch.einsum("ncoi,goi->gnc", M**2, weights64(w0, w1, DELTAS, mode, Do, Dk))
    assert relerr(var, want) < 1e-5
    if C <= 10 and mode != 1:  # G calls of the single-delta kernels
        for g, d in enumerate(DELTAS):
            fv = torch.zeros(B, C, C, device=DEV)
            if mode == 0:
                K().kron_quadform_shared(dev(uu), dev(v), dev(w0), dev(w1), d.reshape(1).to(DEV), fv, seed_major=seed_major)
            else:
                K().diag_quadform_shared(dev(u), dev(v), dev(1.0 / (w0 + d)), fv)
            assert relerr(var[g], torch.diagonal(fv, dim1=1, dim2=2)) < 1e-5


def test_shared_grid_kernel_is_bit_reproducible():
    gen = torch.Generator().manual_seed(1)
    u, v = torch.randn(4, 10, 64, 16, generator=gen).to(DEV), torch.randn(4, 200, 16, generator=gen).to(DEV)
    l1, l2 = (torch.rand(64, generator=gen) + 0.01).to(DEV), (torch.rand(200, generator=gen) + 0.01).to(DEV)
    d = torch.logspace(-4, 4, 150).to(DEV)  # more than one launch's worth of grid points
    a = K().quadform_shared_grid(u, v, l1, l2, d, 0, torch.zeros(150, 4, 10, device=DEV))
    b = K().quadform_shared_grid(u, v, l1, l2, d, 0, torch.zeros(150, 4, 10, device=DEV))
    assert torch.equal(a, b)
    want = torch.einsum("ncoi,goi->gnc", torch.einsum("ncol,nil->ncoi", u.double(), v.double()) ** 2,
                        weights64(l1.cpu(), l2.cpu(), d.cpu(), 0, 64, 200).to(DEV))
    assert relerr(a, want) < 1e-5


@pytest.mark.parametrize("C", [1, 2, 10, 100])
def test_probit_nll_grid_kernel(C):
    gen = torch.Generator().manual_seed(C)
    G, B = 7, 300
    f = torch.randn(B, C, generator=gen) * 3
    var = torch.rand(G, B, C, generator=gen) * torch.logspace(-3, 3, G)[:, None, None]
    y = torch.randint(C, (B,), generator=gen)
    out = torch.zeros(G, dtype=torch.float64, device=DEV)
    K().probit_nll_grid(f.to(DEV), var.to(DEV), y.to(DEV), out)
    kappa = 1 / torch.sqrt(1.0 + pi / 8 * var.double())
    p = torch.softmax(kappa * f.double()[None], -1)
    want = -torch.log(p[:, torch.arange(B), y].clamp_min(1e-30)).sum(1)
    assert ((out.cpu() - want).abs() / want.abs().clamp_min(1.0)).max().item() < 1e-5  # (C = 1: every loss is 0)


@pytest.mark.parametrize("name", ["mlp", "conv", "seqlin", "resnetish"])
def test_grid_predictives_against_the_oracle(name):
    from laplace_amd import HipGGN
    from laplace_amd import predictive as P
    from oracle import curvature_oracle as co

    g = load_golden(name, "classification")
    m64, X64, y = golden_model(name, g)
    model = copy.deepcopy(m64).float().to(DEV)
    X = X64.float().to(DEV)
    backend = HipGGN(model, "classification")
    _, kron = backend.kron(X, y.to(DEV), N=len(X))
    dec = kron.decompose()
    Js = co.jacobians(m64, X64)[0]
    Qs = [[Q.double().cpu() for Q in b] for b in dec.eigenvectors]
    ls = [[e.double().cpu() for e in b] for b in dec.eigenvalues]
    for damping in (False, True):
        dec.damping = damping
        f_mu, var = P.glm_variance_kron_grid(backend, X, dec, DELTAS)
        for gi, d in enumerate(DELTAS):
            want = torch.diagonal(co.functional_variance_kron(Js, Qs, ls, float(d), damping=damping), dim1=1, dim2=2)
            assert relerr(var[gi], want) < 1e-5, (damping, float(d))
    _, h = backend.diag(X, y.to(DEV), N=len(X))
    f_mu, var = P.glm_variance_diag_grid(backend, X, h, DELTAS)
    for gi, d in enumerate(DELTAS):
        want = torch.diagonal(co.functional_variance_diag(Js, 1.0 / (h.double().cpu() + float(d))), dim1=1, dim2=2)
        assert relerr(var[gi], want) < 1e-5


def check_against_loop(la, val, grid):
    from tests.test_prior_grid import loop_losses

    got = la.validation_loss_grid(val, grid)
    again = la.validation_loss_grid(val, grid)
    assert torch.equal(got, again), "two runs differ"
    want = loop_losses(la, val, grid)
    got = got.cpu()
    assert relerr(got, want) < 1e-5, (got, want)
    top = torch.sort(want).values
    if (top[1] - top[0]) > 1e-4 * top[0].abs():
        assert int(got.argmin()) == int(want.argmin())


@pytest.mark.parametrize("name,hs,sow", [("mlp", "kron", "all"), ("conv", "kron", "all"), ("resnetish", "kron", "all"),
                                         ("conv", "diag", "all"), ("mlp", "kron", "last_layer"),
                                         ("resnetish", "diag", "last_layer")])
def test_batched_search_matches_the_loop(name, hs, sow):
    from laplace_amd.laplace import HipLaplace

    g = load_golden(name, "classification")
    model, X, y = golden_model(name, g, dtype=torch.float32, device=DEV)
    la = HipLaplace(model, "classification", sow, hs, prior_precision=1.0)
    la.fit(DataLoader(TensorDataset(X, y), batch_size=5))
    check_against_loop(la, DataLoader(TensorDataset(X, y), batch_size=4), torch.logspace(-3, 3, 13))


def test_batched_search_resnet18_c4_shape():
    from laplace_amd.laplace import HipLaplace
    from laplace_amd.nets import ResNet18

    torch.manual_seed(0)
    model = ResNet18(10).to(DEV).eval()
    X, y = torch.randn(128, 3, 32, 32, device=DEV), torch.randint(10, (128,), device=DEV)
    la = HipLaplace(model, "classification", "all", "kron", prior_precision=1.0)
    la.fit(DataLoader(TensorDataset(X, y), batch_size=128))
    check_against_loop(la, DataLoader(TensorDataset(X, y), batch_size=128), torch.logspace(-2, 4, 10))


def test_batched_search_dict_inputs_last_layer():
    from laplace_amd.laplace import HipLaplace
    from tests.test_dict_inputs_c5 import TinyEncoderClassifier, _data

    torch.manual_seed(711)
    model = TinyEncoderClassifier().to(DEV)
    rows, collate = _data(DEV)
    loader = DataLoader(rows, batch_size=8, collate_fn=collate)
    la = HipLaplace(model, "classification", "last_layer", "kron", last_layer_name="classifier", prior_precision=1.0)
    la.fit(loader)
    check_against_loop(la, loader, torch.logspace(-3, 3, 13))
    want = la.gridsearch_prior_precision(loader, -3, 3, 13).clone()
    assert torch.equal(la.gridsearch_prior_precision(loader, -3, 3, 13, batched=True), want)
