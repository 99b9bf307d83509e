"""Batched prior-precision grid search (``validation_loss_grid``, ``gridsearch_prior_precision(batched=True)``) against
the per-point loop, on CPU: the three grid kernels are restated in torch on a subclass of the emulated kernels."""
from math import pi

import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from oracle.make_golden import PRIOR_PREC, SIGMA_NOISE
from tests.conftest import golden_model, load_golden
from tests.emulated_kernels import EmulatedKernels


class GridKernels(EmulatedKernels):
    """torch restatements of lk_quadform_linear_grid_f32 / lk_quadform_shared_grid_f32 / lk_probit_nll_grid_f32"""

    GRID_KRON, GRID_KRON_DAMPED, GRID_DIAG = 0, 1, 2

    @staticmethod
    def _weights(w0, w1, deltas, mode, Do, Di):  # [G, Do, Di]
        d = deltas.reshape(-1, 1, 1)
        if mode == 0:
            return 1.0 / (torch.outer(w0, w1)[None] + d)
        if mode == 1:
            sd = torch.sqrt(d)
            return 1.0 / ((w0[None, :, None] + sd) * (w1[None, None, :] + sd))
        return 1.0 / (w0.reshape(1, Do, Di) + d)

    def quadform_linear_grid(self, u, v, w0, w1, deltas, mode, var, ub=None, wb=None):
        W = self._weights(w0, w1, deltas, mode, u.shape[2], v.shape[1])
        S = torch.einsum("ni,goi->gno", v**2, W)
        var += torch.einsum("cno,gno->gnc", u**2, S)
        if ub is not None:
            var += torch.einsum("cno,go->gnc", ub**2, 1.0 / (wb[None] + deltas[:, None]))
        return var

    def quadform_shared_grid(self, u, v, w0, w1, deltas, mode, var, seed_major=False):
        if seed_major:
            u = u.permute(1, 0, 2, 3)
        M = torch.einsum("ncol,nil->ncoi", u, v)
        var += torch.einsum("ncoi,goi->gnc", M**2, self._weights(w0, w1, deltas, mode, u.shape[2], v.shape[1]))
        return var

    def probit_nll_grid(self, f_mu, var, y, loss_sum):
        kappa = 1 / torch.sqrt(1.0 + pi / 8 * var)
        p = torch.softmax(kappa * f_mu[None], dim=-1)
        loss_sum += -torch.log(p[:, torch.arange(len(y)), y].clamp_min(1e-30)).double().sum(1)
        return loss_sum


@pytest.fixture
def grid_kernels():
    from laplace_amd import _lib

    K = GridKernels()
    prev = _lib.set_kernels_for_testing(K)
    yield K
    _lib.set_kernels_for_testing(prev)


def fitted(name, lik, sow, hs, dtype=torch.float32, **kw):
    from laplace_amd.laplace import HipLaplace

    g = load_golden(name, lik)
    model, X, y = golden_model(name, g, dtype=dtype, device="cpu")
    sig = SIGMA_NOISE if lik == "regression" else 1.0
    la = HipLaplace(model, lik, sow, hs, prior_precision=PRIOR_PREC, sigma_noise=sig, **kw)
    loader = DataLoader(TensorDataset(X, y), batch_size=5)
    la.fit(loader)
    return la, DataLoader(TensorDataset(X, y), batch_size=4)  # validation batches of another size


def loop_losses(la, loader, interval, **kw):
    """the per-point losses of gridsearch_prior_precision's loop (its argmin is what it installs)"""
    out = []
    for pp in interval:
        la.gridsearch_prior_precision(loader, grid_size=1, log_prior_prec_min=float(torch.log10(pp)),
                                      log_prior_prec_max=float(torch.log10(pp)), **kw)
        tot, cnt = 0.0, 0
        for X, y in la._val_batches(loader):  # tensor or dict (HuggingFace-style) batches, as the loop reads them
            o = la(X, **{k: v for k, v in kw.items() if k in ("link_approx", "n_samples")})
            if la.likelihood == "regression":
                tot += float(((o[0] - y.reshape(o[0].shape)) ** 2).sum())
            else:
                tot += float(-torch.log(o[torch.arange(len(y)), y].clamp_min(1e-30)).sum())
            cnt += len(y)
        out.append(tot / cnt)
    return torch.tensor(out, dtype=torch.float64)


GRID = torch.logspace(-3, 3, 7)
CASES = [(n, hs, sow) for n in ("mlp", "conv", "seqlin") for hs in ("kron", "diag") for sow in ("all", "last_layer")]


@pytest.mark.parametrize("name,hs,sow", CASES)
def test_grid_losses_match_the_loop(grid_kernels, name, hs, sow):
    la, val = fitted(name, "classification", sow, hs)
    got = la.validation_loss_grid(val, GRID)
    assert got.dtype == torch.float64 and got.shape == (len(GRID),)
    want = loop_losses(la, val, GRID)
    assert torch.allclose(got, want, rtol=1e-6, atol=0), (got, want)


@pytest.mark.parametrize("name", ["mlp", "conv"])
def test_grid_losses_match_the_loop_with_damping(grid_kernels, name):
    la, val = fitted(name, "classification", "all", "kron", damping=True)
    got = la.validation_loss_grid(val, GRID)
    assert torch.allclose(got, loop_losses(la, val, GRID), rtol=1e-6, atol=0)


@pytest.mark.parametrize("name,hs,sow", [("mlp", "kron", "all"), ("conv", "diag", "all"), ("seqlin", "kron", "last_layer")])
def test_batched_gridsearch_installs_what_the_loop_does(grid_kernels, name, hs, sow):
    la, val = fitted(name, "classification", sow, hs)
    want = la.gridsearch_prior_precision(val, -2, 2, 21).clone()
    la.prior_precision = 123.0
    got = la.gridsearch_prior_precision(val, -2, 2, 21, batched=True)
    assert torch.equal(got, want)
    la.prior_precision = 123.0
    got = la.optimize_prior_precision(method="gridsearch", val_loader=val, log_prior_prec_min=-2, log_prior_prec_max=2,
                                      grid_size=21, batched=True)
    assert torch.equal(got, want)


def _uncovered_model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(4, 6), torch.nn.LayerNorm(6), torch.nn.Tanh(), torch.nn.Linear(6, 3))


@pytest.mark.parametrize("case", ["full", "mc", "loss", "fp64"])
def test_out_of_scope_falls_back_to_the_loop(grid_kernels, case):
    kw = {}
    if case == "full":
        la, val = fitted("mlp", "classification", "all", "full")
    elif case == "fp64":  # the fused single-delta predictive refuses a non-fp32 model (NotImplementedError)
        la, val = fitted("conv", "classification", "all", "kron", dtype=torch.float64)
    else:
        la, val = fitted("mlp", "classification", "all", "kron")
        kw = {"link_approx": "mc", "n_samples": 20} if case == "mc" else {
            "loss": lambda out, y: (out.argmax(-1) != y).float().mean()}
    with pytest.raises(NotImplementedError):
        la.validation_loss_grid(val, GRID, **{k: v for k, v in kw.items() if k != "n_samples"})
    torch.manual_seed(3)
    want = la.gridsearch_prior_precision(val, -2, 2, 9, **kw).clone()
    torch.manual_seed(3)
    got = la.gridsearch_prior_precision(val, -2, 2, 9, batched=True, **kw)
    assert torch.equal(got, want)


def test_uncovered_model_is_out_of_scope(grid_kernels):
    from laplace_amd.laplace import HipLaplace

    X, y = torch.randn(8, 4), torch.randint(3, (8,))
    la = HipLaplace(_uncovered_model(), "classification", "all", "diag")
    la.fit(DataLoader(TensorDataset(X, y), batch_size=4))
    val = DataLoader(TensorDataset(X, y), batch_size=4)
    with pytest.raises(NotImplementedError):
        la.validation_loss_grid(val, GRID)
    want = la.gridsearch_prior_precision(val, -2, 2, 9).clone()
    assert torch.equal(la.gridsearch_prior_precision(val, -2, 2, 9, batched=True), want)


def test_nan_scores_inf(grid_kernels, monkeypatch):
    la, val = fitted("mlp", "classification", "all", "kron")
    orig = GridKernels.probit_nll_grid

    def poisoned(self, f_mu, var, y, loss_sum):
        orig(self, f_mu, var, y, loss_sum)
        loss_sum[0] = float("nan")
        return loss_sum

    monkeypatch.setattr(GridKernels, "probit_nll_grid", poisoned)
    got = la.validation_loss_grid(val, GRID)
    assert torch.isinf(got[0]) and torch.isfinite(got[1:]).all()
    pp = la.gridsearch_prior_precision(val, -3, 3, 7, batched=True)
    assert pp != GRID[0]


@pytest.mark.parametrize("hs", ["kron", "diag"])
def test_regression_loss_is_prior_free_and_ties_pick_the_first_point(grid_kernels, hs):
    la, val = fitted("mlp", "regression", "all", hs)
    got = la.validation_loss_grid(val, GRID)
    assert torch.allclose(got, loop_losses(la, val, GRID), rtol=1e-6, atol=0)
    assert (got == got[0]).all()
    pp = la.gridsearch_prior_precision(val, -3, 3, 7, batched=True)
    assert pp == torch.logspace(-3, 3, 7)[0]
