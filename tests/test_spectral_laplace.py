"""Host logic of ``HipFullLaplace(spectral=True)`` on the CPU emulation of the kernels (tests/spectral_emulation.py): what is
served, what falls back, when the cached spectrum is dropped, and that the default object is what it was."""
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from oracle.make_golden import PRIOR_PREC, SIGMA_NOISE
from tests.conftest import golden_model, load_golden
from tests.spectral_emulation import SpectralEmulatedKernels


@pytest.fixture
def K():
    from laplace_amd import _lib

    k = SpectralEmulatedKernels()
    prev = _lib.set_kernels_for_testing(k)
    yield k
    _lib.set_kernels_for_testing(prev)


def fitted(name, lik, sow, spectral, **kw):
    from laplace_amd.laplace import HipLaplace

    g = load_golden(name, lik)
    model, X, y = golden_model(name, g, dtype=torch.float32, device="cpu")
    sig = SIGMA_NOISE if lik == "regression" else 1.0
    la = HipLaplace(model, lik, sow, "full", prior_precision=PRIOR_PREC, sigma_noise=sig, spectral=spectral, **kw)
    la.fit(DataLoader(TensorDataset(X, y), batch_size=5))
    return la, X, y


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def test_the_default_object_is_unchanged(K):
    la, X, y = fitted("mlp", "classification", "last_layer", False)
    assert la.spectral is False
    with pytest.raises(NotImplementedError, match="no batched grid route for the full structure"):
        la.validation_loss_grid(DataLoader(TensorDataset(X, y), batch_size=4), torch.logspace(-1, 1, 3))
    la(X), la.log_marginal_likelihood(), la.sample(3)
    assert not K.calls  # no eigensolver, no spectral kernel
    ls, _, _ = fitted("mlp", "classification", "last_layer", True)
    ls(X)
    assert set(ls.state_dict()) == set(la.state_dict())  # no new keys
    assert all(not (torch.is_tensor(v) and v.ndim == 2 and v is ls.spectrum[1]) for v in ls.state_dict().values())


@pytest.mark.parametrize("name", ["mlp", "conv"])
@pytest.mark.parametrize("sow", ["all", "last_layer"])
@pytest.mark.parametrize("lik", ["classification", "regression"])
def test_predictive_and_marglik_match_the_cholesky_route(K, name, sow, lik):
    lc, X, _ = fitted(name, lik, sow, False)
    ls, _, _ = fitted(name, lik, sow, True)
    _, vc = lc._glm_predictive_distribution(X)
    K.calls.clear()
    _, vs = ls._glm_predictive_distribution(X)
    assert K.calls == ["syevj", "spectral_quadform_ll" if sow == "last_layer" else "spectral_quadform"]
    assert _rel(vs, vc) < 1e-4
    Js = lc._jacobians(X)[0]
    assert _rel(ls.functional_variance(Js), lc.functional_variance(Js)) < 1e-4
    assert _rel(ls.functional_covariance(Js), lc.functional_covariance(Js)) < 1e-4
    assert _rel(ls.posterior_covariance, lc.posterior_covariance) < 1e-4
    grads = {}
    for tag, la in (("c", lc), ("s", ls)):
        pp = torch.tensor([PRIOR_PREC], requires_grad=True)
        sn = torch.tensor(SIGMA_NOISE if lik == "regression" else 1.0, requires_grad=lik == "regression")
        ml = la.log_marginal_likelihood(prior_precision=pp, sigma_noise=sn if lik == "regression" else None)
        g = torch.autograd.grad(ml, [pp] + ([sn] if lik == "regression" else []))
        grads[tag] = (ml.detach(), *g)
    for a, b in zip(grads["s"], grads["c"]):
        assert float((a.double() - b.double()).abs().max()) <= 1e-4 * max(1.0, float(b.double().abs().max())), grads
    assert K.calls.count("syevj") == 1  # the prior and the noise changed: no further decomposition


def test_marglik_optimisation_needs_no_factorisation_per_step(K, monkeypatch):
    ls, _, _ = fitted("mlp", "classification", "last_layer", True)
    lc, _, _ = fitted("mlp", "classification", "last_layer", False)
    want = lc.optimize_prior_precision(method="marglik", n_steps=20, prior_structure="scalar").clone()

    def boom(*a, **k):
        raise AssertionError("a factorisation on the spectral route")

    monkeypatch.setattr(torch.linalg, "cholesky", boom)
    monkeypatch.setattr(torch.Tensor, "logdet", boom)
    got = ls.optimize_prior_precision(method="marglik", n_steps=20, prior_structure="scalar")
    assert torch.allclose(got, want, rtol=1e-3)
    assert K.calls.count("syevj") == 1


def test_a_non_scalar_prior_takes_the_cholesky_route(K):
    ls, X, _ = fitted("mlp", "classification", "all", True)
    ls.prior_precision = torch.linspace(0.5, 2.0, ls.n_layers)
    K.calls.clear()
    _, v = ls._glm_predictive_distribution(X)
    ls.log_marginal_likelihood()
    assert not K.calls
    lc, _, _ = fitted("mlp", "classification", "all", False)
    lc.prior_precision = torch.linspace(0.5, 2.0, ls.n_layers)
    assert torch.equal(v, lc._glm_predictive_distribution(X)[1])
    ls.prior_precision = torch.full((ls.n_layers,), 0.3)  # all entries equal: served
    ls._glm_predictive_distribution(X)
    assert "spectral_quadform" in K.calls


def test_the_cache_is_dropped_when_H_changes(K):
    ls, X, y = fitted("mlp", "classification", "last_layer", True)
    lam0 = ls.spectrum[0].clone()
    assert ls.spectrum[0] is ls.spectrum[0] and K.calls.count("syevj") == 1
    ls.fit(DataLoader(TensorDataset(X, y), batch_size=5), override=False)
    assert ls._spectrum is None
    assert torch.allclose(ls.spectrum[0], 2 * lam0, rtol=1e-4, atol=1e-5 * float(lam0.max()))
    sd = ls.state_dict()
    other, _, _ = fitted("mlp", "classification", "last_layer", True)
    other.spectrum
    other.load_state_dict(sd)
    assert other._spectrum is None
    assert torch.allclose(other.spectrum[0], ls.spectrum[0])


def test_the_sample_transform_has_the_posterior_covariance(K):
    ls, _, _ = fitted("mlp", "classification", "last_layer", True)
    T = ls._sample_transform(torch.eye(ls.n_params)).T  # row i of (I T^T) is column i of T
    lc, _, _ = fitted("mlp", "classification", "last_layer", False)
    assert _rel(T @ T.T, lc.posterior_covariance) < 1e-4
    g = torch.Generator().manual_seed(0)
    s = ls.sample(7, generator=g)
    assert s.shape == (7, ls.n_params) and bool(torch.isfinite(s).all())


@pytest.mark.parametrize("name,sow,lik", [("mlp", "last_layer", "classification"), ("conv", "all", "classification"),
                                          ("mlp", "all", "regression")])
def test_the_batched_grid_installs_what_the_loop_installs(K, name, sow, lik):
    ls, X, y = fitted(name, lik, sow, True)
    val = DataLoader(TensorDataset(X, y), batch_size=4)
    want = ls.gridsearch_prior_precision(val, -2, 2, 21).clone()
    ls.prior_precision = 123.0
    K.calls.clear()
    got = ls.gridsearch_prior_precision(val, -2, 2, 21, batched=True)
    assert torch.equal(got, want)
    assert ("spectral_grid_ll" if sow == "last_layer" else "spectral_grid") in K.calls
    losses = ls.validation_loss_grid(val, torch.logspace(-2, 2, 21))
    assert losses.dtype == torch.float64 and losses.shape == (21,)


def test_the_grid_chunks_the_rotated_jacobians_under_the_budget(K):
    ls, X, y = fitted("mlp", "classification", "all", True)
    val = DataLoader(TensorDataset(X, y), batch_size=4)
    want = ls.validation_loss_grid(val, torch.logspace(-2, 2, 5))
    ls.grid_var_budget_bytes = 4 * ls.n_outputs * ls.n_params * 2  # two samples per chunk
    K.calls.clear()
    got = ls.validation_loss_grid(val, torch.logspace(-2, 2, 5))
    assert K.calls.count("spectral_grid") > len(val)
    assert torch.allclose(got, want, rtol=1e-6)


def test_a_solve_that_runs_out_of_sweeps_is_retried_with_jitter_then_raises(K):
    ls, X, _ = fitted("mlp", "classification", "last_layer", True)
    want = ls.spectrum[0].clone()
    ls._spectrum = None
    K.calls.clear()
    K.fail_syevj = 1  # the first solve fails, H + I succeeds: 1 is subtracted again
    lam, Q = ls.spectrum
    assert K.calls == ["syevj", "syevj"]
    assert torch.allclose(lam, want, rtol=1e-4, atol=1e-5 * float(want.max())) and float(lam.min()) >= 0.0
    ls._spectrum = None
    K.fail_syevj = 2
    with pytest.raises(RuntimeError, match="did not converge, also not with jitter"):
        ls.spectrum
    assert ls._spectrum is None


def test_functional_covariance_of_many_rows_goes_through_one_gemm(K):
    ls, X, _ = fitted("mlp", "classification", "last_layer", True)
    lc, _, _ = fitted("mlp", "classification", "last_layer", False)
    Js = lc._jacobians(X)[0]
    assert Js.shape[0] * Js.shape[1] > 10
    K.calls.clear()
    got = ls.functional_covariance(Js)
    assert "spectral_quadform" not in K.calls
    assert _rel(got, lc.functional_covariance(Js)) < 1e-4
    K.calls.clear()
    few = Js[:2, :2]
    assert _rel(ls.functional_covariance(few), lc.functional_covariance(few)) < 1e-4 and "spectral_quadform" in K.calls


def test_the_equal_entries_question_is_asked_once_per_prior_tensor(K, monkeypatch):
    ls, X, _ = fitted("mlp", "classification", "all", True)
    ls.prior_precision = torch.full((ls.n_layers,), 0.3)
    assert ls._spectral_route()
    seen = ls._pp_equal
    for _ in range(3):
        assert ls._spectral_route() and ls._pp_equal is seen
    ls.prior_precision = torch.linspace(0.5, 2.0, ls.n_layers)
    assert not ls._spectral_route() and ls._pp_equal is not seen
