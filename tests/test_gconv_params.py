"""Weights of grouped / depthwise convolutions on the device route - host logic on the kernel emulation
(tests/emulated_gconv_kernels.py) against the goldens of the unmodified reference (tools/make_gconv_golden.py).

Tolerance: 1e-4 max-normalised, the bar of every golden test here (BASELINE.json north_star).
"""
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from oracle.make_golden import PRIOR_PREC, SIGMA_NOISE
from tests.gconv_fixtures import (GCONV_FIXTURES, GROUPED, N_PARAMS, ef_gradients_from_golden, golden_model, load_golden, rel,
                                  route_check)

LIKS = ("classification", "regression")
CASES = [(n, l) for n in GCONV_FIXTURES for l in LIKS]
TOL = 1e-4


@pytest.fixture
def gconv_kernels():
    from laplace_amd import _lib
    from tests.emulated_gconv_kernels import EmulatedGConvKernels

    prev = _lib.set_kernels_for_testing(EmulatedGConvKernels())
    yield
    _lib.set_kernels_for_testing(prev)


@pytest.fixture
def norm_only_kernels():
    from laplace_amd import _lib
    from tests.emulated_norm_kernels import EmulatedNormKernels

    prev = _lib.set_kernels_for_testing(EmulatedNormKernels())
    yield
    _lib.set_kernels_for_testing(prev)


def check(got, want, what):
    e = rel(got, want)
    print(f"{what}: {e:.3e}")
    assert e < TOL, f"{what}: rel err {e:.3e}"


@pytest.mark.parametrize("use_sweep", (True, False))
@pytest.mark.parametrize("name,lik", CASES)
def test_ggn_and_ef_against_reference_golden(gconv_kernels, name, lik, use_sweep):
    from laplace_amd import HipEF, HipGGN

    g = load_golden(name, lik)
    assert g["Js"].shape[-1] == N_PARAMS[name]
    model, X, y = golden_model(name, g)
    b = HipGGN(model, lik)
    b.use_sweep = use_sweep
    assert b._supported()
    Js, f = b.jacobians(X)
    check(Js, g["Js"], "jacobians")
    check(f, g["f"], "f")
    loss, H = b.full(X, y)
    check(H, g["H_ggn"], "full GGN")
    check(loss, g["loss"], "loss")
    loss, h = b.diag(X, y)
    check(h, g["h_ggn"], "diag GGN")
    check(b.diag(X[:5], y[:5])[1] + b.diag(X[5:], y[5:])[1], g["h_ggn"], "diag additivity")
    e = HipEF(model, lik)
    e.use_sweep = use_sweep
    loss, H = e.full(X, y)
    check(H, g["H_ef"], "full EF")
    check(loss, g["loss_ef"], "EF loss")
    check(e.diag(X, y)[1], g["h_ef"], "diag EF")
    Gs, loss = e.gradients(X, y)
    check(Gs, ef_gradients_from_golden(g, lik), "EF gradients")


@pytest.mark.parametrize("hs", ("diag", "full"))
@pytest.mark.parametrize("name,lik", CASES)
def test_laplace_all_against_reference_golden(gconv_kernels, name, lik, hs):
    from laplace_amd.laplace import HipLaplace

    g = load_golden(name, lik)
    model, X, y = golden_model(name, g)
    la = HipLaplace(model, lik, "all", hs, prior_precision=PRIOR_PREC,
                    sigma_noise=SIGMA_NOISE if lik == "regression" else 1.0)
    la.fit(DataLoader(TensorDataset(X, y), batch_size=5))
    tag = f"la.all.{hs}"
    check(la.loss, g[f"{tag}.loss"], "loss")
    check(la.H, g[f"{tag}.H"], "accumulated H")
    f_mu, f_var = la._glm_predictive_distribution(X)
    check(f_mu, g[f"{tag}.f_mu"], "f_mu")
    check(f_var, g[f"{tag}.f_var"], "f_var")
    check(la.log_marginal_likelihood(), g[f"{tag}.marglik"], "marglik")


def test_route_check_generic_route_forbidden(gconv_kernels, monkeypatch):
    route_check(monkeypatch, "cpu")


def test_block_budget_cuts_the_batch(gconv_kernels, monkeypatch):
    """a block budget below one minibatch's block: the diagonal and the diagonal predictive go through in batch chunks"""
    from laplace_amd import HipGGN
    from laplace_amd.predictive import glm_variance_diag
    from tests.gconv_fixtures import count_gconv_calls

    g = load_golden("gcsep", "classification")
    model, X, y = golden_model("gcsep", g)
    b = HipGGN(model, "classification")
    post_var = torch.rand(N_PARAMS["gcsep"], generator=torch.Generator().manual_seed(2)) + 0.1
    want = glm_variance_diag(b, X, post_var)[1]
    b.gconv_block_bytes = 4 * 3 * 108 * 4  # four samples of the wider grouped layer's [b, 3, 108] block
    calls = count_gconv_calls(monkeypatch)
    check(b.diag(X, y)[1], g["h_ggn"], "diag GGN in chunks")
    assert len(calls) > 2  # (more than one call per grouped tap; how many depends on the likelihood's number of seeds)
    seen = len(calls)
    check(glm_variance_diag(b, X, post_var)[1], want, "diagonal predictive in chunks")
    # 3 identity seeds: ceil(10 / 4) chunks of the 108-column layer, ceil(10 / 5) of the 72 + 8-column one (5.4 samples fit)
    assert len(calls) - seen == 3 + 2, len(calls) - seen


@pytest.mark.parametrize("name", GCONV_FIXTURES)
def test_kfac_refuses_and_names_the_layer(gconv_kernels, name):
    from laplace_amd import HipEF, HipGGN
    from laplace_amd.laplace import HipLaplace
    from laplace_amd.predictive import glm_variance_kron

    g = load_golden(name, "classification")
    model, X, y = golden_model(name, g)
    layer = GROUPED[name][0]
    for b in (HipGGN(model, "classification"), HipEF(model, "classification")):
        with pytest.raises(NotImplementedError, match=rf"^{layer}: KFAC has no rule for a grouped convolution.*freeze.*'diag' or 'full'"):
            b.kron(X, y, N=len(X))
        with pytest.raises(NotImplementedError, match=rf"^{layer}: KFAC has no rule"):
            b.kron_accumulator(len(X)).add_batch(X, y)
    with pytest.raises(NotImplementedError, match=rf"^{layer}: KFAC has no rule"):
        glm_variance_kron(HipGGN(model, "classification"), X, None)
    # the batched diagonal grid is out of scope for such a model and says so the way it does for every uncovered model
    la = HipLaplace(model, "classification", "all", "diag")
    la.fit(DataLoader(TensorDataset(X, y), batch_size=5))
    from laplace_amd.predictive import glm_variance_diag_grid

    with pytest.raises(NotImplementedError):
        glm_variance_diag_grid(la.backend, X, la.H, [0.1, 1.0])


def test_frozen_grouped_convolution_leaves_kfac_alone(gconv_kernels):
    from laplace_amd import HipGGN

    g = load_golden("gcdw7", "classification")
    model, X, y = golden_model("gcdw7", g)
    for p in model[1].parameters():
        p.requires_grad_(False)
    b = HipGGN(model, "classification")
    assert b._tape().gconv_taps == [] and b._supported()
    loss, kron = b.kron(X, y, N=len(X))
    assert len(kron.kfacs) == 4 and torch.isfinite(loss)
    # the sweep now carries the cotangent THROUGH the frozen grouped layer: same factors as the autograd tape
    assert b._tape().sweep
    t = HipGGN(model, "classification")
    t.use_sweep = False
    loss_t, kron_t = t.kron(X, y, N=len(X))
    assert not getattr(t._tape(), "sweep", None)
    assert rel(loss, loss_t) < 1e-5
    for F, Ft in zip(kron.kfacs, kron_t.kfacs):
        for A, At in zip(F, Ft):
            assert rel(A, At) < 1e-5


@pytest.mark.parametrize("name", ("gcsep", "gcres"))
def test_sweep_delivers_the_tape_s_gradients(gconv_kernels, name):
    """the seed-batched sweep (one reverse pass for all seeds, grouped backward-data included) against the autograd tape:
    inputs and output cotangents of every tap"""
    from laplace_amd import HipGGN
    from laplace_amd.sweep import SeedBatchedSweep

    g = load_golden(name, "classification")
    model, X, y = golden_model(name, g)
    seeds = torch.eye(3)[:, None, :].expand(3, len(X), 3).contiguous()
    got = {}
    for use_sweep in (True, False):
        b = HipGGN(model, "classification")
        b.use_sweep = use_sweep
        f, tape, grad_fn = b._forward(X, extra=True)
        taps = b._served_taps(tape)
        assert [t.name for t in taps if t.kind == "gconv"] == GROUPED[name]
        grads = grad_fn(seeds)
        assert len(grads) == len(taps)
        got[use_sweep] = {t.name: (t.a.clone(), gr.clone()) for t, gr in zip(taps, grads)}
        assert tape.route == (frozenset({"gconv", "norm"}) if name == "gcres" else frozenset({"gconv"}))
        sweep = tape.sweeps.get(tape.route)
        if use_sweep:
            assert isinstance(sweep, SeedBatchedSweep) and not getattr(sweep, "split_ok", False)
            assert set(tape.sweeps) == {tape.route}  # (only the sweep of this route was built)
        else:
            assert sweep is None
        tape.release()
    assert set(got[True]) == set(got[False]) and len(got[True]) == {"gcsep": 5, "gcres": 8}[name]
    for tap, (a, gr) in got[False].items():
        assert rel(got[True][tap][0], a) < 1e-5, tap
        assert rel(got[True][tap][1], gr) < 1e-5, tap


def test_split_sweep_reports_a_grouped_convolution_as_foreign(gconv_kernels):
    from laplace_amd import conv as cv
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep_nhwc import SplitSweep

    nn = torch.nn
    model = nn.Sequential(nn.Conv2d(3, 32, 3, padding=1), nn.ReLU(), nn.Conv2d(32, 32, 3, padding=1, groups=32), nn.ReLU(),
                          nn.Conv2d(32, 32, 3, padding=1), nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(32, 3)).eval()
    assert not cv.supported(model[2]) and cv.supported(model[4])
    sweep = SplitSweep(model, {"0": model[0], "2": model[2], "4": model[4], "7": model[7]}, kernels=get_kernels)
    assert not sweep.split_ok and sweep.split_reason.startswith("2: grouped convolution")
    dense = nn.Sequential(*[nn.Conv2d(32, 32, 3, padding=1) if i == 2 else m for i, m in enumerate(model)]).eval()
    assert SplitSweep(dense, {"0": dense[0], "2": dense[2], "4": dense[4], "7": dense[7]}, kernels=get_kernels).split_ok
    # a grouped FIRST convolution with 8 output channels does not slip through the first-layer exemption either
    first = torch.nn.Sequential(torch.nn.Conv2d(2, 8, 3, padding=1, groups=2), torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten()).eval()
    sweep = SplitSweep(first, {"0": first[0]}, kernels=get_kernels)
    assert not sweep.split_ok and "grouped convolution" in sweep.split_reason


def test_kernel_object_without_the_entry_point_takes_the_generic_route(norm_only_kernels, monkeypatch):
    from laplace_amd import HipGGN
    from laplace_amd._lib import get_kernels

    assert getattr(get_kernels(), "jac_gconv", None) is None
    used = []
    inner = torch.func.jacrev

    def spy(*a, **kw):
        used.append(1)
        return inner(*a, **kw)

    monkeypatch.setattr(torch.func, "jacrev", spy)
    g = load_golden("gcsep", "classification")
    model, X, y = golden_model("gcsep", g)
    b = HipGGN(model, "classification")
    assert not b._supported()
    Js, _ = b.jacobians(X)
    assert used and rel(Js, g["Js"]) < TOL
    assert rel(b.diag(X, y)[1], g["h_ggn"]) < TOL


def test_dense_models_keep_their_tape_and_sweep(gconv_kernels):
    from laplace_amd import HipGGN
    from tests.conftest import golden_model as gm, load_golden as lg

    g = lg("bnres", "classification")
    model, X, y = gm("bnres", g, dtype=torch.float32)
    b = HipGGN(model, "classification")
    b.jacobians(X), b.diag(X, y)
    tape = b._tape()
    assert tape.gconv_taps == [] and tape.sweep and set(tape.sweeps) == {frozenset()}


def test_emulation_agrees_with_autograd_on_an_asymmetric_grouped_layer(gconv_kernels):
    """the emulation itself (the witness of the device tests) against per-sample autograd weight gradients"""
    from laplace_amd._lib import get_kernels

    torch.manual_seed(4)
    m = torch.nn.Conv2d(6, 6, (1, 3), stride=(2, 1), padding=(0, 1), groups=3).double()
    x = torch.randn(2, 6, 5, 7, dtype=torch.float64)
    out = m(x)
    g = torch.randn(3, *out.shape, dtype=torch.float64)
    Js = torch.full((2, 3, 6 * 2 * 3 + 6 + 4), 7.5, dtype=torch.float64)
    get_kernels().jac_gconv(x, g, m.kernel_size, m.stride, m.padding, m.dilation, m.groups, Js, 2, 40)
    for n in range(2):
        for s in range(3):
            gw, gb = torch.autograd.grad(m(x[n:n + 1]), (m.weight, m.bias), g[s, n:n + 1])
            assert torch.allclose(Js[n, s, 2:38], gw.flatten(), atol=1e-12) and torch.allclose(Js[n, s, 40:46], gb, atol=1e-12)
    assert bool((Js[:, :, :2] == 7.5).all()) and bool((Js[:, :, 38:40] == 7.5).all())


def test_batched_grid_search_falls_back_to_the_loop(gconv_kernels):
    """``gridsearch_prior_precision(batched=True)`` on a model with a grouped convolution: the batched grid declares itself out
    of scope and the per-point loop runs - the same choice as without ``batched``, and no error"""
    from laplace_amd.laplace import HipLaplace

    g = load_golden("gcsep", "classification")
    model, X, y = golden_model("gcsep", g)
    loader = DataLoader(TensorDataset(X, y), batch_size=5)
    picks = []
    for batched in (True, False):
        la = HipLaplace(model, "classification", "all", "diag")
        la.fit(loader)
        picks.append(float(la.gridsearch_prior_precision(loader, grid_size=5, batched=batched)))
    assert picks[0] == picks[1]
