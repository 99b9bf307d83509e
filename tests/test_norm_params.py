"""Parameters of BatchNorm / LayerNorm / GroupNorm layers on the device route - host logic on the kernel emulation
(tests/emulated_norm_kernels.py) against the goldens of the unmodified reference (tools/make_norm_golden.py).

Tolerance ``1e-5`` max-normalised in fp32: the emulation is stock torch, and the reference's own fp32 run of these models
sits at most ``1.0e-6`` from its fp64 values - ten times that.
"""
import pytest
import torch
from torch import nn
from torch.utils.data import DataLoader, TensorDataset

from oracle.make_golden import PRIOR_PREC, SIGMA_NOISE
from tests.norm_fixtures import (NORM_FIXTURES, count_norm_calls, ef_gradients_from_golden, golden_model, load_golden, rel,
                                 route_check)

LIKS = ("classification", "regression")
CASES = [(n, l) for n in NORM_FIXTURES for l in LIKS]
TOL = 1e-5


@pytest.fixture
def norm_kernels():
    from laplace_amd import _lib
    from tests.emulated_norm_kernels import EmulatedNormKernels

    prev = _lib.set_kernels_for_testing(EmulatedNormKernels())
    yield
    _lib.set_kernels_for_testing(prev)


@pytest.fixture
def stock_kernels():
    from laplace_amd import _lib
    from tests.emulated_kernels import EmulatedKernels

    prev = _lib.set_kernels_for_testing(EmulatedKernels())
    yield
    _lib.set_kernels_for_testing(prev)


def check(got, want, what):
    e = rel(got, want)
    print(f"{what}: {e:.3e}")
    assert e < TOL, f"{what}: rel err {e:.3e}"


@pytest.mark.parametrize("use_sweep", (True, False))
@pytest.mark.parametrize("name,lik", CASES)
def test_ggn_and_ef_against_reference_golden(norm_kernels, name, lik, use_sweep):
    from laplace_amd import HipEF, HipGGN

    g = load_golden(name, lik)
    model, X, y = golden_model(name, g)
    b = HipGGN(model, lik)
    b.use_sweep = use_sweep
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
def test_laplace_all_against_reference_golden(norm_kernels, name, lik, hs):
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


def test_route_check_generic_route_forbidden(norm_kernels, monkeypatch):
    route_check(monkeypatch, "cpu")


def _embedding_model():
    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.emb = nn.Embedding(7, 6)
            self.ln = nn.LayerNorm(6)
            self.fc = nn.Linear(6, 3)

        def forward(self, x):
            return self.fc(torch.tanh(self.ln(self.emb(x).mean(1))))

    return M()


def test_uncovered_keeps_its_meaning_and_unserved_is_per_call(norm_kernels):
    from laplace_amd import HipGGN

    for name in NORM_FIXTURES:
        g = load_golden(name, "classification")
        model, X, y = golden_model(name, g)
        b = HipGGN(model, "classification")
        tape = b._tape()
        norm_params = [p for m in model.modules() if isinstance(m, (nn.BatchNorm2d, nn.LayerNorm, nn.GroupNorm))
                       for p in (m.weight, m.bias)]
        assert [id(p) for p in tape.uncovered] == [id(p) for p in norm_params]  # (what it was before the norm taps)
        assert tape.unserved == [] and b._supported()
        assert all(t.kind == "norm" for t in tape.norm_taps) and all(t.kind != "norm" for t in tape.taps)
        with pytest.raises(NotImplementedError, match="KFAC supports"):
            b.kron(X, y, N=len(X))
    # a BatchNorm in training mode is not served, in the call in which it is in training mode
    g = load_golden("normbn", "classification")
    model, X, y = golden_model("normbn", g)
    b = HipGGN(model, "classification")
    assert b._supported()
    model.train()
    assert len(b._tape().unserved) == 4 and not b._supported()
    model.eval()
    assert b._supported()
    model[1].bn1.running_mean = model[1].bn1.running_var = None  # (no running statistics: batch statistics in eval mode)
    assert len(b._tape().unserved) == 2 and not b._supported()
    # an embedding stays unserved (its LayerNorm alone would be served)
    torch.manual_seed(0)
    m = _embedding_model()
    b = HipGGN(m, "classification")
    tape = b._tape()
    assert [id(p) for p in tape.unserved] == [id(m.emb.weight)] and len(tape.uncovered) == 3 and not b._supported()


def test_frozen_weight_or_bias_of_a_norm_layer(norm_kernels, monkeypatch):
    """either affine parameter may be frozen (or absent): its columns do not exist, the other one is served"""
    from torch.func import functional_call, jacrev, vmap

    from laplace_amd import HipGGN

    torch.manual_seed(3)
    X = torch.randn(6, 4, 5)
    for freeze in ("weight", "bias"):
        m = nn.Sequential(nn.Linear(5, 8), nn.LayerNorm(8), nn.Tanh(), nn.Flatten(), nn.Linear(32, 2))
        m[1].weight.data.uniform_(0.5, 1.5), m[1].bias.data.normal_()
        getattr(m[1], freeze).requires_grad_(False)
        params = {k: v for k, v in m.named_parameters() if v.requires_grad}
        frozen = {k: v for k, v in m.named_parameters() if not v.requires_grad}
        J = vmap(lambda x: jacrev(lambda p: functional_call(m, {**p, **frozen}, (x[None],))[0])(params))(X)
        want = torch.cat([J[k].reshape(6, 2, -1) for k in params], -1)
        b = HipGGN(m, "regression")
        tap = b._tape().norm_taps[0]
        assert (tap.w_off < 0) == (freeze == "weight") and (tap.b_off < 0) == (freeze == "bias")
        calls = count_norm_calls(monkeypatch)
        Js, _ = b.jacobians(X)
        assert len(calls) == 1 and Js.shape == want.shape
        assert rel(Js, want) < TOL


def test_nchw_sweep_delivers_the_cotangent_of_a_tapped_batchnorm(norm_kernels):
    """the seed-batched NCHW sweep against the autograd tape (the witness): inputs and output cotangents of every tap,
    the BatchNorm that feeds only a ReLU and the one in front of the in-place residual add included"""
    from laplace_amd import HipGGN
    from laplace_amd.sweep_nhwc import SplitSweep

    g = load_golden("normbn", "classification")
    model, X, y = golden_model("normbn", g)
    seeds = torch.eye(3)[:, None, :].expand(3, len(X), 3).contiguous()
    got = {}
    for use_sweep in (True, False):
        b = HipGGN(model, "classification")
        b.use_sweep = use_sweep
        f, tape, grad_fn = b._forward(X, extra=True)
        taps = tape.taps + tape.norm_taps
        grads = grad_fn(seeds)
        assert len(grads) == len(taps) == 6
        got[use_sweep] = {t.name: (t.a.clone(), gr.clone()) for t, gr in zip(taps, grads)}
        assert tape.route == frozenset({"norm"})
        sweep = tape.sweeps.get(tape.route)
        if use_sweep:
            assert isinstance(sweep, SplitSweep) and not sweep.split_ok and "tapped BatchNorm" in sweep.split_reason
            assert set(tape.sweeps) == {tape.route}  # (the Linear / Conv2d sweep is a separate object, not built here)
        else:
            assert sweep is None
        tape.release()
    assert set(got[True]) == {"0", "1.conv1", "1.conv2", "4", "1.bn1", "1.bn2"}
    for name, (a, gr) in got[False].items():
        assert rel(got[True][name][0], a) < TOL, name
        assert rel(got[True][name][1], gr) < TOL, name


def test_models_without_norm_taps_build_the_sweep_they_built_before(norm_kernels):
    from laplace_amd import HipGGN
    from tests.conftest import golden_model as gm, load_golden as lg

    g = lg("bnres", "classification")
    model, X, y = gm("bnres", g, dtype=torch.float32)
    b = HipGGN(model, "classification")
    b.jacobians(X), b.diag(X, y)
    tape = b._tape()
    assert tape.norm_taps == [] and set(tape.sweeps) == {frozenset()} and tape.sweep


def test_stock_emulation_without_the_entry_point_takes_the_generic_route(stock_kernels, monkeypatch):
    from laplace_amd import HipGGN
    from laplace_amd._lib import get_kernels

    assert getattr(get_kernels(), "jac_norm_affine", None) is None
    used = []
    inner = torch.func.jacrev

    def spy(*a, **kw):
        used.append(1)
        return inner(*a, **kw)

    monkeypatch.setattr(torch.func, "jacrev", spy)
    for name in NORM_FIXTURES:
        g = load_golden(name, "classification")
        model, X, y = golden_model(name, g)
        b = HipGGN(model, "classification")
        assert not b._supported()
        n = len(used)
        Js, _ = b.jacobians(X)
        assert len(used) > n
        assert rel(Js, g["Js"]) < TOL
        assert rel(b.diag(X, y)[1], g["h_ggn"]) < TOL


def test_switch_off_takes_the_generic_route(norm_kernels, monkeypatch):
    from laplace_amd import HipGGN

    g = load_golden("normgn", "regression")
    model, X, y = golden_model("normgn", g)
    b = HipGGN(model, "regression")
    b.use_norm_kernels = False
    calls = count_norm_calls(monkeypatch)
    assert not b._supported()
    assert rel(b.jacobians(X)[0], g["Js"]) < TOL and rel(b.diag(X, y)[1], g["h_ggn"]) < TOL
    assert not calls


def test_fp64_model_is_served_by_its_fp32_twin(norm_kernels, monkeypatch):
    from laplace_amd import HipGGN
    from tests.norm_fixtures import forbid_generic_route

    forbid_generic_route(monkeypatch)
    g = load_golden("normln", "classification")
    model, X, y = golden_model("normln", g, dtype=torch.float64)
    Js, f = HipGGN(model, "classification").jacobians(X)
    assert Js.dtype == torch.float64 and rel(Js, g["Js"]) < TOL


def test_norm_layer_applied_twice_goes_back_to_the_generic_route(norm_kernels):
    from laplace_amd import HipGGN

    class Twice(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1, self.ln, self.fc2 = nn.Linear(4, 6), nn.LayerNorm(6), nn.Linear(6, 2)

        def forward(self, x):
            return self.fc2(self.ln(torch.tanh(self.ln(self.fc1(x)))))

    torch.manual_seed(1)
    m, X = Twice(), torch.randn(5, 4)
    ref = HipGGN(m, "regression")
    ref.use_norm_kernels = False
    want = ref.jacobians(X)[0]
    b = HipGGN(m, "regression")
    assert rel(b.jacobians(X)[0], want) < TOL
    assert rel(b.diag(X, torch.zeros(5, 2))[1], ref.diag(X, torch.zeros(5, 2))[1]) < TOL
