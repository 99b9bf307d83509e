"""The `nn` predictive of a last-layer posterior on the sampled-heads route (laplace_amd/laplace.py, csrc/lk_nnhead.hip), on a CPU
emulation of the kernel: ONE backbone pass per call, the values of the per-draw loop it replaces, and every case outside the route
on the path it should take."""
import os
import sys

import pytest
import torch
from torch import nn
from torch.utils.data import DataLoader, TensorDataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from laplace_amd._lib import set_kernels_for_testing  # noqa: E402
from laplace_amd.laplace import HipLaplace  # noqa: E402
from tests.emulated_kernels import EmulatedKernels  # noqa: E402
from tests.emulated_nn_head_kernels import EmulatedNnHeadKernels  # noqa: E402

N_S = 6


@pytest.fixture
def K():
    K = EmulatedNnHeadKernels()
    prev = set_kernels_for_testing(K)
    yield K
    set_kernels_for_testing(prev)


def fitted(likelihood="classification", subset="last_layer", on=True, frozen_bias=False):
    """(la, X, the list a forward hook on the backbone's first layer appends to)"""
    torch.manual_seed(3)
    C = 4 if likelihood == "classification" else 2
    model = nn.Sequential(nn.Linear(5, 7), nn.Tanh(), nn.Linear(7, C)).eval()
    model[2].bias.requires_grad_(not frozen_bias)  # (frozen: the posterior is over the weight alone)
    X = torch.randn(8, 5)
    y = torch.randint(C, (8,)) if likelihood == "classification" else torch.randn(8, C)
    la = HipLaplace(model, likelihood, subset, "kron", prior_precision=3.0)
    la.fit(DataLoader(TensorDataset(X, y), batch_size=8))
    la.backend.use_sweep = False  # (the feature pass calls the modules, so that the hook sees it)
    la.use_nn_head_kernels = on
    passes = []
    model[0].register_forward_hook(lambda *a: passes.append(1))
    return la, X, passes


def parent_loop(la, X, generator):  # the per-draw loop of n_samples model passes that the route replaces
    fs = []
    for sample in la.sample(N_S, generator):
        nn.utils.vector_to_parameters(sample, la.params)
        fs.append(la.model(X).detach())
    nn.utils.vector_to_parameters(la.mean, la.params)
    return torch.stack(fs)


CALLS = {"call": lambda la, X, g: la(X, pred_type="nn", link_approx="mc", n_samples=N_S, generator=g),
         "functional": lambda la, X, g: la.functional_samples(X, pred_type="nn", n_samples=N_S, generator=g),
         "predictive": lambda la, X, g: la.predictive_samples(X, pred_type="nn", n_samples=N_S, generator=g)}


@pytest.mark.parametrize("likelihood", ["classification", "regression"])
@pytest.mark.parametrize("call", list(CALLS))
def test_one_backbone_pass_and_the_values_of_the_loop(K, call, likelihood):
    la, X, passes = fitted(likelihood)
    out = CALLS[call](la, X, torch.Generator().manual_seed(5))
    assert len(passes) == 1 and len(K.seen) == 1, (len(passes), K.seen)
    fs = parent_loop(la, X, torch.Generator().manual_seed(5))
    ps = fs.softmax(-1) if likelihood == "classification" else fs
    want = {"functional": fs, "predictive": ps, "call": (ps.mean(0), ps.var(0)) if likelihood == "regression" else ps.mean(0)}[call]
    for a, b in zip(out if isinstance(out, tuple) else (out,), want if isinstance(want, tuple) else (want,)):
        assert a.shape == b.shape and (a - b).abs().max() <= 1e-6


# (case, keyword arguments of `fitted`, what is done to it before the call, backbone passes expected)
FALLBACKS = [
    ("switch-off", dict(on=False), lambda la: None, 1),
    ("frozen-bias", dict(frozen_bias=True), lambda la: None, 1),
    ("C-over-the-limit", dict(), lambda la: setattr(EmulatedNnHeadKernels, "NN_HEAD_MAX_C", 3), 1),
    ("no-nn_head", dict(), lambda la: set_kernels_for_testing(EmulatedKernels()), 1),
    ("training", dict(), lambda la: la.model.model.train(), N_S),
    ("all-weights", dict(subset="all"), lambda la: None, N_S),
]


@pytest.mark.parametrize("name,kw,prepare,n_passes", FALLBACKS, ids=[f[0] for f in FALLBACKS])
def test_outside_the_route(K, monkeypatch, name, kw, prepare, n_passes):
    """no kernel call; a last-layer posterior outside training mode still runs the backbone once (the cached-feature loop)"""
    monkeypatch.setattr(EmulatedNnHeadKernels, "NN_HEAD_MAX_C", 1024)
    la, X, passes = fitted(**kw)
    prepare(la)
    before = [p.detach().clone() for p in la.model.parameters()]
    out = la(X, pred_type="nn", link_approx="mc", n_samples=N_S, generator=torch.Generator().manual_seed(5))
    assert not K.seen and len(passes) == n_passes, (K.seen, len(passes))
    assert all(torch.equal(a, b) for a, b in zip(before, la.model.parameters()))
    want = parent_loop(la, X, torch.Generator().manual_seed(5)).softmax(-1).mean(0)
    assert (out - want).abs().max() <= 1e-6
