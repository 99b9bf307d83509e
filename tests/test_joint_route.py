"""`la(X, joint=True)` of the Kron and diag flavours on the joint kernels' route (laplace_amd/predictive.py, csrc/lk_joint.hip), on a
CPU emulation of the kernels: the values of the unmodified reference, one kernel call per Linear layer and no Jacobian; with the
switch off or a provider without the kernels, the Jacobian route and the same values."""
import pytest
import torch
from torch import nn

from laplace_amd._lib import set_kernels_for_testing
from tests.emulated_joint_kernels import EmulatedJointKernels
from tests.emulated_kernels import EmulatedKernels
from tests.test_sampling import _pair

CASES = [(hs, sow) for hs in ("kron", "diag") for sow in ("all", "last_layer")]


@pytest.fixture
def K(reference_dropin, monkeypatch):
    from laplace_amd.laplace import _HipLaplace

    monkeypatch.setattr(_HipLaplace, "use_joint_kernels", True)
    K = EmulatedJointKernels()
    prev = set_kernels_for_testing(K)
    yield K
    set_kernels_for_testing(prev)


def _count_jacobians(la, monkeypatch):
    calls = []
    for name in ("jacobians", "last_layer_jacobians"):
        real = getattr(la.backend, name)
        monkeypatch.setattr(la.backend, name, lambda *a, _real=real, **kw: (calls.append(1), _real(*a, **kw))[1])
    return calls


def _close(got, want):
    torch.testing.assert_close(got[0], want[0], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(got[1], want[1], rtol=5e-4, atol=1e-6)


@pytest.mark.parametrize("hs,sow", CASES)
def test_joint_route_matches_the_reference(K, monkeypatch, hs, sow):
    ours, theirs, X, _ = _pair("mlp", "regression", hs, sow)
    calls = _count_jacobians(ours, monkeypatch)
    want = theirs(X, joint=True)
    _close(ours(X, joint=True), want)
    n_linear = 1 if sow == "last_layer" else sum(isinstance(m, nn.Linear) for m in ours.model.modules())
    assert len(K.seen) == n_linear and {s[0] for s in K.seen} == {hs} and not calls, (K.seen, calls)


@pytest.mark.parametrize("off", ["switch", "provider"])
@pytest.mark.parametrize("hs,sow", CASES)
def test_outside_the_route(K, monkeypatch, hs, sow, off):
    ours, theirs, X, _ = _pair("mlp", "regression", hs, sow)
    if off == "switch":
        ours.use_joint_kernels = False
    else:
        monkeypatch.setattr("laplace_amd._lib._KERNELS", EmulatedKernels())
    calls = _count_jacobians(ours, monkeypatch)
    _close(ours(X, joint=True), theirs(X, joint=True))
    assert not K.seen and len(calls) == 1, (K.seen, calls)


@pytest.mark.parametrize("hs,sow", CASES)
def test_dropin_takes_the_joint_route(K, hs, sow):
    from torch.utils.data import DataLoader, TensorDataset

    from laplace_amd.dropin import reference_classes

    ours, theirs, X, y = _pair("mlp", "regression", hs, sow)
    la = reference_classes()[(sow, hs)](theirs.model if sow == "all" else theirs.model.model, "regression", prior_precision=0.7)
    la.fit(DataLoader(TensorDataset(X, y), batch_size=5))
    K.seen.clear()
    _close(la(X, joint=True), theirs(X, joint=True))
    assert K.seen and {s[0] for s in K.seen} == {hs}, K.seen
