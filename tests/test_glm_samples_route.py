"""The route of the GLM samples through the samples kernel (laplace_amd/laplace.py: `use_glm_sample_kernels`,
`_glm_sample_kernels`), on the CPU with a stub provider that records its calls: which calls take it, that classification asks for the
softmax in the same launch, and that the route consumes exactly the draw the torch sequence makes."""
import pytest
import torch
from torch import nn

from laplace_amd._lib import HipKernels, set_kernels_for_testing
from laplace_amd.laplace import HipKronLaplace


class StubKernels:
    LINK_MAX_C, GLM_SAMPLES_MAX_C_DIAG = 192, 4096

    def __init__(self):
        self.calls = []

    def glm_samples(self, f_mu, f_var, z, diag=False, softmax=False):
        self.calls.append(dict(z=z.clone(), diag=diag, softmax=softmax, f_var=tuple(f_var.shape)))
        scaled = f_var.sqrt().unsqueeze(-1) * z if diag else torch.linalg.cholesky(f_var) @ z
        fs = (f_mu.unsqueeze(-1) + scaled).permute(2, 0, 1).contiguous()
        return (fs.softmax(-1) if softmax else fs), torch.zeros(f_mu.shape[0], dtype=torch.int32)


@pytest.fixture
def K():
    K = StubKernels()
    prev = set_kernels_for_testing(K)
    yield K
    set_kernels_for_testing(prev)


def _la(likelihood, on=True):
    la = HipKronLaplace(nn.Linear(2, 3), likelihood)
    la.use_glm_sample_kernels = on
    return la


def _moments(C, B=4, dtype=torch.float32):
    g = torch.Generator().manual_seed(C)
    A = torch.randn(B, C, C, generator=g, dtype=dtype)
    return torch.randn(B, C, generator=g, dtype=dtype), A @ A.transpose(1, 2) / C + 0.1 * torch.eye(C, dtype=dtype)


@pytest.mark.parametrize("case,C,diag,served", [("fp32", 192, False, True), ("fp32", 193, True, True), ("fp32", 193, False, False),
                                                ("fp32", 4097, True, False), ("fp64", 3, False, False), ("off", 3, False, False),
                                                ("no-method", 3, False, False), ("cpu-tensors-real-provider", 3, False, False)])
def test_which_calls_the_kernel_serves(K, case, C, diag, served):
    f_mu, f_var = _moments(C, dtype=torch.float64 if case == "fp64" else torch.float32)
    if case == "no-method":
        set_kernels_for_testing(object())
    elif case == "cpu-tensors-real-provider":
        K = HipKernels()
        set_kernels_for_testing(K)
    got = _la("regression", on=case != "off")._glm_sample_kernels(f_mu, f_var, diag)
    assert got is (K if served else None)


@pytest.mark.parametrize("diag", [False, True])
@pytest.mark.parametrize("likelihood", ["classification", "regression"])
def test_the_route_takes_the_same_draw_and_asks_for_the_softmax(K, likelihood, diag):
    f_mu, f_var = _moments(3)
    la, n = _la(likelihood), 7
    g = torch.Generator().manual_seed(11)
    fs, ps = la._glm_functional_samples(f_mu, f_var, n, diag, g), la._glm_predictive_samples(f_mu, f_var, n, diag, g)
    after = torch.randn(2, generator=g)
    want = torch.Generator().manual_seed(11)
    z = [torch.randn(3, n, generator=want), torch.randn(3, n, generator=want)]
    assert [c["softmax"] for c in K.calls] == [False, likelihood == "classification"]
    assert all(c["diag"] == diag and c["f_var"] == ((4, 3) if diag else (4, 3, 3)) for c in K.calls)
    assert all(torch.equal(c["z"], zz) for c, zz in zip(K.calls, z)) and torch.equal(after, torch.randn(2, generator=want))
    la.use_glm_sample_kernels = False  # the torch sequence from the same seed: the same values
    g = torch.Generator().manual_seed(11)
    torch.testing.assert_close(fs, la._glm_functional_samples(f_mu, f_var, n, diag, g))
    torch.testing.assert_close(ps, la._glm_predictive_samples(f_mu, f_var, n, diag, g))
    assert len(K.calls) == 2
