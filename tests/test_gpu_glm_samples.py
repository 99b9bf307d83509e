"""The GLM samples kernel (csrc/lk_glmsamples.hip) against the formulas of `_HipLaplace._glm_functional_samples` /
`_glm_predictive_samples` in fp64 on the CPU, with the same draw.  The bound of a case is element-wise
|out - out64| <= max(4 x the worst error of the SAME formulas in fp32 torch on the device, 2^-20 max(1, |out64|)): the kernel and
torch run chains of equal length in different orders, 4 x covers the order; the floor is for cases where torch happens to be
exact.  profiles/glm_samples_instances.md has every case as measured on an MI355X."""
import functools

import pytest
import torch

from tests.test_gpu_link import make_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 2.0 ** -20


def samples_ref(f_mu, f_var, z, diag, softmax):
    """the torch sequence of laplace_amd/laplace.py, line by line, in the dtype and on the device of the arguments"""
    scaled = f_var.sqrt().unsqueeze(-1) * z.unsqueeze(0) if diag else torch.matmul(torch.linalg.cholesky(f_var), z.unsqueeze(0))
    fs = (f_mu.unsqueeze(-1) + scaled).permute(2, 0, 1)
    return torch.softmax(fs, dim=-1) if softmax else fs


@functools.lru_cache(maxsize=None)
def inputs(C, B, n, diag):
    """full covariance: f_var_b = (A A^T / C + 0.1 I) 2^k of tests/test_gpu_link.py (correlated outputs, condition < 1e3);
    marginal variances: (0.1 + U(0, 1)) 2^k; k in {-6, 0, 4} by sample; fp32 values, held in fp64"""
    if not diag:
        return make_inputs(C, B, n, seed=C + n)
    g = torch.Generator().manual_seed(1000 + C + n)
    k = torch.tensor([(-6.0, 0.0, 4.0)[b % 3] for b in range(B)], dtype=torch.float64)
    f_var = ((0.1 + torch.rand(B, C, generator=g, dtype=torch.float64)) * torch.exp2(k).view(B, 1)).float().double()
    return (3 * torch.randn(B, C, generator=g, dtype=torch.float64)).float().double(), f_var, torch.randn(C, n, generator=g).double()


def run_kernel(f_mu, f_var, z, diag, softmax):
    """the kernel on fp32 device copies, its outputs inside guard bands; -> (out, info)"""
    from laplace_amd._lib import get_kernels

    (B, C), n = f_mu.shape, z.shape[1]
    obuf = torch.full((n * B * C + 128,), float("nan"), device=DEV)
    ibuf = torch.full((B + 8,), -7, dtype=torch.int32, device=DEV)
    dev = lambda t: t.float().to(DEV).contiguous()  # noqa: E731
    out, info = get_kernels().glm_samples(dev(f_mu), dev(f_var), dev(z), diag=bool(diag), softmax=bool(softmax),
                                          out=obuf[64:64 + n * B * C].view(n, B, C), info=ibuf[4:4 + B])
    assert torch.isnan(obuf[:64]).all() and torch.isnan(obuf[64 + n * B * C:]).all(), "a write outside out"
    assert (ibuf[:4] == -7).all() and (ibuf[4 + B:] == -7).all(), "a write outside info"
    return out.clone(), info.clone()


def errors(f_mu, f_var, z, diag, softmax, out):
    """(worst error over its bound, worst error, the largest bound, torch fp32's worst error)"""
    o64 = samples_ref(f_mu, f_var, z, diag, softmax)
    dev = lambda t: t.float().to(DEV)  # noqa: E731
    e32 = float((samples_ref(dev(f_mu), dev(f_var), dev(z), diag, softmax).double().cpu() - o64).abs().max())
    err = (out.double().cpu() - o64).abs()
    tol = torch.clamp(FLOOR * o64.abs().clamp(min=1.0), min=4 * e32)
    return float((err / tol).max()), float(err.max()), float(tol.max()), e32


# (C, B, n, diag).  Full covariance: the register tiers 16 | 32 | 64, the regime boundary 64 | 65, C % 4 != 0 (65, 177: scalar
# stores) and == 0 (80, 192), a partial 16-wide panel (65, 177), the largest C.  Marginal variances: the stages of 16 | 8 | 4 draws
# (C <= 1024 | 2048 | 4096), scalar (17, 2047) and 16-byte (1000, 4096) stores.  B = 1, 5 (a remainder of the four waves), and
# B = 2048 / 512: one chunk.  n = 1, 16 | 17 (the stage boundary), 40 and 100: chunks of 16, 16, 8 and 16 x 6, 4 draws.
CASES = [(1, 1, 1, 0), (2, 2048, 17, 0), (17, 5, 16, 0), (63, 5, 17, 0), (64, 5, 40, 0), (65, 5, 16, 0), (80, 1, 100, 0),
         (177, 5, 17, 0), (192, 5, 40, 0), (1, 1, 1, 1), (17, 512, 17, 1), (1000, 5, 40, 1), (2047, 1, 17, 1), (4096, 5, 17, 1)]
ONE_CHUNK = {(2, 2048, 17, 0), (17, 512, 17, 1), (1, 1, 1, 0), (1, 1, 1, 1), (65, 5, 16, 0), (17, 5, 16, 0)}


@pytest.mark.parametrize("softmax", [0, 1])
@pytest.mark.parametrize("C,B,n,diag", CASES, ids=lambda v: str(v))
def test_samples_against_fp64(C, B, n, diag, softmax):
    from laplace_amd._lib import get_kernels

    f_mu, f_var, z = inputs(C, B, n, diag)
    out, info = run_kernel(f_mu, f_var, z, diag, softmax)
    ratio, err, tol, e32 = errors(f_mu, f_var, z, diag, softmax, out)
    v = get_kernels().glm_samples_variant(B, C, n, diag, softmax)
    print(f"| {C} | {B} | {n} | {diag} | {softmax} | {v['regime']} | {v['chunks']} | {err:.3e} | {tol:.3e} | {e32:.3e} |")
    assert (v["chunks"] == 1) == ((C, B, n, diag) in ONE_CHUNK)
    assert not info.any() and torch.isfinite(out).all()
    assert ratio <= 1.0, f"worst error {err:.3e}, {ratio:.2f} of its bound (torch fp32: {e32:.3e})"
    if softmax:
        assert float((out.double().sum(-1) - 1).abs().max()) <= C * 2.0 ** -23
    again, _ = run_kernel(f_mu, f_var, z, diag, softmax)
    assert torch.equal(out, again), "two equal calls differ"


@pytest.mark.parametrize("C", [10, 100])
def test_a_factorisation_that_fails_is_reported_per_sample(C):
    from laplace_amd.laplace import HipLaplace

    f_mu, V, z = (t.clone() for t in inputs(C, 5, 40, 0))
    w, Q = torch.linalg.eigh(V[2])
    w[C // 2] = -0.5
    V[2] = ((Q * w) @ Q.T).float().double()
    V[2] = torch.tril(V[2]) + torch.tril(V[2], -1).T
    out, info = run_kernel(f_mu, V, z, 0, 0)
    good = [0, 1, 3, 4]
    assert int(info[2]) == int(torch.linalg.cholesky_ex(V[2]).info) and not info[good].any()
    assert torch.isnan(out[:, 2]).all() and torch.isfinite(out[:, good]).all()
    ratio, err, tol, e32 = errors(f_mu[good], V[good], z, 0, 0, out[:, good])
    print(f"| {C}, sample 2 indefinite | 5 | 40 | 0 | 0 | | | {err:.3e} | {tol:.3e} | {e32:.3e} |")
    assert ratio <= 1.0
    la = HipLaplace(torch.nn.Linear(4, C).to(DEV), "classification", "all", "kron")
    la.use_glm_sample_kernels = True
    la._glm_predictive_distribution = lambda x, diagonal_output=False: (f_mu.float().to(DEV), V.float().to(DEV))
    with pytest.raises(torch.linalg.LinAlgError, match="not positive-definite"):
        la.functional_samples(torch.zeros(5, 4, device=DEV), n_samples=40)


@pytest.mark.parametrize("structure", ["kron", "diag"])
@pytest.mark.parametrize("likelihood,C", [("classification", 3), ("regression", 2)])
def test_the_sampling_predictives_with_the_kernel_on_and_off(likelihood, C, structure):
    from torch import nn
    from torch.utils.data import DataLoader, TensorDataset

    from laplace_amd.laplace import HipLaplace

    torch.manual_seed(3)
    model = nn.Sequential(nn.Linear(6, 8), nn.Tanh(), nn.Linear(8, C)).to(DEV)
    X = torch.randn(12, 6, device=DEV)
    y = torch.randint(C, (12,), device=DEV) if likelihood == "classification" else torch.randn(12, C, device=DEV)
    la = HipLaplace(model, likelihood, "all", structure, prior_precision=0.5)
    la.fit(DataLoader(TensorDataset(X, y), batch_size=12))
    f_mu, f_var = (t.double().cpu() for t in la._glm_predictive_distribution(X))
    z = torch.randn(C, 33, device=DEV, generator=torch.Generator(DEV).manual_seed(11)).double().cpu()
    for name in ("functional_samples", "predictive_samples"):
        for diag in (False, True):
            got, nxt = {}, {}
            for on in (True, False):
                la.use_glm_sample_kernels = on
                g = torch.Generator(DEV).manual_seed(11)
                got[on] = getattr(la, name)(X, n_samples=33, diagonal_output=diag, generator=g)
                nxt[on] = torch.randn(4, device=DEV, generator=g)
            assert got[True].shape == (33, 12, C) and got[True].is_contiguous() and torch.equal(nxt[True], nxt[False])
            fv = torch.diagonal(f_var, dim1=1, dim2=2) if diag else f_var
            o64 = samples_ref(f_mu, fv, z, diag, name == "predictive_samples" and likelihood == "classification")
            err, e32 = ((got[on].double().cpu() - o64).abs() for on in (True, False))
            assert (err <= torch.clamp(FLOOR * o64.abs().clamp(min=1.0), min=4 * float(e32.max()))).all(), (name, diag, err.max(), e32.max())
