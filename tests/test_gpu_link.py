"""The fused link kernels of the GLM predictive (csrc/lk_link.hip) against the formulas of laplace_amd/laplace.py in fp64 on the
CPU.  The bound of a case is element-wise |p - p64| <= max(4 x the error of the SAME formulas in fp32 torch on the device, 2^-20):
the kernel and torch run chains of equal length in different orders, 4 x covers the order; 2^-20 is the floor where torch happens
to be exact.  Measured on an MI355X (profiles/link_instances.md has every case): the kernel's worst error is 5.5e-7, every case
but one sits under the floor; on bridge_norm at C = 100 the samples scaled by 2^-6 overflow exp() in fp32 torch and in the kernel
alike, so that case also holds the samples fp32 can serve to their own bound."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 2.0 ** -20


def link_ref(f_mu, f_var, z, link, diag):
    """_HipLaplace.__call__'s link approximations, line by line, in the dtype and on the device of the arguments"""
    C = f_mu.shape[1]
    if link == "mc":
        scaled = f_var.sqrt().unsqueeze(-1) * z.unsqueeze(0) if diag else torch.matmul(torch.linalg.cholesky(f_var), z.unsqueeze(0))
        return torch.softmax(f_mu.unsqueeze(-1) + scaled, dim=1).mean(dim=-1)
    if link == "probit":
        var_diag = f_var if diag else torch.diagonal(f_var, dim1=1, dim2=2)
        return torch.softmax(f_mu / torch.sqrt(1.0 + math.pi / 8 * var_diag), dim=-1)
    V = torch.diag_embed(f_var) if diag else f_var
    row, col, tot = V.sum(-1), V.sum(-2), V.sum((1, 2))
    mu = f_mu - row * (f_mu.sum(-1) / tot).unsqueeze(-1)
    var = torch.diagonal(V, dim1=1, dim2=2) - row * col / tot.unsqueeze(-1)
    if link == "bridge_norm":
        scale = var.mean(dim=1, keepdim=True) / (C / 2) ** 0.5
        mu, var = mu / scale.sqrt(), var / scale
    alpha = (1 - 2 / C + mu.exp() / C**2 * torch.exp(-mu).sum(dim=1, keepdim=True)) / var
    return torch.nan_to_num(alpha / alpha.sum(dim=1, keepdim=True), nan=1.0)


def make_inputs(C, B, n, seed):
    """f_var_b = (A A^T / C + 0.1 I) 2^k, k in {-6, 0, 4} by sample; f_mu ~ 3 N(0, 1); z ~ N(0, 1): fp32 values, held in fp64"""
    g = torch.Generator().manual_seed(1000 + seed)
    A = torch.randn(B, C, C, generator=g, dtype=torch.float64)
    V = A @ A.transpose(1, 2) / C + 0.1 * torch.eye(C, dtype=torch.float64)
    k = torch.tensor([(-6.0, 0.0, 4.0)[(b + seed) % 3] for b in range(B)], dtype=torch.float64)
    V = (V * torch.exp2(k).view(B, 1, 1)).float().double()
    V = torch.tril(V) + torch.tril(V, -1).transpose(1, 2)
    assert float(torch.linalg.cond(V).max()) < 1e3  # fp32 Cholesky is stable by construction
    return (3 * torch.randn(B, C, generator=g, dtype=torch.float64)).float().double(), V, torch.randn(C, n, generator=g).double()


def run_kernel(f_mu, f_var, z, link, diag):
    """the kernel on fp32 device copies, its outputs inside guard bands; -> (probs, info)"""
    from laplace_amd._lib import get_kernels

    B, C = f_mu.shape
    pbuf = torch.full((B * C + 128,), float("nan"), device=DEV)
    ibuf = torch.full((B + 8,), -7, dtype=torch.int32, device=DEV)
    dev = lambda t: t.float().to(DEV).contiguous()  # noqa: E731
    probs, info = get_kernels().glm_link(dev(f_mu), dev(f_var), dev(z) if link == "mc" else None, link, diag,
                                         probs=pbuf[64:64 + B * C].view(B, C), info=ibuf[4:4 + B])
    assert torch.isnan(pbuf[:64]).all() and torch.isnan(pbuf[64 + B * C:]).all(), "a write outside probs"
    assert (ibuf[:4] == -7).all() and (ibuf[4 + B:] == -7).all(), "a write outside info"
    return probs.clone(), info.clone()


def bound_and_errors(f_mu, f_var, z, link, diag, probs, rows=slice(None)):
    p64 = link_ref(f_mu, f_var, z, link, diag)
    dev = lambda t: t.float().to(DEV)  # noqa: E731
    p32 = link_ref(dev(f_mu), dev(f_var), dev(z), link, diag)
    e32 = float((p32.double().cpu() - p64)[rows].abs().max())
    err = float((probs.double().cpu() - p64)[rows].abs().max())
    return err, max(4 * e32, FLOOR), e32, (p32.double().cpu() - p64).abs().amax(dim=1) < 0.1


# (link, C, B, n_samples, diag): both regimes and their boundary (64 | 65), the largest C, C = 1, the 16-draw stage and the
# 16-wide panel with and without a remainder (n, C = 16 | 17; C = 100 and 65 leave a partial tile), the register tiers 16 | 32 | 64
CASES = [
    ("mc", 1, 1, 1, 0), ("mc", 2, 5, 7, 0), ("mc", 3, 1, 16, 1), ("mc", 10, 5, 100, 0), ("mc", 16, 5, 17, 0), ("mc", 17, 5, 16, 0),
    ("mc", 64, 5, 17, 0), ("mc", 65, 5, 17, 0), ("mc", 100, 5, 100, 0), ("mc", 100, 1, 7, 1), ("mc", 192, 5, 17, 0),
    ("mc", 192, 1, 1, 0),
    ("bridge", 3, 5, 1, 0), ("bridge", 64, 5, 1, 0), ("bridge", 65, 5, 1, 0), ("bridge", 10, 5, 1, 1),
    ("bridge_norm", 2, 5, 1, 0), ("bridge_norm", 100, 5, 1, 0), ("bridge_norm", 192, 1, 1, 0),
    ("probit", 1, 1, 1, 0), ("probit", 64, 5, 1, 1), ("probit", 65, 5, 1, 0), ("probit", 192, 5, 1, 0),
]


@pytest.mark.parametrize("link,C,B,n,diag", CASES, ids=lambda v: str(v))
def test_link_against_fp64(link, C, B, n, diag):
    f_mu, V, z = make_inputs(C, B, n, seed=C + n)
    f_var = torch.diagonal(V, dim1=1, dim2=2).contiguous() if diag else V
    probs, info = run_kernel(f_mu, f_var, z, link, diag)
    err, tol, e32, sane = bound_and_errors(f_mu, f_var, z, link, diag, probs)
    print(f"| {link} | {C} | {B} | {n} | {diag} | {err:.3e} | {tol:.3e} | {e32:.3e} |")
    assert not info.any() and torch.isfinite(probs).all()
    assert err <= tol, f"worst error {err:.3e} over the bound {tol:.3e} (torch fp32: {e32:.3e})"
    if not sane.all():  # fp32 torch itself is off by O(1) on some samples (exp overflows): the others against their own bound
        err, tol, e32, _ = bound_and_errors(f_mu, f_var, z, link, diag, probs, rows=sane)
        print(f"| {link}, the {int(sane.sum())} samples fp32 serves | {C} | {B} | {n} | {diag} | {err:.3e} | {tol:.3e} | {e32:.3e} |")
        assert sane.any() and err <= tol, f"worst error {err:.3e} over the bound {tol:.3e} (torch fp32: {e32:.3e})"
    again, _ = run_kernel(f_mu, f_var, z, link, diag)
    assert torch.equal(probs, again), "two equal calls differ"


@pytest.mark.parametrize("C", [10, 100])
def test_a_factorisation_that_fails_is_reported_per_sample(C):
    from laplace_amd.laplace import HipLaplace

    f_mu, V, z = make_inputs(C, 5, 17, seed=C)
    w, Q = torch.linalg.eigh(V[2])
    w[C // 2] = -0.5
    V[2] = ((Q * w) @ Q.T).float().double()
    V[2] = torch.tril(V[2]) + torch.tril(V[2], -1).T
    probs, info = run_kernel(f_mu, V, z, "mc", 0)
    assert info[2] != 0 and not info[[0, 1, 3, 4]].any()
    assert torch.isnan(probs[2]).all()
    good = [0, 1, 3, 4]
    err, tol, e32, _ = bound_and_errors(f_mu[good], V[good], z, "mc", 0, probs[good])
    print(f"| mc, sample 2 indefinite | {C} | 5 | 17 | 0 | {err:.3e} | {tol:.3e} | {e32:.3e} |")
    assert err <= tol
    la = HipLaplace(torch.nn.Linear(4, C).to(DEV), "classification", "all", "kron")
    la._glm_predictive_distribution = lambda x, diagonal_output=False: (f_mu.float().to(DEV), V.float().to(DEV))
    with pytest.raises(torch.linalg.LinAlgError, match="not positive-definite"):
        la(torch.zeros(5, 4, device=DEV), link_approx="mc", n_samples=17)


def _nets():
    from torch import nn

    mlp = nn.Sequential(nn.Linear(6, 8), nn.Tanh(), nn.Linear(8, 3))
    conv = nn.Sequential(nn.Conv2d(2, 4, 3, padding=1), nn.ReLU(), nn.Flatten(), nn.Linear(4 * 5 * 5, 10))
    return {"mlp": (mlp, (12, 6), 3), "conv": (conv, (12, 2, 5, 5), 10)}


@pytest.mark.parametrize("structure", ["kron", "diag"])
@pytest.mark.parametrize("net", ["mlp", "conv"])
def test_the_predictive_with_the_kernels_on_and_off(net, structure):
    from torch.utils.data import DataLoader, TensorDataset

    from laplace_amd.laplace import HipLaplace

    torch.manual_seed(3)
    model, shape, C = _nets()[net]
    X, y = torch.randn(*shape, device=DEV), torch.randint(C, (shape[0],), device=DEV)
    la = HipLaplace(model.to(DEV), "classification", "all", structure, prior_precision=0.5)
    la.fit(DataLoader(TensorDataset(X, y), batch_size=shape[0]))
    assert la._link_kernels(*la._glm_predictive_distribution(X)) is not None, "the kernel does not serve this predictive"
    f_mu, f_var = (t.double().cpu() for t in la._glm_predictive_distribution(X))
    z = torch.randn(C, 33, device=DEV, generator=torch.Generator(DEV).manual_seed(11)).double().cpu()
    for link in ("probit", "mc", "bridge", "bridge_norm"):
        out = {}
        for on in (True, False):
            la.use_link_kernels = on
            out[on] = la(X, link_approx=link, n_samples=33, generator=torch.Generator(DEV).manual_seed(11))
        p64 = link_ref(f_mu, f_var, z, link, 0)
        err, e32 = ((out[on].double().cpu() - p64).abs().max().item() for on in (True, False))
        assert err <= max(4 * e32, FLOOR), f"{link}: {err:.3e} with the kernel, {e32:.3e} with torch"
