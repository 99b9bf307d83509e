"""The wide link kernels of the GLM predictive (csrc/lk_linkwide.hip, 193 to 4096 classes) against the formulas of
laplace_amd/laplace.py in fp64 on the CPU, by the rule of tests/test_gpu_link.py: element-wise |p - p64| <= max(4 x the error of the
SAME formulas in fp32 torch on the device, 2^-20); where fp32 torch itself is off by O(1) on some samples (bridge_norm: exp
overflows), the samples fp32 serves are also held to their own bound.  Every case runs twice, bit-equal.
profiles/link_wide_instances.md has every case as measured on an MI355X.

mc with the full covariance is served, and held here, up to LK_LINK_WIDE_MAX_C_FULL = 224 classes."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_gpu_link import DEV, FLOOR, bound_and_errors, link_ref, make_inputs  # noqa: E402

pytestmark = pytest.mark.gpu


def diag_inputs(C, B, n, seed):
    """marginal variances (0.1 + U(0, 1)) 2^k, k in {-6, 0, 4} by sample; f_mu ~ 3 N(0, 1); z ~ N(0, 1): fp32 values in fp64"""
    g = torch.Generator().manual_seed(2000 + seed)
    k = torch.tensor([(-6.0, 0.0, 4.0)[(b + seed) % 3] for b in range(B)], dtype=torch.float64)
    var = (0.1 + torch.rand(B, C, generator=g, dtype=torch.float64)) * torch.exp2(k).view(B, 1)
    return (3 * torch.randn(B, C, generator=g)).double(), var.float().double(), torch.randn(C, n, generator=g).double()


def run_wide(f_mu, f_var, z, link, diag, slabs=None):
    """the kernel on fp32 device copies, its outputs inside guard bands, with a workspace of `slabs` slabs if given"""
    from laplace_amd._lib import get_kernels

    B, C = f_mu.shape
    pbuf = torch.full((B * C + 128,), float("nan"), device=DEV)
    ibuf = torch.full((B + 8,), -7, dtype=torch.int32, device=DEV)
    dev = lambda t: t.float().to(DEV).contiguous()  # noqa: E731
    work = None if slabs is None else torch.empty(slabs * (32 * ((C + 31) // 32)) ** 2, device=DEV)
    probs, info = get_kernels().glm_link_wide(dev(f_mu), dev(f_var), dev(z) if link == "mc" else None, link, diag,
                                              probs=pbuf[64:64 + B * C].view(B, C), info=ibuf[4:4 + B], work=work)
    assert torch.isnan(pbuf[:64]).all() and torch.isnan(pbuf[64 + B * C:]).all(), "a write outside probs"
    assert (ibuf[:4] == -7).all() and (ibuf[4 + B:] == -7).all(), "a write outside info"
    return probs.clone(), info.clone()


# (link, C, B, n_samples, diag, slabs of the workspace or None for the size the library asks for)
CASES = [
    ("mc", 193, 5, 17, 0, None),   # first wide C: one-row remainder of the 32-panel, partial 16-tile, draw-stage remainder
    ("mc", 224, 2, 16, 0, None),   # exact panels and an exact stage
    ("mc", 193, 5, 17, 0, 2),      # the persistent loop reuses a slab
    ("mc", 193, 2, 16, 1, None),
    ("mc", 257, 2, 3, 1, None),    # scalar draw loads
    ("mc", 1000, 2, 100, 1, None),
    ("mc", 4096, 3, 17, 1, None),  # 16 classes per thread, the limit
    ("probit", 193, 5, 1, 0, None),
    ("probit", 4096, 3, 1, 1, None),
    ("bridge", 193, 5, 1, 0, None),
    ("bridge", 1000, 2, 1, 0, None),
    ("bridge", 2080, 1, 1, 0, None),  # 64 column sums per lane, more than 48 KiB of LDS
    ("bridge_norm", 257, 5, 1, 0, None),
    ("bridge", 300, 5, 1, 1, None),
]


@pytest.mark.parametrize("link,C,B,n,diag,slabs", CASES, ids=lambda v: str(v))
def test_link_wide_against_fp64(link, C, B, n, diag, slabs):
    f_mu, f_var, z = diag_inputs(C, B, n, seed=C + n) if diag else make_inputs(C, B, n, seed=C + n)
    probs, info = run_wide(f_mu, f_var, z, link, diag, slabs)
    err, tol, e32, sane = bound_and_errors(f_mu, f_var, z, link, diag, probs)
    print(f"| {link} | {C} | {B} | {n} | {diag} | {slabs} | {err:.3e} | {tol:.3e} | {e32:.3e} |")
    assert not info.any() and torch.isfinite(probs).all()
    assert err <= tol, f"worst error {err:.3e} over the bound {tol:.3e} (torch fp32: {e32:.3e})"
    if not sane.all():  # fp32 torch itself is off by O(1) on some samples (exp overflows): the others against their own bound
        err, tol, e32, _ = bound_and_errors(f_mu, f_var, z, link, diag, probs, rows=sane)
        print(f"| {link}, the {int(sane.sum())} samples fp32 serves | {C} | {B} | {n} | {diag} | {slabs} | {err:.3e} | {tol:.3e} | {e32:.3e} |")
        assert sane.any() and err <= tol, f"worst error {err:.3e} over the bound {tol:.3e} (torch fp32: {e32:.3e})"
    again, _ = run_wide(f_mu, f_var, z, link, diag, slabs)
    assert torch.equal(probs, again), "two equal calls differ"


def test_a_factorisation_that_fails_is_reported_per_sample():
    from laplace_amd.laplace import HipLaplace

    C = 200
    f_mu, V, z = make_inputs(C, 5, 17, seed=C)
    w, Q = torch.linalg.eigh(V[2])
    w[C // 2] = -0.5
    V[2] = ((Q * w) @ Q.T).float().double()
    V[2] = torch.tril(V[2]) + torch.tril(V[2], -1).T
    probs, info = run_wide(f_mu, V, z, "mc", 0, slabs=2)  # (the workgroup of sample 2 goes on to sample 4)
    assert info[2] != 0 and not info[[0, 1, 3, 4]].any()
    assert torch.isnan(probs[2]).all()
    good = [0, 1, 3, 4]
    err, tol, e32, _ = bound_and_errors(f_mu[good], V[good], z, "mc", 0, probs[good])
    print(f"| mc, sample 2 indefinite | {C} | 5 | 17 | 0 | 2 | {err:.3e} | {tol:.3e} | {e32:.3e} |")
    assert err <= tol
    la = HipLaplace(torch.nn.Linear(4, C).to(DEV), "classification", "all", "kron")
    la.use_link_wide_kernels = True
    la._glm_predictive_distribution = lambda x, diagonal_output=False: (f_mu.float().to(DEV), V.float().to(DEV))
    with pytest.raises(torch.linalg.LinAlgError, match="not positive-definite"):
        la(torch.zeros(5, 4, device=DEV), link_approx="mc", n_samples=17)


@pytest.mark.parametrize("structure", ["kron", "diag"])
def test_the_predictive_with_the_wide_kernels_on_and_off(structure):
    from torch import nn
    from torch.utils.data import DataLoader, TensorDataset

    from laplace_amd.laplace import HipLaplace

    torch.manual_seed(3)
    C, B = 200, 6
    model = nn.Sequential(nn.Linear(6, 8), nn.Tanh(), nn.Linear(8, C)).to(DEV)
    X, y = torch.randn(B, 6, device=DEV), torch.randint(C, (B,), device=DEV)
    la = HipLaplace(model, "classification", "all", structure, prior_precision=0.5)
    la.fit(DataLoader(TensorDataset(X, y), batch_size=B))
    f_mu, f_var = (t.double().cpu() for t in la._glm_predictive_distribution(X))
    f_dg = la._glm_predictive_distribution(X, diagonal_output=True)[1].double().cpu()
    z = torch.randn(C, 33, device=DEV, generator=torch.Generator(DEV).manual_seed(11)).double().cpu()
    asked, inner = [], la._glm_predictive_distribution
    la._glm_predictive_distribution = lambda x, diagonal_output=False: (asked.append(diagonal_output), inner(x, diagonal_output))[1]
    for link, diag in (("probit", False), ("mc", True), ("mc", False), ("bridge", False)):
        out = {}
        for on in (True, False):
            la.use_link_wide_kernels = on
            del asked[:]
            out[on] = la(X, link_approx=link, n_samples=33, diagonal_output=diag, generator=torch.Generator(DEV).manual_seed(11))
            if link == "probit":
                assert asked == [on], f"probit with the switch {on} asked for diagonal_output = {asked}"
        p64 = link_ref(f_mu, f_dg if diag else f_var, z, link, int(diag))
        err, e32 = ((out[on].double().cpu() - p64).abs().max().item() for on in (True, False))
        assert err <= max(4 * e32, FLOOR), f"{link}, diagonal_output {diag}: {err:.3e} with the kernel, {e32:.3e} with torch"
