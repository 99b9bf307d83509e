"""The joint-covariance kernels of an nn.Linear layer (csrc/lk_joint.hip) against the formula in fp64,
  cov[(n,c),(m,k)] += sum_oi u[c,n,o] u[k,m,o] v[n,i] v[m,i] w[o,i] + sum_o ub[c,n,o] ub[k,m,o] bw[o],
element-wise within (K + 16) 2^-24 A, A the fp64 sum of the absolute values of the element's terms (its previous value included).
K, the longest chain of fp32 additions behind one element: Di in the accumulator of the matrix instruction (one per i), 5 levels of
the butterfly over the 32 o of a tile, at most ceil(Do / 32) + 1 for the running sums over the Do tiles (within a workgroup, then
over the splits), 1 for the bias block and 1 for `cov +=`: K = Di + ceil(Do / 32) + 8.  The 16 covers the roundings of the factors:
v v, u u and their product with T one each, w three (product, sum, reciprocal).
Then `la(X, joint=True)` end to end with the Jacobian routes patched to raise, against the oracle at the project's parity bar.
profiles/joint_instances.md has every case as measured on an MI355X."""
import copy
import functools
import os
import sys

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV, U = "cuda", 2.0 ** -24
# (B, C, Do, Di, delta, the variant the shape must take): pair tiles of 16 samples, Do tiles of 32, Di chunks of 128
CASES = [
    (1, 1, 1, 1, 1e-3, dict(tier=1, splits=1)),
    (15, 2, 31, 127, 1e2, dict(tier=2, splits=1)),      # one below the pair tile, the Do tile and the Di chunk
    (16, 3, 33, 129, 1e-3, dict(tier=4, splits=2)),     # at the pair tile, C between tiers, one above the tile and the chunk
    (17, 4, 65, 6, 1e2, dict(tier=4, splits=3)),        # one above: a diagonal and an off-diagonal block; Di % 4 != 0
    (33, 1, 33, 130, 1e-3, dict(tier=1, splits=2)),     # six pair blocks, a 2-column chunk tail
    (250, 1, 250, 5, 1e-3, dict(tier=1, splits=4)),     # two Do tiles per split, four splits through the workspace
    (500, 1, 65, 6, 1e2, dict(tier=1, splits=1)),       # enough pair blocks: a workgroup walks all three Do tiles
]
MODES = [(m, b) for m in ("kron", "diag") for b in (True, False)]


@functools.lru_cache(maxsize=None)
def make_case(B, C, Do, Di, delta):
    """fp32 operands of both modes, the symmetric non-zero start of cov, and per (mode, bias) the fp64 result and bound"""
    g = torch.Generator().manual_seed(1000 * B + 10 * Do + C)
    u, v, ub = torch.randn(C, B, Do, generator=g), torch.randn(B, Di, generator=g), torch.randn(C, B, Do, generator=g)
    ls = [10.0 ** (6 * torch.rand(n, generator=g) - 3) for n in (Do, Di, Do)]  # log-uniform over six decades
    for l in ls:
        l[::5] = 0.0  # clamped factors
    l1, l2, lb = ls
    d = torch.tensor([delta])
    var_w, var_b = 10.0 ** (4 * torch.rand(Do, Di, generator=g) - 4), 10.0 ** (4 * torch.rand(Do, generator=g) - 4)
    c0 = torch.randn(B * C, B * C, generator=g)
    c0 = c0 + c0.T
    want = {}
    for mode, bias in MODES:
        w = 1.0 / (torch.outer(l1.double(), l2.double()) + delta) if mode == "kron" else var_w.double()
        bw = 1.0 / (lb.double() + delta) if mode == "kron" else var_b.double()
        uu, bb = u.double(), (ub if mode == "kron" else u).double()
        val, A = c0.double().clone(), c0.double().abs()
        for x, y, f in ((uu, v.double(), lambda t: t), (uu.abs(), v.double().abs(), torch.abs)):
            T = torch.einsum("ni,mi,oi->nmo", y, y, w)
            t = torch.einsum("cno,kmo,nmo->ncmk", x, x, T)
            if bias:
                t = t + torch.einsum("cno,kmo,o->ncmk", f(bb), f(bb), bw)
            (val if x is uu else A).add_(t.reshape(B * C, B * C))
        want[mode, bias] = (val, (Di + (Do + 31) // 32 + 8 + 16) * U * A)
    return dict(u=u, v=v, ub=ub, l1=l1, l2=l2, lb=lb, d=d, var_w=var_w, var_b=var_b, c0=c0), want


def run_kernel(ops, mode, bias, B, C, Do, Di):
    """cov after one call on the NaN-guarded buffers, and whether the guard bands of cov and the workspace are untouched"""
    from laplace_amd._lib import get_kernels

    K, o = get_kernels(), {k: t.to(DEV) for k, t in ops.items()}
    N, need = B * C, int(K.lib.lk_joint_linear_workspace_bytes(B, C, Do, Di)) // 4
    cbuf, wbuf = torch.full((N * N + 128,), float("nan"), device=DEV), torch.full((need + 128,), float("nan"), device=DEV)
    cov, work = cbuf[64:-64].view(N, N), wbuf[64:-64] if need else None
    cov.copy_(o["c0"])
    if mode == "kron":
        K.kron_joint_linear(o["u"], o["v"], o["l1"], o["l2"], o["d"], cov, *((o["ub"], o["lb"], o["d"]) if bias else ()), work=work)
    else:
        K.diag_joint_linear(o["v"], o["u"], o["var_w"].reshape(-1), o["var_b"] if bias else None, cov, work=work)
    assert all(torch.isnan(b[:64]).all() and torch.isnan(b[-64:]).all() for b in (cbuf, wbuf)), "a write outside cov or the workspace"
    return cov.clone()


@pytest.mark.gpu
@pytest.mark.parametrize("mode,bias", MODES)
@pytest.mark.parametrize("B,C,Do,Di,delta,variant", CASES, ids=lambda v: str(v) if not isinstance(v, dict) else "")
def test_joint_kernels_against_fp64(B, C, Do, Di, delta, variant, mode, bias):
    from laplace_amd._lib import get_kernels

    assert get_kernels().joint_linear_variant(mode, B, C, Do, Di) == variant
    ops, want = make_case(B, C, Do, Di, delta)
    val, tol = want[mode, bias]
    cov = run_kernel(ops, mode, bias, B, C, Do, Di)
    ratio = ((cov.double().cpu() - val).abs() / tol).max().item()
    print(f"| {B} | {C} | {Do} | {Di} | {delta:g} | {mode} | {int(bias)} | {variant['splits']} | {ratio:.3f} |")
    assert ratio <= 1.0, f"worst error {ratio:.3f} of its bound"
    assert torch.equal(cov, cov.T), "cov is not exactly symmetric"
    again = run_kernel(ops, mode, bias, B, C, Do, Di)
    assert torch.equal(cov.view(torch.int32), again.view(torch.int32)), "two equal calls differ"


def _models(name):
    from tests.conftest import golden_model, load_golden

    if name == "mlp":
        return golden_model("mlp", load_golden("mlp", "regression"), dtype=torch.float32, device=DEV)
    torch.manual_seed(3)  # the block branch: a convolution in front of two Linear layers
    model = nn.Sequential(nn.Conv2d(3, 4, 2, 2), nn.Flatten(), nn.Tanh(), nn.Linear(16, 20), nn.Tanh(), nn.Linear(20, 2)).to(DEV)
    return model, torch.randn(6, 3, 5, 5, device=DEV), torch.randn(6, 2, device=DEV)


def rel(got, want):
    return ((got.double().cpu() - want).abs().max() / want.abs().max()).item()


@pytest.mark.gpu
@pytest.mark.parametrize("sow", ["all", "last_layer"])
@pytest.mark.parametrize("hs", ["kron", "diag"])
@pytest.mark.parametrize("name", ["mlp", "conv"])
def test_joint_predictive_without_jacobians(name, hs, sow, monkeypatch):
    from torch.utils.data import DataLoader, TensorDataset

    from laplace_amd.laplace import HipLaplace
    from oracle import curvature_oracle as co

    model, X, y = _models(name)
    m64 = copy.deepcopy(model).double().cpu()
    la = HipLaplace(model, "regression", sow, hs, prior_precision=0.7)
    la.fit(DataLoader(TensorDataset(X, y), batch_size=5))
    la.use_joint_kernels = True

    def refuse(*a, **kw):
        raise AssertionError("the joint predictive asked for the materialised Jacobians")

    monkeypatch.setattr(la.backend, "jacobians", refuse)
    monkeypatch.setattr(la.backend, "last_layer_jacobians", refuse)
    f_mu, cov = la(X, joint=True)
    params = list(m64.parameters()) if sow == "all" else list(list(m64.children())[-1].parameters())
    Js, f = co.jacobians(m64, X.double().cpu(), params)
    (B, C, P), Js = Js.shape, Js.reshape(1, -1, Js.shape[-1])
    if hs == "kron":
        post, d64 = la.posterior_precision, lambda blocks: [[t.double().cpu() for t in b] for b in blocks]  # noqa: E731
        want = co.krondecomposed_inv_square_form(d64(post.eigenvectors), d64(post.eigenvalues), post.deltas.double().cpu(), Js)[0]
    else:
        want = torch.einsum("np,p,mp->nm", Js[0], la.posterior_variance.double().cpu(), Js[0])
    assert cov.shape == (B * C, B * C) and rel(cov, want) < 1e-4 and rel(f_mu, f.flatten()) < 1e-4, (rel(cov, want), rel(f_mu, f.flatten()))
    blocks = torch.stack([cov[i * C:(i + 1) * C, i * C:(i + 1) * C] for i in range(B)])
    assert rel(blocks, la(X)[1].double().cpu()) < 1e-4
