"""nn.Embedding weights and lone parameters on the device (-m gpu): the three kernels alone (csrc/lk_embed.hip through the C
ABI) on the case table of tests/embed_fixtures.py, the backend and the Laplace classes against the goldens of the unmodified
reference (tools/make_embed_golden.py), and a small TextTransformer against float64 autograd.

Kernel checks, none with a tolerance chosen by hand:
  * sentinel: every element of ``Js`` that is no sum of a non-padding run keeps its bits;
  * integer-valued cotangents in [-8, 8] (every partial sum exact, which the test verifies from the data first): bit-equal to
    the float64 result;
  * full-mantissa data: ``|err| <= gamma_k * sum|terms|`` per element, ``gamma_k = k u / (1 - k u)``, ``u = 2^-24``, with ``k`` the
    number of roundings a term of the fully expanded sum can pass through IN ANY ORDER of summation (a sum of ``m`` terms: at
    most ``m - 1`` additions per term; additions of an exact zero do not round):
      jac    one run of ``n`` positions:                                   k = n - 1
      diag   ``alpha * sum_(s,b) r^2``, ``m`` nonzero (s, b) terms, runs <= L: k = 2 (L - 1) + 1 + (m - 1) + 2   (square; alpha, +=)
      quad   ``sum_(v,d) r_c r_k var``, ``m`` terms, runs <= L:                k = 2 (L - 1) + 2 + (m - 1) + 1   (two products; +=)
    and ``sum|terms|`` the same expression on ``|g|`` (and ``|var|``), all evaluated in float64;
  * two launches on the same data are ``torch.equal``.
Tolerance of the golden comparisons: 1e-4 max-normalised (BASELINE.json north_star), as every golden test here.
``LK_TEST_DEVICE=cpu`` rehearses this file's host logic on the kernel emulation, as tests/test_gpu_backend.py does.
"""
import copy
import os

import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from oracle.make_golden import PRIOR_PREC, SIGMA_NOISE
from tests.embed_fixtures import (EMBED_FIXTURES, KERNEL_CASES, LONE, check_diag_case, check_jac_case, check_quad_case,
                                  ef_gradients_from_golden, forbid_generic_route, golden_model, load_golden, rel)

pytestmark = pytest.mark.gpu
DEV = os.environ.get("LK_TEST_DEVICE", "cuda")
LIKS = ("classification", "regression")
CASES = [(n, l) for n in EMBED_FIXTURES for l in LIKS]
BY_NAME = {c["name"]: c for c in KERNEL_CASES}


@pytest.fixture(autouse=True, scope="module")
def _kernels():
    if DEV != "cpu":
        yield
        return
    from laplace_amd import _lib
    from tests.emulated_embed_kernels import EmulatedEmbedKernels

    prev = _lib.set_kernels_for_testing(EmulatedEmbedKernels())
    yield
    _lib.set_kernels_for_testing(prev)


@pytest.fixture(autouse=True)
def _switch_on(monkeypatch):
    """the route ships opt-in: every test of this file runs with the class default switched on"""
    from laplace_amd.backend import _HipCurvatureMixin

    monkeypatch.setattr(_HipCurvatureMixin, "use_embed_kernels", True)


def check(got, want, tol=1e-4, what=""):
    e = rel(got, want)
    print(f"{what}: {e:.3e}")
    assert e < tol, f"{what}: rel err {e:.3e}"


# ---- 1. the kernels alone (the checks live in tests/embed_fixtures.py, where tests/test_embed_fixtures.py turns mutants on them) ----
def _cases(kernel):
    return [c["name"] for c in KERNEL_CASES if kernel in c["kernels"]]


@pytest.mark.parametrize("name", _cases("jac"))
def test_jac_embed_case(name):
    from laplace_amd._lib import get_kernels

    for integer in (True, False):
        check_jac_case(get_kernels(), BY_NAME[name], DEV, integer)


@pytest.mark.parametrize("name", _cases("diag"))
def test_diag_embed_case(name):
    from laplace_amd._lib import get_kernels

    for integer in (True, False):
        check_diag_case(get_kernels(), BY_NAME[name], DEV, integer)


@pytest.mark.parametrize("name", _cases("quad"))
def test_diag_quadform_embed_case(name):
    from laplace_amd._lib import get_kernels

    for integer in (True, False):
        check_quad_case(get_kernels(), BY_NAME[name], DEV, integer)


def test_empty_batch_is_a_no_op():
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    g = torch.zeros(2, 0, 7, 4, device=DEV)
    ids = torch.zeros(0, 7, dtype=torch.int64, device=DEV)
    h = torch.full((20,), 3.0, device=DEV)
    K.diag_embed(g, ids, 5, None, 1.0, h)
    K.jac_embed(g, ids, 5, None, torch.zeros(0, 2, 20, device=DEV), 0)
    K.diag_quadform_embed(g, ids, 5, None, h.clone(), torch.zeros(0, 2, 2, device=DEV))
    assert bool((h == 3.0).all())


# ---- 2. backend and Laplace against the reference's goldens ---------------------------------------------------------------
@pytest.mark.parametrize("use_sweep", (True, False))
@pytest.mark.parametrize("name,lik", CASES)
def test_backend_against_reference_golden(name, lik, use_sweep):
    from laplace_amd import HipEF, HipGGN

    g = load_golden(name, lik)
    model, X, y = golden_model(name, g, device=DEV)
    b = HipGGN(model, lik)
    b.use_sweep = use_sweep
    assert b._supported() == use_sweep  # (the lone parameter needs the sweep; the tape sends the model to the generic route)
    Js, f = b.jacobians(X)
    check(Js, g["Js"], what="jacobians")
    check(f, g["f"], what="f")
    loss, H = b.full(X, y)
    check(H, g["H_ggn"], what="full GGN")
    check(loss, g["loss"], what="loss")
    check(b.diag(X, y)[1], g["h_ggn"], what="diag GGN")
    e = HipEF(model, lik)
    e.use_sweep = use_sweep
    check(e.full(X, y)[1], g["H_ef"], what="full EF")
    check(e.diag(X, y)[1], g["h_ef"], what="diag EF")
    check(e.gradients(X, y)[0], ef_gradients_from_golden(g, lik), what="EF gradients")


@pytest.mark.parametrize("hs", ("diag", "full"))
@pytest.mark.parametrize("name,lik", CASES)
def test_laplace_all_against_reference_golden(name, lik, hs, monkeypatch):
    """(the backend class is handed over: ``HipLaplace``'s default is bound when laplace.py is imported, and a test module that
    re-derives the boundary classes from the reference's - tests/test_gpu_dropin_reference.py reloads laplace_amd.backend - leaves that
    default on the classes from before the reload, which a switch set on the current class does not reach)"""
    from laplace_amd import HipGGN
    from laplace_amd.laplace import HipLaplace

    g = load_golden(name, lik)
    model, X, y = golden_model(name, g, device=DEV)
    forbid_generic_route(monkeypatch)
    la = HipLaplace(model, lik, "all", hs, backend=HipGGN, prior_precision=PRIOR_PREC, sigma_noise=SIGMA_NOISE if lik == "regression" else 1.0)
    la.fit(DataLoader(TensorDataset(X, y), batch_size=5))
    tag = f"la.all.{hs}"
    check(la.loss, g[f"{tag}.loss"], what="loss")
    check(la.H, g[f"{tag}.H"], what="accumulated H")
    f_mu, f_var = la._glm_predictive_distribution(X)
    check(f_mu, g[f"{tag}.f_mu"], what="f_mu")
    check(f_var, g[f"{tag}.f_var"], what="f_var")
    check(la.log_marginal_likelihood(), g[f"{tag}.marglik"], what="marglik")


@pytest.mark.parametrize("name", EMBED_FIXTURES)
def test_embedding_on_the_tape(name, monkeypatch):
    """lone parameter frozen: the autograd tape serves the embedding with the same kernels"""
    from laplace_amd import HipGGN

    g = load_golden(name, "classification")
    model, X, y = golden_model(name, g, device=DEV)
    getattr(model, LONE[name]).requires_grad_(False)
    off, cols = 0, []
    for n, p in golden_model(name, g)[0].named_parameters():
        if n != LONE[name]:
            cols += list(range(off, off + p.numel()))
        off += p.numel()
    forbid_generic_route(monkeypatch)
    b = HipGGN(model, "classification")
    b.use_sweep = False
    assert b._supported()
    check(b.jacobians(X)[0], g["Js"][:, :, cols], what="jacobians")
    check(b.diag(X, y)[1], g["h_ggn"][cols], what="diag")


# ---- 3. a small TextTransformer against float64 autograd ------------------------------------------------------------------
def test_text_transformer_against_autograd(monkeypatch):
    from laplace_amd import HipGGN
    from laplace_amd.nets import TextTransformer
    from laplace_amd.predictive import glm_variance_diag

    torch.manual_seed(11)
    m64 = TextTransformer(vocab=50, T=8, dim=32, depth=1, heads=1, num_classes=4, freeze_norm=False).double().eval()
    ids = torch.randint(1, 50, (6, 8))
    ids[:, 5] = ids[:, 2]  # a repeated token in every row
    ids[0, 6:] = 0  # padding
    params = [p for p in m64.parameters() if p.requires_grad]
    want = torch.stack([torch.stack([torch.cat([g.flatten() for g in torch.autograd.grad(m64(ids[n:n + 1])[0, c], params)])
                                     for c in range(4)]) for n in range(6)])
    model = copy.deepcopy(m64).float().to(DEV)
    X, y = ids.to(DEV), torch.tensor([0, 1, 2, 3, 0, 1], device=DEV)
    forbid_generic_route(monkeypatch)
    b = HipGGN(model, "classification")
    assert b._supported()
    Js, f = b.jacobians(X)
    assert getattr(b._tape(), "sweep_reason", None) is None
    check(Js, want, what="jacobians")
    p = torch.softmax(m64(ids), -1)
    Hl = torch.diag_embed(p) - p[:, :, None] * p[:, None, :]
    check(b.diag(X, y)[1], torch.einsum("ncp,nck,nkp->p", want, Hl, want), what="diag GGN")
    post_var = torch.rand(want.shape[-1], generator=torch.Generator().manual_seed(2)) + 0.1
    _, fvar = glm_variance_diag(b, X, post_var.to(DEV))
    check(fvar, torch.einsum("ncp,p,nkp->nck", want, post_var.double(), want), what="diagonal predictive")


def test_kron_with_frozen_tokens_equals_the_tape():
    from laplace_amd import HipGGN
    from laplace_amd.nets import TextTransformer

    torch.manual_seed(12)
    model = TextTransformer(vocab=50, T=8, dim=32, depth=1, heads=1, num_classes=4, freeze_embed=True).to(DEV).eval()
    X = torch.randint(0, 50, (6, 8), device=DEV)
    y = torch.tensor([0, 1, 2, 3, 0, 1], device=DEV)
    b = HipGGN(model, "classification")
    loss, kron = b.kron(X, y, N=6)
    tape = b._tape()
    assert getattr(tape, "sweep_reason", None) is None and tape.sweep  # ONE reverse pass
    t = HipGGN(model, "classification")
    t.use_sweep = False
    loss_t, kron_t = t.kron(X, y, N=6)
    assert not getattr(t._tape(), "sweep", None)
    check(loss, loss_t, tol=1e-5, what="loss")
    for i, (F, Ft) in enumerate(zip(kron.kfacs, kron_t.kfacs)):
        for A, At in zip(F, Ft):
            check(A, At, what=f"factor {i}")
