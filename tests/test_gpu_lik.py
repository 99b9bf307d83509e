"""The likelihood kernels of csrc/lk_lik.hip on the batches of tests/lik_fixtures.py, on the MI355X (-m gpu): both roots of
the softmax Hessian and the two loss sums against fp64, each SAMPLE's root and each sample's S S^T normalised by that
sample's own largest expected entry -- a saturated row next to an unsaturated one is measured at its own scale, six or more
decades below -- and the loss accumulated onto a non-zero ``loss_accum``.  Every figure is below 1e-5, the bound a careful
fp32 evaluation meets on every one of these cases (tests/test_lik_fixtures.py).

LK_TEST_DEVICE=cpu runs the bodies against the CPU restatement of the kernels (a self-check of this file on a GPU-less
box); the real run uses the HIP library on cuda:0."""
import os

import pytest
import torch

from tests import lik_fixtures as LF
from tests.emulated_kernels import EmulatedKernels
from tests.lik_fixtures import BOUND
from tests.parity_log import record_error

pytestmark = pytest.mark.gpu

DEV = os.environ.get("LK_TEST_DEVICE", "cuda")
CASES = {False: LF.cases(False), True: LF.cases(True)}


@pytest.fixture(scope="module")
def K():
    if DEV == "cpu":
        return EmulatedKernels()
    from laplace_amd._lib import HipKernels

    return HipKernels()


def _sync():
    if DEV != "cpu":
        torch.cuda.synchronize()


def _dev(t64):
    """what the kernels read: fp32 on the device (every fixture value is an fp32 number); the emulation keeps fp64"""
    return t64.double() if DEV == "cpu" else t64.float().to(DEV).contiguous()


def _root(K, case, cholesky):
    B, C = case.f.shape
    acc = _dev(torch.tensor([LF.LOSS_BASE], dtype=torch.float64))
    before = acc.clone()
    y = case.y.to(DEV)
    S = K.softmax_hess_sqrt(_dev(case.f), y, acc, cholesky=cholesky)
    _sync()
    what = f"{'cholesky' if cholesky else 'symmetric'} root {case.name}"
    assert tuple(S.shape) == ((C - 1 if cholesky else C), B, C)
    assert LF.structure_ok(S, C, cholesky), f"{what}: C{' - 1' if cholesky else ''} seeds, zero above the diagonal"
    root, lam, loss = LF.errors(case, cholesky, S, acc.item())
    tag = "chol" if cholesky else "sym"
    record_error(root, f"{tag} root per sample")
    record_error(lam, f"{tag} S S^T per sample")
    print(f"{what}: root {root:.2e} S S^T {lam:.2e} loss {'-' if loss is None else format(loss, '.2e')}")
    if loss is not None:
        record_error(loss, f"{tag} loss")
    assert root < BOUND, f"{what}: a sample's root is off by {root:.2e} of its own largest entry"
    assert lam < BOUND, f"{what}: a sample's S S^T is off by {lam:.2e} of its own largest entry"
    if loss is None:
        assert torch.equal(acc, before), f"{what}: no valid label, loss_accum must come back bit for bit"
    else:
        assert loss < BOUND, f"{what}: loss off by {loss:.2e}"


@pytest.mark.parametrize("case", CASES[False], ids=repr)
def test_symmetric_root(K, case):
    _root(K, case, False)


@pytest.mark.parametrize("case", CASES[True], ids=repr)
def test_cholesky_root(K, case):
    _root(K, case, True)


def test_root_without_labels_or_accumulator(K):
    """the loss is optional: the same root, bit for bit, with no labels and with labels but no accumulator"""
    case = LF.batch(5, 10, 60)
    for cholesky in (False, True):
        acc = _dev(torch.tensor([LF.LOSS_BASE], dtype=torch.float64))
        y = case.y.clamp(min=0).to(DEV)
        S = K.softmax_hess_sqrt(_dev(case.f), y, acc, cholesky=cholesky)
        S0 = K.softmax_hess_sqrt(_dev(case.f), None, None, cholesky=cholesky)
        S1 = K.softmax_hess_sqrt(_dev(case.f), y, None, cholesky=cholesky)
        assert torch.equal(S, S0) and torch.equal(S, S1)


@pytest.mark.parametrize("kind", LF.SQ_KINDS)
@pytest.mark.parametrize("numel", LF.SQ_NUMELS)
def test_sq_err_sum(K, numel, kind):
    f, y = LF.sq_case(numel, kind)
    acc = _dev(torch.tensor([LF.LOSS_BASE], dtype=torch.float64))
    before = acc.clone()
    K.sq_err_sum(_dev(f), _dev(y), LF.SQ_SCALE, acc)
    want = LF.sq_reference(f, y)
    if kind == "equal":
        assert want == 0 and torch.equal(acc, before), "targets equal to predictions: exactly nothing is added"
        return
    e = record_error(LF.loss_err(acc.item(), LF.LOSS_BASE + want), "sq_err")
    print(f"sq_err_sum numel={numel} {kind}: {e:.2e}")
    assert e < BOUND, f"sq_err_sum numel={numel} {kind}: off by {e:.2e}"
