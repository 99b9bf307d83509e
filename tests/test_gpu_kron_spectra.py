"""The eigenvalue algebra of the Kron posterior on the spectra KFAC factors really have (tests/kronalg_fixtures.py), on the
MI355X (-m gpu): ``kron_pow`` and ``kron_sandwich`` called directly, ``kron_logdet`` / ``kron_logdet_blocks`` with their
derivatives, and every quadratic form of the GLM predictive with samples whose scales lie 2^40 apart in one batch, each
sample measured against its own largest entry.  Eigenvalues graded over many decades, rank 1 and rank 0, scaled by 2^-20
and 2^16; ``delta`` from 1e-4 to 1e4.  A plain fp32 evaluation on the CPU meets every bound on every case
(tests/test_kronalg_fixtures.py).

LK_TEST_DEVICE=cpu runs the bodies against the CPU restatement of the kernels in fp64 (a self-check of this file on a
GPU-less box); the real run uses the HIP library on cuda:0."""
import os

import pytest
import torch

from tests import kronalg_fixtures as KF
from tests.parity_log import record_error

pytestmark = pytest.mark.gpu

DEV = os.environ.get("LK_TEST_DEVICE", "cuda")


@pytest.fixture(scope="module")
def K():
    if DEV == "cpu":
        return KF.GridKernels()
    from laplace_amd._lib import HipKernels

    return HipKernels()


def _dev(t64):
    """what the kernels read: fp32 on the device (every fixture value is an fp32 number); the emulation keeps fp64"""
    return t64.double().clone() if DEV == "cpu" else t64.float().to(DEV).contiguous()


def _assert(w):
    assert w, "nothing was measured"
    for name, value in w.items():  # logged and printed before anything is asserted
        record_error(value, name)
        print(f"{name}: {value:.2e} (bound {KF.bound_of(name):g})")
    for name, value in w.items():
        assert value < KF.bound_of(name), f"{name}: {value:.2e} >= {KF.bound_of(name):g}"


@pytest.mark.parametrize("n1,n2", KF.SIZES)
@pytest.mark.parametrize("family", KF.FAMILIES)
def test_kron_pow(K, family, n1, n2):
    _assert(KF.check_pow(K, _dev, family, n1, n2))


@pytest.mark.parametrize("n1,n2", KF.SIZES)
@pytest.mark.parametrize("family", KF.FAMILIES)
def test_kron_logdet(K, family, n1, n2):
    _assert(KF.check_logdet(K, _dev, family, n1, n2))


@pytest.mark.parametrize("scale", [None, 2.0 ** -10, 5e4])
def test_kron_logdet_blocks(K, scale):
    _assert(KF.check_logdet_blocks(K, _dev, scale))


@pytest.mark.parametrize("pi,po", KF.SANDWICH_SIZES)
@pytest.mark.parametrize("family", KF.FAMILIES)
def test_kron_sandwich(K, family, pi, po):
    _assert(KF.check_sandwich(K, _dev, family, pi, po))


@pytest.mark.parametrize("shape", KF.LINEAR_SHAPES, ids=str)
@pytest.mark.parametrize("family", KF.FAMILIES)
def test_linear_quadforms(K, family, shape):
    _assert(KF.check_quad_linear(K, _dev, family, shape))


@pytest.mark.parametrize("shape", KF.LINEAR_SHAPES, ids=str)
@pytest.mark.parametrize("family", KF.FAMILIES)
def test_linear_grid(K, family, shape):
    _assert(KF.check_grid_linear(K, _dev, family, shape))


@pytest.mark.parametrize("shape", KF.SHARED_SHAPES, ids=str)
@pytest.mark.parametrize("family", KF.FAMILIES)
def test_shared_quadforms_and_grid(K, family, shape):
    _assert(KF.check_quad_shared(K, _dev, family, shape))
