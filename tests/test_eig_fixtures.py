"""The eigensolver fixtures (tests/eig_fixtures.py) are well-posed for an fp32 solver: fp32 LAPACK on the CPU meets the
bound that tests/test_gpu_eigensolver.py asks of ``lk_syevj_f32`` on every family, size and scale -- so a failure on the
device is the kernel's, not the input's."""
import pytest
import torch

from tests.eig_fixtures import BOUND, FAMILIES, SIZES, eig_errors, lapack_errors, scaled, spectrum


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family", FAMILIES)
def test_fp32_lapack_meets_the_bound(family, n):
    for k in (-60, 0, 60):
        val, orth, rec = lapack_errors(family, n, k)
        print(f"{family} n={n} k={k}: val {val:.2e} orth {orth:.2e} rec {rec:.2e}")
        assert val < BOUND and orth < BOUND and rec < BOUND, (family, n, k, val, orth, rec)


@pytest.mark.parametrize("family", FAMILIES)
def test_fixture_is_what_it_says(family):
    n = 65
    A = spectrum(family, n)
    assert A.dtype == torch.float64 and A.shape == (n, n) and torch.equal(A, A.T)
    assert torch.equal(A, spectrum(family, n)), "seeded: the same matrix every time"
    lam = torch.linalg.eigvalsh(A)
    want = {"graded": (1e-6, 1.0), "indefinite": (-1.0, 2.0), "pairs": (1.0, 33.0), "identity": (1.0, 1.0), "zero": (0.0, 0.0),
            "ones": (0.0, float(n))}.get(family)
    if want is not None:
        assert abs(lam[0].item() - want[0]) < 1e-9 * max(1.0, abs(want[1])) and abs(lam[-1].item() - want[1]) < 1e-9 * max(1.0, want[1])
    if family == "spiked":
        assert lam[-1] > 0.5 * n * lam[-2], "one eigenvalue ~ n x the bulk"
    if family == "dscaled":
        d = A.diagonal()
        assert d.max() / d.min() > 1e5, "rows span six decades"
    if family == "pairs":
        gaps = (lam[1::2] - lam[0:-1:2]) / lam[0:-1:2]
        assert (gaps - 1e-7).abs().max() < 1e-9


def test_eig_errors_sees_a_wrong_solve():
    """the three figures are zero for the fp64 solve and each reacts to its own kind of damage"""
    A = spectrum("indefinite", 33)
    w, Q = torch.linalg.eigh(A)
    assert max(eig_errors(A, w, Q, clamp=False)) < 1e-13
    val, orth, rec = eig_errors(A, w.clamp(min=0), Q, clamp=True)
    assert val < 1e-13 and orth < 1e-13 and rec > 0.1  # (a clamped solve does not reconstruct an indefinite matrix)
    w2 = w.clone()
    w2[5] += 1e-4
    assert eig_errors(A, w2, Q, clamp=False)[0] > 4e-5
    Q2 = Q.clone()
    Q2[:, 3] *= 1 + 1e-4
    assert eig_errors(A, w, Q2, clamp=False)[1] > 1e-4
    # a power-of-two scale is exact and moves nothing
    assert eig_errors(scaled(A, 60), scaled(w, 60), Q, clamp=False) == eig_errors(A, w, Q, clamp=False)
