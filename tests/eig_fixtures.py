"""Seeded fp64 symmetric matrices with the spectra, sizes and scales that KFAC factors have, for the eigensolver tests
(tests/test_eig_fixtures.py pins them as well-posed for an fp32 solver on the CPU; tests/test_gpu_eigensolver.py holds
``lk_syevj_f32`` to the same bounds on the device).

TEST INFRASTRUCTURE, in the style of tests/gconv_fixtures.py and tests/norm_fixtures.py: everything is built on the CPU in
fp64 from fixed seeds, nothing needs a GPU.  ``Q`` below is a seeded random orthogonal matrix (QR of a Gaussian matrix).

  * ``spiked``     X = randn(3n+5, n) + 3, X^T X / (3n): one eigenvalue ~ n x the bulk (a mean-shifted activation factor,
                   the case the power-iteration scale of csrc/lk_eigh.hip exists for)
  * ``graded``     Q diag(logspace(0, -6, n)) Q^T
  * ``dscaled``    D W D, W Wishart, D = diag(logspace(0, -3, n)): rows span six decades (an A factor whose input
                   channels are not normalised)
  * ``indefinite`` Q diag(linspace(-1, 2, n)) Q^T
  * ``pairs``      Q diag(l) Q^T, l_2k = k+1, l_2k+1 = (k+1)(1 + 1e-7): eigenvalue pairs closer than fp32 resolves
  * ``identity``, ``zero``: every eigenvalue tied;  ``ones``: rank 1 (lambda = n) with exact zeros elsewhere
"""
from __future__ import annotations

import torch

FAMILIES = ("spiked", "graded", "dscaled", "indefinite", "pairs", "identity", "zero", "ones")
SIZES = (2, 32, 33, 63, 64, 65, 127, 129, 193, 257)
#: every family is solved with clamp=True (what Kron.decompose passes) except the one with negative eigenvalues
CLAMPED = {f: f != "indefinite" for f in FAMILIES}
#: the project's bound on each of (val, orth, rec) (``_eig_checks`` of tests/test_gpu_kernels.py)
BOUND = 5e-6


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def orthogonal(n: int, seed: int) -> torch.Tensor:
    Q, _ = torch.linalg.qr(_randn(n, n, seed=seed))
    return Q


def wishart(n: int, seed: int | None = None) -> torch.Tensor:
    """X^T X / (3n), X = randn(3n+5, n): the O(1), well-conditioned PSD matrix of ``test_syevj_psd``"""
    X = _randn(3 * n + 5, n, seed=n if seed is None else seed)
    return X.T @ X / (3 * n)


def _from_spectrum(lam: torch.Tensor, seed: int) -> torch.Tensor:
    Q = orthogonal(lam.numel(), seed)
    return (Q * lam) @ Q.T


def spectrum(family: str, n: int) -> torch.Tensor:
    """the symmetric fp64 [n, n] matrix of ``family`` (seeded by the family and n: the same matrix in every test)"""
    A = _build(family, n)
    return (A + A.T) / 2  # exactly symmetric: the solver reads the upper triangle, the fp64 reference the lower


def _build(family: str, n: int) -> torch.Tensor:
    seed = 1000 * (FAMILIES.index(family) + 1) + n
    if family == "spiked":
        X = _randn(3 * n + 5, n, seed=seed) + 3.0
        return X.T @ X / (3 * n)
    if family == "graded":
        return _from_spectrum(torch.logspace(0, -6, n, dtype=torch.float64), seed)
    if family == "dscaled":
        d = torch.logspace(0, -3, n, dtype=torch.float64)
        return d[:, None] * wishart(n, seed) * d[None, :]
    if family == "indefinite":
        return _from_spectrum(torch.linspace(-1, 2, n, dtype=torch.float64), seed)
    if family == "pairs":
        k = torch.arange(n, dtype=torch.float64) // 2 + 1
        lam = torch.where(torch.arange(n) % 2 == 1, k * (1 + 1e-7), k)
        return _from_spectrum(lam, seed)
    if family == "identity":
        return torch.eye(n, dtype=torch.float64)
    if family == "zero":
        return torch.zeros(n, n, dtype=torch.float64)
    if family == "ones":
        return torch.ones(n, n, dtype=torch.float64)
    raise ValueError(family)


def scaled(A64: torch.Tensor, k: int) -> torch.Tensor:
    """A * 2^k: exact in fp64 and in fp32 (as long as nothing leaves the normal range)"""
    return torch.ldexp(A64, torch.tensor(k))


def eig_errors(A64: torch.Tensor, w: torch.Tensor, Q: torch.Tensor, clamp: bool = True):
    """(val, orth, rec) of a solve of ``A64``, as ``_eig_checks`` of tests/test_gpu_kernels.py defines them: eigenvalue
    error, max|Q^T Q - I| and max|Q diag(w) Q^T - A|, the first and the last normalised by max|lambda_ref|; the reference is
    the fp64 ``eigvalsh``, clamped at 0 only when the solve clamped."""
    n = A64.shape[0]
    w64, Q64 = w.detach().double().cpu(), Q.detach().double().cpu()
    wref = torch.linalg.eigvalsh(A64)
    if clamp:
        wref = wref.clamp(min=0)
    scale = wref.abs().max().item() or 1.0  # (no additive guard: it would count at 2^-100; the zero matrix is absolute)
    val = (w64 - wref).abs().max().item() / scale
    orth = (Q64.T @ Q64 - torch.eye(n, dtype=torch.float64)).abs().max().item()
    rec = ((Q64 * w64) @ Q64.T - A64).abs().max().item() / scale
    return val, orth, rec


def lapack_errors(family: str, n: int, k: int = 0):
    """(val, orth, rec) of fp32 LAPACK (``torch.linalg.eigh`` on the CPU) on ``spectrum(family, n) * 2^k``: what an fp32
    solver can be asked for on this matrix.  Unclamped (LAPACK does not clamp)."""
    A64 = scaled(spectrum(family, n), k)
    w, Q = torch.linalg.eigh(A64.float())
    return eig_errors(A64, w, Q, clamp=False)
