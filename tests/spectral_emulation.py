"""torch restatements of the spectral dense-Laplace kernels (csrc/lk_spectral.hip) and of the one form of ``lk_gemm_f32`` the
spectral route calls, for the ``not gpu`` tests of the host logic (tests/test_spectral_laplace.py)."""
from __future__ import annotations

import torch

from tests.test_prior_grid import GridKernels


class SpectralEmulatedKernels(GridKernels):
    SP_QUAD_LL, SP_GRID_LL, SP_QUAD_R, SP_GRID_R, SP_BIAS = 0, 1, 2, 3, 4

    def __init__(self):
        self.calls = []  # names of the spectral / eigensolver calls, in order
        self.fail_syevj = 0

    def syevj(self, A, clamp=True, max_sweeps=0):
        self.calls.append("syevj")
        w, Q, info = super().syevj(A, clamp, max_sweeps)
        if self.fail_syevj > 0:  # the next solves report "sweeps ran out"
            self.fail_syevj -= 1
            info = info.clone()
            info[0] = 1
        return w, Q, info

    def spectral_variant(self, form, N, C, D_or_P, G=1, aligned=True):
        ll = (form & 3) in (0, 1)
        if ll and D_or_P > 896:
            return None
        return {"ll": ll}

    def gemm(self, A, B, C, batch, M, N, Kd, lda, ldb, ldc, sa=0, sb=0, sc=0, ta=False, tb=False, E=None, lde=0,
             alpha=1.0, accumulate=False):
        assert batch == 1 and not ta and E is None and not accumulate and lda == Kd and ldc == N
        a = A.reshape(-1)[:M * Kd].reshape(M, Kd)
        b = B.reshape(-1)[:N * Kd].reshape(N, Kd).T if tb else B.reshape(-1)[:Kd * N].reshape(Kd, N)
        C.reshape(-1)[:M * N].copy_((alpha * (a @ b)).reshape(-1))

    @staticmethod
    def _rotate_ll(phi, Q, C, has_bias):
        B, D = phi.shape
        R = torch.einsum("nd,cdj->ncj", phi, Q[:C * D].reshape(C, D, -1))
        return R + Q[C * D:][None] if has_bias else R

    def spectral_quadform(self, R, lam, hfac, delta):
        self.calls.append("spectral_quadform")
        return torch.einsum("ncj,nkj,j->nck", R, R, 1.0 / (hfac * lam + delta.reshape(())))

    def spectral_grid(self, R, lam, hfac, deltas, var):
        self.calls.append("spectral_grid")
        var += torch.einsum("ncj,gj->gnc", R * R, 1.0 / (hfac * lam[None, :] + deltas[:, None]))
        return var

    def spectral_quadform_ll(self, phi, Q, lam, hfac, delta, C, has_bias):
        self.calls.append("spectral_quadform_ll")
        R = self._rotate_ll(phi, Q, C, has_bias)
        return torch.einsum("ncj,nkj,j->nck", R, R, 1.0 / (hfac * lam + delta.reshape(())))

    def spectral_grid_ll(self, phi, Q, lam, hfac, deltas, C, has_bias, var):
        self.calls.append("spectral_grid_ll")
        R = self._rotate_ll(phi, Q, C, has_bias)
        var += torch.einsum("ncj,gj->gnc", R * R, 1.0 / (hfac * lam[None, :] + deltas[:, None]))
        return var
