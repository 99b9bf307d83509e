"""``EmulatedKernels`` plus the product kernel (csrc/lk_mul.hip) in stock torch, for the CPU test tier.

TEST INFRASTRUCTURE.  The stock emulation (tests/emulated_kernels.py) deliberately has no ``mul_vjp``: a ``SeedBatchedSweep`` on it
takes the torch math of the product rule.  ``mul_vjp`` states the kernel's rule through tests/mul_fixtures.torch_math - ``da = g * b``
and ``db = g * a``, summed over the row for a row gate - with the binding's own checks on what belongs together; ``mutant`` selects
one of that function's MUTANTS for tests/test_mul_fixtures.py.  ``seen`` records the calls.
"""
import torch

from tests import mul_fixtures as mf
from tests.emulated_kernels import EmulatedKernels


class EmulatedMulKernels(EmulatedKernels):
    mutant = None

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.seen = []

    def mul_vjp(self, g, a, b, S, b_row, want=(True, True)):
        for t in (g, a, b):
            assert t.dtype == torch.float32 and t.is_contiguous()
        S, b_row, want = int(S), bool(b_row), (bool(want[0]), bool(want[1]))
        assert S >= 1 and any(want) and g.numel() == S * a.numel()
        R = b.numel() if b_row else a.shape[0]
        L = a.numel() // R if R else 1
        assert R * L == a.numel() and (b_row or b.numel() == a.numel())
        self.seen.append(("mul_vjp", "row" if b_row else "full", S, int(R), int(L), want))
        da, db = mf.torch_math(g.reshape(S, R, L), a.reshape(R, L), b.reshape(R) if b_row else b.reshape(R, L), b_row, want, self.mutant)
        if da is not None:
            da = da.reshape(g.shape)
        if db is not None:
            db = db.reshape((S * b.shape[0], *b.shape[1:])) if b_row else db.reshape(g.shape)
        return da, db

    def mul_variant(self, S, R, L, b_row, want=(True, True), aligned=True):
        """the host-only launch plan of the library itself (no device call)"""
        from laplace_amd._lib import HipKernels

        return HipKernels().mul_variant(S, R, L, b_row, want, aligned)
