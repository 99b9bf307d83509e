"""``EmulatedKernels`` plus the matrix-product VJP kernel (csrc/lk_matmul.hip) in stock torch, for the CPU test tier, and
``EmulatedEagerAttnKernels``: both kernels of hand-written attention on one object.

TEST INFRASTRUCTURE.  The stock emulation (tests/emulated_kernels.py) deliberately has no ``matmul_vjp``: a ``SeedBatchedSweep`` on it
takes the torch math of the matrix-product rule.  ``matmul_vjp`` states the kernel's rule through
tests/eager_attn_fixtures.matmul_math - ``da = g b^T``, ``db = a^T g`` per seed and sample matrix - with the binding's own checks on
what belongs together; ``matmul_mutant`` selects one of that function's MATMUL_MUTANTS.  ``seen`` records the calls.
"""
import torch

from tests import eager_attn_fixtures as ef
from tests.emulated_kernels import EmulatedKernels
from tests.emulated_softmax_kernels import EmulatedSoftmaxKernels


class EmulatedMatmulKernels(EmulatedKernels):
    matmul_mutant = None

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.seen = []

    def matmul_vjp(self, g, a, b, S, want=(True, True)):
        for t in (g, a, b):
            assert t.dtype == torch.float32 and t.is_contiguous()
        S, want = int(S), (bool(want[0]), bool(want[1]))
        assert a.dim() == b.dim() == g.dim() >= 3 and a.shape[:-2] == b.shape[:-2] and a.shape[-1] == b.shape[-2]
        M, K, N = int(a.shape[-2]), int(a.shape[-1]), int(b.shape[-1])
        NB = a.numel() // (M * K)
        assert S >= 1 and any(want) and g.numel() == S * NB * M * N and tuple(g.shape[-2:]) == (M, N)
        self.seen.append(("matmul_vjp", S, NB, M, K, N, want))
        da, db = ef.matmul_math(g.reshape(S, NB, M, N), a.reshape(NB, M, K), b.reshape(NB, K, N), want, None, self.matmul_mutant)
        lead = (S * a.shape[0], *a.shape[1:-2])
        return (None if da is None else da.reshape(*lead, M, K)), (None if db is None else db.reshape(*lead, K, N))

    def matmul_vjp_variant(self, S, NB, M, K, N, want=(True, True)):
        """the host-only launch plan of the library itself (no device call)"""
        from laplace_amd._lib import HipKernels

        return HipKernels().matmul_vjp_variant(S, NB, M, K, N, want)


class EmulatedEagerAttnKernels(EmulatedMatmulKernels, EmulatedSoftmaxKernels):
    pass
