"""``EmulatedKernels`` plus the softmax VJP kernel (csrc/lk_softmax.hip) in stock torch, for the CPU test tier.

TEST INFRASTRUCTURE.  The stock emulation (tests/emulated_kernels.py) deliberately has no ``softmax_vjp``: a ``SeedBatchedSweep`` on
it takes the torch math of the softmax rule.  ``softmax_vjp`` states the kernel's rule through tests/eager_attn_fixtures.softmax_math
- ``y * (g - sum g y)``, or ``g - exp(y) sum g`` for a log-softmax, along the last dim - with the binding's own checks on what
belongs together; ``softmax_mutant`` selects one of that function's SOFTMAX_MUTANTS.  ``seen`` records the calls.
"""
import torch

from tests import eager_attn_fixtures as ef
from tests.emulated_kernels import EmulatedKernels


class EmulatedSoftmaxKernels(EmulatedKernels):
    softmax_mutant = None

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.seen = []

    def softmax_vjp(self, g, y, S, is_log=False):
        for t in (g, y):
            assert t.dtype == torch.float32 and t.is_contiguous()
        S, is_log = int(S), bool(is_log)
        L = int(y.shape[-1])
        R = y.numel() // L
        assert S >= 1 and L >= 1 and g.numel() == S * y.numel()
        self.seen.append(("softmax_vjp", "log" if is_log else "softmax", S, R, L))
        return ef.softmax_math(g.reshape(S, R, L), y.reshape(R, L), is_log, mutant=self.softmax_mutant).reshape(g.shape)

    def softmax_vjp_variant(self, S, R, L, is_log=False, aligned=True):
        """the host-only launch plan of the library itself (no device call)"""
        from laplace_amd._lib import HipKernels

        return HipKernels().softmax_vjp_variant(S, R, L, is_log, aligned)
