"""``EmulatedGConvKernels`` plus the maximum over positions (csrc/lk_reduce.hip) in stock torch, for the CPU test tier.

TEST INFRASTRUCTURE.  The emulations below this one deliberately have no reduction methods: a ``SeedBatchedSweep`` on them runs the
rule on its torch math.  ``maxred_forward`` / ``maxred_vjp`` state the kernels' rules through tests/conv1d_fixtures
(``forward_reference``, ``vjp_reference``): the first maximum for ``idx``, an even split over the maxima when ``x``, ``y`` and
``cnt`` are given, every element written.  ``mutant`` selects one of the reference's MUTANTS for tests/test_conv1d_fixtures.py.
``seen`` records the calls.
"""
import torch

from tests import conv1d_fixtures as cf
from tests.emulated_gconv_kernels import EmulatedGConvKernels


class EmulatedReduceKernels(EmulatedGConvKernels):
    mutant = None

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if not hasattr(self, "seen"):
            self.seen = []

    def maxred_forward(self, x, outer, L, inner):
        assert x.dtype == torch.float32 and x.is_contiguous() and x.numel() == outer * L * inner and L >= 1 and inner >= 1
        self.seen.append(("maxred_forward", int(outer), int(L), int(inner)))
        return cf.forward_reference(x.reshape(outer, L, inner), "last" if self.mutant == "last" else None)

    def maxred_vjp(self, g, S, outer, L, inner, idx=None, x=None, y=None, cnt=None):
        even = x is not None
        assert g.dtype == torch.float32 and g.is_contiguous() and g.numel() == S * outer * inner
        if even:
            assert x.is_contiguous() and x.numel() == outer * L * inner and y.numel() == cnt.numel() == outer * inner
            assert cnt.dtype == torch.int32
            xr = x.reshape(outer, L, inner)
        else:
            assert idx.dtype == torch.int32 and idx.numel() == outer * inner
            # (an operand with the recorded first maxima: the reference rebuilds idx from it)
            pos = torch.arange(L, dtype=torch.int32).reshape(1, L, 1)
            xr = (pos == idx.reshape(outer, 1, inner)).float()
        self.seen.append(("maxred_vjp", "even" if even else "first", int(S), int(outer), int(L), int(inner)))
        into = torch.full((S, outer, L, inner), 7.0) if self.mutant == "no-fill" else None
        return cf.vjp_reference(g.reshape(S, outer, inner), xr, even, self.mutant, into).float()

    def reduce_variant(self, vjp, S, outer, L, inner, even=False, aligned=True):
        """the host-only launch plan of the library itself (no device call)"""
        from laplace_amd._lib import HipKernels

        return HipKernels().reduce_variant(vjp, S, outer, L, inner, even, aligned)
