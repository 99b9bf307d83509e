"""``EmulatedCatKernels`` plus static slicing (csrc/lk_slice.hip) in stock torch, for the CPU test tier.

TEST INFRASTRUCTURE.  The stock emulation (tests/emulated_kernels.py) and the concatenation one deliberately have no slicing
methods: a ``SplitSweep`` on them keeps a model that slices a feature map on the NCHW sweep, and a ``SeedBatchedSweep`` assembles
the cotangent of a sliced tensor with the torch sequence.  ``slice_vjp`` states the kernel's rule through
tests/slice_fixtures.vjp_reference: per column the value of the first listed piece that covers it plus the later covering pieces
in the listed order, ``+0.0`` where none covers.  ``mutant`` selects one of that reference's MUTANTS for
tests/test_slice_fixtures.py.  ``seen`` records the calls (beside the concatenation's).
"""
import torch

from laplace_amd._lib import SplitTensor
from tests import slice_fixtures as sf
from tests.emulated_cat_kernels import EmulatedCatKernels


class EmulatedSliceKernels(EmulatedCatKernels):
    SLICE_MAX_PIECES = 8
    mutant = None

    def slice_forward(self, x, R, Ct, c0, Cs):
        assert x.dtype == torch.float32 and x.is_contiguous() and x.numel() == R * Ct
        assert Cs >= 1 and c0 >= 0 and c0 + Cs <= Ct
        self.seen.append(("slice_forward", int(R), int(Ct), int(c0), int(Cs)))
        return sf.forward_reference(x.reshape(R, Ct), c0, Cs)

    def slice_vjp(self, pieces, R, Ct, amax=None):
        pieces = list(pieces)
        assert 1 <= len(pieces) <= self.SLICE_MAX_PIECES, len(pieces)
        for p, c0, cs in pieces:
            assert cs >= 1 and c0 >= 0 and c0 + cs <= Ct
            if isinstance(p, SplitTensor):
                assert p.sexp.numel() == 1 and not p.chunked and p.planes.is_contiguous() and p.planes[0].numel() == R * cs
            else:
                assert p.dtype == torch.float32 and p.is_contiguous() and p.numel() == R * cs
        self.seen.append(("slice_vjp", tuple(("split" if isinstance(p, SplitTensor) else "f32", int(c0), int(cs)) for p, c0, cs in pieces),
                          int(R), int(Ct), amax is not None))
        dx = sf.vjp_reference(pieces, R, Ct, self.mutant)
        if amax is not None and dx.numel():
            amax.copy_(torch.maximum(amax.reshape(1), dx.abs().max().reshape(1).float()))
        return dx

    def slice_variant(self, split_mask, c0, cs, R, Ct, aligned=True):
        """the host-only launch plan of the library itself (no device call)"""
        from laplace_amd._lib import HipKernels

        return HipKernels().slice_variant(split_mask, c0, cs, R, Ct, aligned)
