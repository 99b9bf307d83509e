"""``EmulatedReduceKernels`` plus the static separable resampling VJP (csrc/lk_resample.hip) in stock torch, for the CPU test tier.

TEST INFRASTRUCTURE.  The emulations below this one deliberately have no resampling methods: a ``SeedBatchedSweep`` on them runs the
rule on its torch math.  ``resample_pack`` validates the transposed tap lists as the library's wrapper does (it IS the wrapper's
code, run on CPU tensors); ``resample_vjp`` states the kernel's contract through tests/resample_fixtures (``vjp_reference``): the sum
over the taps with the fp32 tables, EVERY element written into a NaN-filled output, ``+0.0`` for an input that no output reads.
``mutant`` selects one of the reference's MUTANTS for tests/test_resample_fixtures.py.  ``seen`` records the calls.
"""
import torch

from laplace_amd._lib import HipKernels
from tests import resample_fixtures as rf
from tests.emulated_reduce_kernels import EmulatedReduceKernels


class _OnCpu(HipKernels):
    """the library's wrapper with its tensor check relaxed to CPU tensors (the validation itself is what is reused)"""

    def __init__(self):
        pass


class EmulatedResampleKernels(EmulatedReduceKernels):
    mutant = None
    RESAMPLE_MAX_TAPS = rf.CAP

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if not hasattr(self, "seen"):
            self.seen = []

    def resample_pack(self, ptr, idx, w, L, OL):
        from laplace_amd import _lib

        assert ptr.dtype == idx.dtype == torch.int32 and w.dtype == torch.float32
        check, _lib._check = _lib._check, lambda t, name, dtype=torch.float32: t
        try:
            return HipKernels.resample_pack(_OnCpu(), ptr.contiguous(), idx.contiguous(), w.contiguous(), L, OL)
        finally:
            _lib._check = check

    def resample_vjp(self, g, axis_h, axis_w):
        (_, _, _, H, OH, th), (_, _, _, W, OW, tw) = axis_h, axis_w
        assert g.dtype == torch.float32 and g.is_contiguous() and g.dim() == 3 and tuple(g.shape[1:]) == (OH, OW) and g.shape[0] >= 1
        assert max(th, tw) <= self.RESAMPLE_MAX_TAPS
        self.seen.append(("resample_vjp", int(g.shape[0]), OH, OW, H, W, th, tw))
        into = torch.full((g.shape[0], H, W), float("nan"))
        dx, _, untapped = rf.vjp_reference(g, axis_h, axis_w, self.mutant, into if self.mutant == "no-zero" else None)
        into.copy_(dx)  # (every element written)
        if self.mutant != "no-zero":
            into[untapped.expand_as(into)] = 0.0  # (+0.0, whatever the sign of the sum of nothing)
        return into

    def resample_variant(self, P, OH, OW, H, W, taps_h, taps_w, aligned=True):
        """the host-only launch plan of the library itself (no device call)"""
        return HipKernels().resample_variant(P, OH, OW, H, W, taps_h, taps_w, aligned)
