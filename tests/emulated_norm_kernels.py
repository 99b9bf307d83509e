"""``EmulatedKernels`` plus the norm-parameter entry point (csrc/lk_norm.hip) in stock torch, for the CPU test tier.

TEST INFRASTRUCTURE.  The stock emulation (tests/emulated_kernels.py) deliberately has no ``jac_norm_affine``: a backend on
it keeps the reference's generic route for normalisation parameters, which two existing tests pin.
"""
import torch

from tests.emulated_kernels import EmulatedKernels


class EmulatedNormKernels(EmulatedKernels):
    def jac_norm_affine(self, g, xhat, Ch, layout, Js, wcol0, bcol0=-1):
        S, B = g.shape[:2]
        if layout == 0:
            g4, x3 = g.reshape(S, B, Ch, -1), xhat.reshape(B, Ch, -1)
            Jw, Jb = torch.einsum("sbcl,bcl->bsc", g4, x3), g4.sum(-1).permute(1, 0, 2)
        else:
            g4, x3 = g.reshape(S, B, -1, Ch), xhat.reshape(B, -1, Ch)
            Jw, Jb = torch.einsum("sblc,blc->bsc", g4, x3), g4.sum(2).permute(1, 0, 2)
        if wcol0 >= 0:
            Js[:, :, wcol0:wcol0 + Ch] = Jw
        if bcol0 >= 0:
            Js[:, :, bcol0:bcol0 + Ch] = Jb
