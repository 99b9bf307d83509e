"""``EmulatedNormKernels`` plus the grouped-convolution entry point (csrc/lk_gconv.hip) in stock torch, for the CPU test tier.

TEST INFRASTRUCTURE.  The emulations below this one deliberately have no ``jac_gconv``: a backend on them sends a model with
a tracked grouped convolution to the reference's generic route.
"""
import torch
import torch.nn.functional as F

from tests.emulated_norm_kernels import EmulatedNormKernels


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


class EmulatedGConvKernels(EmulatedNormKernels):
    def jac_gconv(self, x, g, kernel_size, stride, padding, dilation, groups, Js, col0, bcol0=-1):
        """unfold per group: ``Js[n, s, col0 + o * Dkg + k] = sum_l g[s, n, o, l] * patch_group(o)[n, k, l]``"""
        B, Cin = x.shape[:2]
        S, _, Do = g.shape[:3]
        Cig, Dog = Cin // groups, Do // groups
        gl = g.reshape(S, B, Do, -1)
        Dkg = Cig * _pair(kernel_size)[0] * _pair(kernel_size)[1]
        for q in range(groups):
            cols = F.unfold(x[:, q * Cig:(q + 1) * Cig], kernel_size, dilation=dilation, padding=padding, stride=stride)
            J = torch.einsum("sbol,bkl->bsok", gl[:, :, q * Dog:(q + 1) * Dog], cols)
            Js[:, :, col0 + q * Dog * Dkg:col0 + (q + 1) * Dog * Dkg] = J.reshape(B, S, Dog * Dkg)
        if bcol0 >= 0:
            Js[:, :, bcol0:bcol0 + Do] = gl.sum(-1).permute(1, 0, 2)
