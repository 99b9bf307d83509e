"""``EmulatedNormKernels`` plus the forward and input VJP of nn.RMSNorm (csrc/lk_rmsnorm.hip) in stock torch, for the CPU test tier.

TEST INFRASTRUCTURE.  The stock emulation (tests/emulated_kernels.py) deliberately has neither method: a ``SeedBatchedSweep`` on it
takes the torch math of the rule (laplace_amd/sweep.py, ``rmsnorm_forward_math``).  The two methods here are written independently
of that code - through ``Tensor.norm`` and an ``einsum`` over a flat ``[S, rows, D]`` view - so that the CPU tests compare two
statements of the rule, with the binding's own checks on what belongs together.  ``seen`` records the calls.
"""
import torch

from tests.emulated_norm_kernels import EmulatedNormKernels


class EmulatedRmsNormKernels(EmulatedNormKernels):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.seen = []

    def rmsnorm_forward(self, x2d, w, eps):
        assert x2d.dtype == torch.float32 and x2d.is_contiguous() and x2d.dim() == 2 and x2d.shape[1] >= 1
        assert w is None or (w.dtype == torch.float32 and w.is_contiguous() and w.numel() == x2d.shape[1])
        rows, D = x2d.shape
        self.seen.append(("rmsnorm_forward", int(rows), int(D), w is not None, float(eps)))
        rstd = torch.rsqrt(x2d.norm(dim=1) ** 2 / D + eps)
        y = torch.einsum("rd,r->rd", x2d, rstd)  # (a buffer of its own: an in-place op behind the layer writes into ``y``)
        return (y if w is None else y * w.reshape(1, D)), rstd

    def rmsnorm_vjp(self, g, x2d, rstd, w, S, amax=None):
        for t in (g, x2d, rstd):
            assert t.dtype == torch.float32 and t.is_contiguous()
        rows, D = x2d.shape
        S = int(S)
        assert S >= 1 and g.numel() == S * rows * D and rstd.numel() == rows and (w is None or w.numel() == D)
        self.seen.append(("rmsnorm_vjp", S, int(rows), int(D), w is not None))
        t = g.reshape(S, rows, D) if w is None else g.reshape(S, rows, D) * w.reshape(1, 1, D)
        xh = x2d * rstd.reshape(rows, 1)
        m2 = torch.einsum("srd,rd->sr", t, xh) / D
        dx = ((t - xh.unsqueeze(0) * m2.unsqueeze(-1)) * rstd.reshape(1, rows, 1)).reshape(g.shape)
        if amax is not None and dx.numel():
            amax.copy_(torch.maximum(amax.reshape(1), dx.abs().max().reshape(1).float()))
        return dx

    def rmsnorm_variant(self, S, rows, D, aligned=True):
        """the host-only launch plan of the library itself (no device call)"""
        from laplace_amd._lib import HipKernels

        return HipKernels().rmsnorm_variant(S, rows, D, aligned)
