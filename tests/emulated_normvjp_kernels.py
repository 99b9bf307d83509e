"""``EmulatedNormKernels`` plus the forward and input VJP of GroupNorm / LayerNorm (csrc/lk_normvjp.hip) in stock torch, for
the CPU test tier.

TEST INFRASTRUCTURE.  The stock emulation (tests/emulated_kernels.py) and ``EmulatedNormKernels`` deliberately have neither
method: a sweep on them applies the same formula in plain torch (laplace_amd/sweep.py, ``norm_forward_math``).  The two
methods here are written independently of that code - on a channels-first copy, through ``Tensor.var`` and a flat
``[S, B, G, N]`` view - so that the CPU tests compare two statements of the rule.
"""
import torch

from tests.emulated_norm_kernels import EmulatedNormKernels


def _channels_first(t, layout):
    """``[.., Ch, L]`` copy of a ``[.., L.., Ch]`` tensor (layout 1) / flat view of ``[.., Ch, L..]`` (layout 0), and the way back"""
    if layout == 0:
        return t.reshape(*t.shape[:2], -1), lambda u: u.reshape(t.shape)
    moved = t.movedim(-1, 1)
    return moved.reshape(*moved.shape[:2], -1), lambda u: u.reshape(moved.shape).movedim(1, -1).contiguous()


class EmulatedNormVjpKernels(EmulatedNormKernels):
    def norm_forward(self, x, w, b, G, layout, eps):
        x3, back = _channels_first(x, layout)
        B, Ch, L = x3.shape
        rows = x3.reshape(B, G, -1)
        rstd = 1.0 / torch.sqrt(rows.var(-1, unbiased=False) + eps)
        # (``F.group_norm`` itself refuses a single value per channel, which the kernel serves)
        xhat = ((rows - rows.mean(-1, keepdim=True)) * rstd.unsqueeze(-1)).reshape(x3.shape)
        # (as the device kernel, ``y`` and ``xhat`` are separate buffers: an in-place op behind the layer writes into ``y``)
        y = xhat.clone() if w is None else xhat * w.reshape(1, Ch, 1)
        if b is not None:
            y = y + b.reshape(1, Ch, 1)
        return back(y), back(xhat), rstd

    def norm_vjp(self, g, xhat, rstd, w, S, G, layout, amax=None):
        B = xhat.shape[0]
        x3, _ = _channels_first(xhat, layout)
        g3, back = _channels_first(g, layout)  # [S*B, Ch, L]
        Ch = x3.shape[1]
        t = g3 if w is None else g3 * w.reshape(1, Ch, 1)
        t = t.reshape(S, B, G, -1)
        xr = x3.reshape(1, B, G, -1)
        N = xr.shape[-1]
        m1 = t.sum(-1, keepdim=True) / N
        m2 = (t * xr).sum(-1, keepdim=True) / N
        dx = back((rstd.reshape(1, B, G, 1) * (t - m1 - xr * m2)).reshape(g3.shape))
        if amax is not None:
            amax.copy_(torch.maximum(amax.reshape(1), dx.abs().max().reshape(1).float()) if dx.numel() else amax)
        return dx

    def norm_sweep_variant(self, S, B, L, Ch, G, layout, aligned=True):
        """the host-only launch plan of the library itself (no device call)"""
        from laplace_amd._lib import HipKernels

        return HipKernels().norm_sweep_variant(S, B, L, Ch, G, layout, aligned)
