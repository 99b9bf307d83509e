"""``EmulatedPoolKernels`` plus the depthwise convolution on NHWC maps (csrc/lk_dwconv.hip) and the grouped-convolution Jacobian in
stock torch, for the CPU test tier.

TEST INFRASTRUCTURE.  The emulations below this one deliberately have no depthwise methods: a ``SplitSweep`` on them keeps a
model with a depthwise layer on the NCHW sweep, which existing tests rely on.  The methods here never call ``conv2d``: the forward
walks the window tap by tap in row-major order, and the backward is the GATHER form of the device kernel - for every tap the
input pixels it reaches, by index - so that the CPU tests compare it with the scatter definition of tests/dwconv_fixtures.py.
Two MUTANTS: ``correlate = True`` does not mirror the taps (the weight of tap ``(kh - 1 - dy, kw - 1 - dx)`` where ``(dy, dx)``
belongs), ``floor_div = True`` drops the divisibility test (``(h + ph - dy) / sh`` rounded down).
"""
import torch

from tests.emulated_gconv_kernels import EmulatedGConvKernels
from tests.emulated_pool_kernels import EmulatedPoolKernels, _pair, _taps


class EmulatedDwconvKernels(EmulatedPoolKernels, EmulatedGConvKernels):
    correlate = False
    floor_div = False

    def dwconv_forward(self, x_nhwc, w_tap, bias, kernel, stride, padding):
        B, H, W, C = x_nhwc.shape
        (kh, kw), (sh, sw), (ph, pw) = _pair(kernel), _pair(stride), _pair(padding)
        OH, OW = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
        assert tuple(w_tap.shape) == (kh * kw, C)
        y = x_nhwc.new_zeros(B, OH, OW, C) if bias is None else bias.to(x_nhwc.dtype).expand(B, OH, OW, C).clone()
        for t, v in _taps(x_nhwc, 0.0, kh, kw, sh, sw, ph, pw, OH, OW):
            y += w_tap[t] * v
        return y

    def dwconv_backward(self, g, w_tap, S, in_hw, kernel, stride, padding, amax=None):
        from laplace_amd._lib import _one_scale

        _one_scale(g, "dwconv_backward")
        H, W = int(in_hw[0]), int(in_hw[1])
        (kh, kw), (sh, sw), (ph, pw) = _pair(kernel), _pair(stride), _pair(padding)
        OH, OW = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
        SB, C = g.planes.shape[1], g.planes.shape[4]
        assert tuple(g.planes.shape[2:4]) == (OH, OW) and SB % S == 0 and tuple(w_tap.shape) == (kh * kw, C)
        gv = g.planes[0].float() + g.planes[1].float()  # (the scale is applied once, to the sum over the taps)
        dx = torch.zeros(SB, H, W, C, dtype=torch.float32)

        def reached(n_in, n_out, p, d, s):
            """input indices a tap offset ``d`` reaches, and the output index each one reads"""
            num = torch.arange(n_in) + p - d
            o = torch.div(num, s, rounding_mode="floor")
            ok = (num >= 0) & (o < n_out)
            if not self.floor_div:
                ok &= num % s == 0
            return torch.nonzero(ok).flatten(), o[ok]

        for dy in range(kh):
            hi, oh = reached(H, OH, ph, dy, sh)
            for dx_ in range(kw):
                wi, ow = reached(W, OW, pw, dx_, sw)
                if not (hi.numel() and wi.numel()):
                    continue
                t = (kh - 1 - dy) * kw + (kw - 1 - dx_) if self.correlate else dy * kw + dx_
                dx[:, hi[:, None], wi[None, :], :] += w_tap[t].float() * gv[:, oh[:, None], ow[None, :], :]
        dx *= torch.exp2(-g.sexp.float()).reshape(())
        if amax is not None and dx.numel():
            amax.copy_(torch.maximum(amax.reshape(1), dx.abs().max().reshape(1).float()))
        return dx

    def dwconv_variant(self, S, B, H, W, C, kernel, stride, padding, aligned=True):
        """the host-only launch plan of the library itself (no device call)"""
        from laplace_amd._lib import HipKernels

        return HipKernels().dwconv_variant(S, B, H, W, C, kernel, stride, padding, aligned)
