"""``EmulatedNormVjpKernels`` plus max / average pooling on NHWC maps (csrc/lk_pool.hip) in stock torch, for the CPU test tier.

TEST INFRASTRUCTURE.  The stock emulation (tests/emulated_kernels.py) deliberately has no pooling methods: a ``SplitSweep`` on it
keeps a pooled model on the NCHW sweep, which existing tests rely on.  The methods here never call ``torch.max_pool2d``: the
window is walked tap by tap in row-major order with a strict ``>`` (the tie rule of the device kernel), so that the CPU tests
compare two statements of the rule.  ``last_wins = True`` is the MUTANT that breaks ties towards the last maximum.
"""
import torch

from tests.emulated_normvjp_kernels import EmulatedNormVjpKernels


def _geometry(x_hw, kernel, stride, padding):
    (H, W), (kh, kw), (ph, pw) = x_hw, kernel, padding
    sh, sw = stride if stride not in (None, (), []) else kernel
    return kh, kw, sh, sw, ph, pw, (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def _taps(t, fill, kh, kw, sh, sw, ph, pw, OH, OW):
    """``[.., H, W, C]`` -> for each tap ``(dy, dx)`` in row-major order the ``[.., OH, OW, C]`` slice of the padded tensor"""
    H, W = t.shape[-3], t.shape[-2]
    tp = t.new_full((*t.shape[:-3], H + 2 * ph, W + 2 * pw, t.shape[-1]), fill)
    tp[..., ph:ph + H, pw:pw + W, :] = t
    for dy in range(kh):
        for dx in range(kw):
            yield dy * kw + dx, tp[..., dy:dy + (OH - 1) * sh + 1:sh, dx:dx + (OW - 1) * sw + 1:sw, :]


def _divisors(x_hw, kh, kw, sh, sw, ph, pw, OH, OW, count_include_pad, divisor_override, dtype):
    """``[OH, OW, 1]`` divisor of every window (``ceil_mode`` false)"""
    if divisor_override:
        return torch.full((OH, OW, 1), float(divisor_override), dtype=dtype)
    if count_include_pad:
        return torch.full((OH, OW, 1), float(kh * kw), dtype=dtype)
    ones = torch.ones(*x_hw, 1, dtype=dtype)
    return sum(v for _, v in _taps(ones, 0.0, kh, kw, sh, sw, ph, pw, OH, OW))


class EmulatedPoolKernels(EmulatedNormVjpKernels):
    POOL_MAX, POOL_AVG = 0, 1
    last_wins = False

    def pool_forward(self, x_nhwc, kind, kernel, stride, padding, count_include_pad=True, divisor_override=None):
        B, H, W, C = x_nhwc.shape
        kh, kw, sh, sw, ph, pw, OH, OW = _geometry((H, W), _pair(kernel), stride and _pair(stride), _pair(padding))
        geo = (kh, kw, sh, sw, ph, pw, OH, OW)
        if kind == self.POOL_AVG:
            total = sum(v for _, v in _taps(x_nhwc, 0.0, *geo))
            return total / _divisors((H, W), *geo, count_include_pad, divisor_override, x_nhwc.dtype), None
        inside = list(_taps(torch.ones(H, W, 1, dtype=torch.bool), False, *geo))
        best = x_nhwc.new_full((B, OH, OW, C), float("-inf"))
        code = torch.full((B, OH, OW, C), -1, dtype=torch.int64)
        for (t, v), (_, ok) in zip(_taps(x_nhwc, float("-inf"), *geo), inside):
            better = (v >= best) if self.last_wins else (v > best)
            take = ok & (better | (code < 0) | v.isnan())  # (the first in-image tap always enters; a NaN wins, as in torch)
            best, code = torch.where(take, v, best), torch.where(take, torch.full_like(code, t), code)
        return best, code.to(torch.uint8)

    def pool_vjp(self, g, arg, S, in_hw, kind, kernel, stride, padding, count_include_pad=True, divisor_override=None,
                 amax=None):
        H, W = int(in_hw[0]), int(in_hw[1])
        kh, kw, sh, sw, ph, pw, OH, OW = _geometry((H, W), _pair(kernel), stride and _pair(stride), _pair(padding))
        geo = (kh, kw, sh, sw, ph, pw, OH, OW)
        SB, C = g.shape[0], g.shape[3]
        assert tuple(g.shape[1:3]) == (OH, OW) and SB % S == 0
        g5 = g.reshape(S, SB // S, OH, OW, C)
        if kind == self.POOL_AVG:
            assert arg is None
            g5 = g5 / _divisors((H, W), *geo, count_include_pad, divisor_override, g.dtype)
        dxp = g.new_zeros(S, SB // S, H + 2 * ph, W + 2 * pw, C)
        for t, into in _taps_view(dxp, *geo):
            into += g5 if kind == self.POOL_AVG else g5 * (arg.to(torch.int64) == t).to(g.dtype)
        dx = dxp[:, :, ph:ph + H, pw:pw + W, :].reshape(SB, H, W, C).contiguous()
        if amax is not None and dx.numel():
            amax.copy_(torch.maximum(amax.reshape(1), dx.abs().max().reshape(1).float()))
        return dx

    def pool_variant(self, kind, S, B, H, W, C, kernel, stride, padding, aligned=True):
        """the host-only launch plan of the library itself (no device call)"""
        from laplace_amd._lib import HipKernels

        return HipKernels().pool_variant(kind, S, B, H, W, C, kernel, stride, padding, aligned)


def _taps_view(tp, kh, kw, sh, sw, ph, pw, OH, OW):
    """the writable tap slices of an already padded ``[.., H + 2 ph, W + 2 pw, C]`` tensor"""
    for dy in range(kh):
        for dx in range(kw):
            yield dy * kw + dx, tp[..., dy:dy + (OH - 1) * sh + 1:sh, dx:dx + (OW - 1) * sw + 1:sw, :]
