"""``EmulatedPoolKernels`` plus the norm-tap Jacobian of the NHWC split-fp16 sweep (csrc/lk_normtap.hip) in stock torch, for the CPU
test tier.

TEST INFRASTRUCTURE.  The emulations below this one deliberately have no ``jac_norm_affine_nhwc``: a ``SplitSweep`` on them refuses
a tapped BatchNorm by name even with ``nhwc_norm_taps`` set, which the tests of that refusal rely on.  The method here follows the
device kernel by index and in its order of operations, all in fp32: a lane row ``ty`` of the launch's ``R`` adds its positions
``ty, ty + R, ..`` one after the other, the rows of a wave meet in the halving tree the xor-shuffles form, the four waves as
``(w0 + w2) + (w1 + w3)``, and the power-of-two scale is applied once, at the store.  (Not bit for bit: the device fuses the
multiply into the add.)  ``R`` comes from ``lk_normtap_variant``, the library's own host code.
Three MUTANTS: ``scaled_cotangent`` reads a cotangent that already carries the BatchNorm scale (the factor the kernel can see,
``rstd``), ``drop_low`` ignores the low plane, ``no_mean`` forms ``xhat`` without subtracting the mean.
"""
import torch

from tests.emulated_pool_kernels import EmulatedPoolKernels


class EmulatedNormtapKernels(EmulatedPoolKernels):
    scaled_cotangent = False
    drop_low = False
    no_mean = False

    def normtap_variant(self, S, B, L, Ch, affine=True, aligned=True):
        """the host-only launch plan of the library itself (no device call)"""
        from laplace_amd._lib import HipKernels

        return HipKernels().normtap_variant(S, B, L, Ch, affine, aligned)

    def jac_norm_affine_nhwc(self, g, x, mu, rstd, S, Js, wcol0, bcol0=-1, aligned=True):
        from laplace_amd._lib import LaplaceHipError, _one_scale

        _one_scale(g, "jac_norm_affine_nhwc")
        if g.chunked:
            raise LaplaceHipError("jac_norm_affine_nhwc: a chunk-major split tensor")
        if not (g.planes.is_contiguous() and x.is_contiguous() and Js.is_contiguous()):
            raise LaplaceHipError("jac_norm_affine_nhwc: tensor must be contiguous")
        B, Ch = x.shape[0], x.shape[-1]
        L = max(x.numel() // max(B * Ch, 1), 1)
        assert g.planes.shape[1] == S * B and (mu is None) == (rstd is None) and tuple(Js.shape[:2]) == (B, S)
        if B == 0 or (wcol0 < 0 and bcol0 < 0):
            return
        R = self.normtap_variant(S, B, L, Ch, mu is not None, aligned)["lane_rows"]
        h, low = g.planes[0].float().reshape(S, B, L, Ch), g.planes[1].float().reshape(S, B, L, Ch)
        gv = h if self.drop_low else h + low
        xh = x.float().reshape(B, L, Ch)
        if mu is not None:
            xh = (xh if self.no_mean else xh - mu.float()) * rstd.float()
            if self.scaled_cotangent:
                gv = gv * rstd.float()
        rows_w = torch.zeros(R, S, B, Ch)
        rows_b = torch.zeros(R, S, B, Ch)
        for l in range(L):  # (lane row l % R adds position l to what it holds)
            rows_w[l % R] += gv[:, :, l] * xh[:, l]
            rows_b[l % R] += gv[:, :, l]
        scale = torch.exp2(-g.sexp.float()).reshape(())
        for rows, col0 in ((rows_w, wcol0), (rows_b, bcol0)):
            if col0 < 0:
                continue
            per_wave = rows.reshape(4, R // 4, S, B, Ch) if R >= 4 else None
            assert per_wave is not None  # (a workgroup has at least four lane rows: 64 channel lanes at the most)
            while per_wave.shape[1] > 1:  # lane row r meets r ^ half: the first half holds the sums
                half = per_wave.shape[1] // 2
                per_wave = per_wave[:, :half] + per_wave[:, half:]
            w = per_wave[:, 0]
            total = (w[0] + w[2]) + (w[1] + w[3])
            Js[:, :, col0:col0 + Ch] = (total * scale).permute(1, 0, 2)
