"""CPU stand-in for ``laplace_amd._lib.HipKernels`` — TEST INFRASTRUCTURE ONLY.

Each method restates, with plain torch CPU ops, what the C-ABI entry point of the same name is
specified to compute (include/laplace_hip.h).  It lets the `not gpu` tests drive the *host logic*
(hooks, factor ordering/scaling, Kron subclasses inside the reference's own fit loop, sharding)
on a machine without a GPU.  The product never installs it (laplace_amd._lib.get_kernels loads
the HIP library or raises).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


class EmulatedKernels:
    name = "emulated-cpu"

    # likelihood
    def softmax_hess_sqrt(self, f, y=None, loss_accum=None, cholesky=False):
        p = torch.softmax(f, dim=-1)
        if cholesky and f.shape[1] >= 2:
            B, C = p.shape
            sfx = torch.flip(torch.cumsum(torch.flip(p, [1]), 1), [1])  # s_j = sum_{k>=j} p_k
            sfx = torch.cat([sfx, torch.zeros(B, 1, dtype=p.dtype)], 1)
            S = torch.zeros(C - 1, B, C, dtype=p.dtype)
            for c in range(C - 1):
                sc, sn = sfx[:, c], sfx[:, c + 1]
                ok = (sn > 0) & (sc > 0)
                r0 = torch.where(ok, torch.sqrt(p[:, c] / sc.clamp_min(1e-300)), torch.zeros_like(sc))
                rs = torch.where(ok, 1.0 / torch.sqrt(sn.clamp_min(1e-300)), torch.zeros_like(sc))
                S[c, :, c] = r0 * torch.sqrt(sn)
                S[c, :, c + 1:] = -(p[:, c + 1:] * rs[:, None]) * r0[:, None]
            if y is not None and loss_accum is not None:
                loss_accum += self._ce_sum(f, y)
            return S
        sp = p.sqrt()
        S = torch.diag_embed(sp) - p.unsqueeze(2) * sp.unsqueeze(1)  # [B, j, c]
        if y is not None and loss_accum is not None:
            loss_accum += self._ce_sum(f, y)
        return S.permute(2, 0, 1).contiguous()  # [c, B, j]

    @staticmethod
    def _ce_sum(f, y):
        """labels outside [0, C) (e.g. an ignore_index of -100) contribute nothing; a batch without a valid label adds
        nothing at all"""
        ok = (y >= 0) & (y < f.shape[1])
        if not bool(ok.any()):
            return 0
        return -torch.log_softmax(f[ok], -1).gather(1, y[ok].view(-1, 1)).sum()

    def sq_err_sum(self, f, y, scale, loss_accum):
        loss_accum += scale * ((f - y) ** 2).sum()

    # split-fp16 convolution family (csrc/lk_conv.hip, lk_sweep16.hip): same splits, fp32 products
    conv_config = 0

    @staticmethod
    def _sexp_for(amax):
        import math

        a = float(amax)
        if not (a > 0) or a < 2.0 ** -126:
            return 120
        return min(120, 14 - math.floor(math.log2(a)))

    @staticmethod
    def _split(x, s):
        from laplace_amd._lib import SplitTensor

        xs = x.float() * (2.0 ** s)
        h = xs.half()
        l = (xs - h.float()).half()
        return SplitTensor(torch.stack([h, l]), torch.tensor([s], dtype=torch.int32))

    def absmax(self, x, out=None):
        v = x.abs().max().reshape(1).float() if x.numel() else torch.zeros(1)
        if out is not None:
            out.copy_(v)
            return out
        return v

    use_copy_absmax = True

    def copy_absmax(self, x, out, amax):
        out.copy_(x)
        amax.copy_(torch.maximum(amax, x.abs().max().reshape(1).float()))
        return out

    def split_images_f16x2(self, x):
        """lk_split_images_f16x2: one scale per image of the leading dimension, from the image's own max|x_n| (-> amax [N])"""
        from laplace_amd._lib import SplitTensor

        N = x.shape[0]
        am = x.detach().abs().reshape(N, -1).amax(1).float() if x.numel() else torch.zeros(N)
        s = torch.tensor([self._sexp_for(a) for a in am.tolist()], dtype=torch.int32)
        xs = x.float() * torch.exp2(s.float()).reshape(N, *([1] * (x.dim() - 1)))
        h = xs.half()
        l = (xs - h.float()).half()
        return SplitTensor(torch.stack([h, l]), s, am)

    def split_f16x2(self, x, amax=None, bound_mul=1.0, out=None):
        if amax is None:
            amax = self.absmax(x)
        st = self._split(x, self._sexp_for(float(amax[0]) * bound_mul))
        if out is not None:
            assert out.dtype == torch.float16 and tuple(out.shape) == (2,) + tuple(x.shape)
            from laplace_amd._lib import SplitTensor

            out.copy_(st.planes)
            st = SplitTensor(out, st.sexp)
        return st

    def conv_prep_weights(self, W, transpose, cscale=None):
        Wf = W.float()
        if cscale is not None:
            Wf = Wf * cscale.reshape(-1, 1, 1, 1)
        Co, Ci = Wf.shape[:2]
        Wt = Wf.reshape(Co, Ci, -1).permute(2, 1, 0) if transpose else Wf.reshape(Co, Ci, -1).permute(2, 0, 1)
        st = self._split(Wt.contiguous(), self._sexp_for(Wt.abs().max()))
        return st.planes, st.sexp

    def conv_nhwc_f16x2(self, x, wplanes, wsexp, Hc, Wc, in_mul, out, out_step, oh0, ow0, taps, accumulate=False,
                        amax_out=None, config=None):
        xin = x.float()                                               # [N, Hi, Wi, Ci]
        w = (wplanes[0].float() + wplanes[1].float()) * 2.0 ** (-int(wsexp[0]))  # [T, Co, Ci]
        N, Hi, Wi, Ci = xin.shape
        res = torch.zeros(N, Hc, Wc, w.shape[1])
        ii, jj = torch.arange(Hc) * in_mul, torch.arange(Wc) * in_mul
        for dh, dw, wt in taps:
            hh, ww = ii + dh, jj + dw
            vh, vw = (hh >= 0) & (hh < Hi), (ww >= 0) & (ww < Wi)
            xt = xin[:, hh.clamp(0, Hi - 1)][:, :, ww.clamp(0, Wi - 1)]
            xt = xt * (vh[:, None] & vw[None, :])[None, :, :, None]
            res += torch.einsum("nijc,oc->nijo", xt, w[wt])
        if config is not None and (config & 16):  # position-contiguous output: `out` is an NHWC-shaped view of [N, Co, Hc*Wc]
            assert not accumulate and out_step == 1 and oh0 == 0 and ow0 == 0 and out.is_contiguous()
            out.view(N, w.shape[1], Hc, Wc).copy_(res.permute(0, 3, 1, 2))
            if amax_out is not None:
                amax_out.copy_(torch.maximum(amax_out, res.abs().max().reshape(1)))
            return out
        view = out[:, oh0::out_step, ow0::out_step][:, :Hc, :Wc]
        if accumulate:
            view += res
        else:
            view.copy_(res)
        if amax_out is not None:
            amax_out.copy_(torch.maximum(amax_out, view.abs().max().reshape(1)))
        return out

    def conv_nhwc_f16x2_planes(self, x, wplanes, wsexp, w_l1, Ho, Wo, in_mul, taps, config=None):
        """lk_conv_nhwc_f16x2_planes: position-contiguous output as a SplitTensor [N, Co, Ho * Wo], scaled per entry of x.sexp
        from the bound max|x_n| * w_l1"""
        from laplace_amd._lib import SplitTensor

        N = x.shape[0]
        Co = wplanes.shape[2]
        res = torch.zeros(N, Ho, Wo, Co)
        self.conv_nhwc_f16x2(x, wplanes, wsexp, Ho, Wo, in_mul, res, 1, 0, 0, taps)
        res = res.permute(0, 3, 1, 2).reshape(N, Co, Ho * Wo)
        ns = x.sexp.numel()
        in_amax = (x.amax.float().reshape(-1) if getattr(x, "amax", None) is not None and x.amax.numel() == ns
                   else torch.exp2(15.0 - x.sexp.float()))
        bound = in_amax * float(w_l1[0])
        got = res.abs().reshape(N, -1).amax(1) if ns > 1 else res.abs().max().reshape(1)
        assert bool((got <= bound * (1 + 1e-5) + 1e-30).all()), "max|in| * l1(W) does not bound the convolution"
        s = torch.tensor([self._sexp_for(b) for b in bound.tolist()], dtype=torch.int32)
        rs = res * torch.exp2(s.float()).reshape(-1, 1, 1)
        h = rs.half()
        l = (rs - h.float()).half()
        return SplitTensor(torch.stack([h, l]), s).chunk_major()  # (the layout the HIP kernel writes)

    def conv_winp_eligible(self, N, Hi, Wi, Ci, Co, T, mask_is_float=False) -> bool:
        # (mirrors lk_conv_winp_eligible, so that the host logic around the chunk-major weights is exercised on the CPU)
        return bool(T == 9 and Wi <= 47 and Hi * Wi >= 16 and Ci % 32 == 0 and Ci >= 32 and Co >= 64 and Co % 64 == 0
                    and N * Hi * Wi * Ci < (1 << 30) and N * Hi * Wi * Co < (1 << 31) and N * Hi * Wi >= 512 and not mask_is_float)

    def conv_nhwc_f16x2_vjp(self, x, wplanes, wsexp, w_l1, Ho, Wo, taps, add=None, mult=None, mult_amax=None, scale=None,
                            scale_amax=None, config=None, amax_word=None, wplanes_chunked=None):
        if wplanes_chunked is not None:  # the same weights, chunk-major: must agree with the GEMM-natural planes
            two, T, N_, Kd = wplanes.shape
            assert torch.equal(wplanes_chunked, wplanes.view(two, T, N_, Kd // 16, 16).permute(0, 1, 3, 2, 4))
        """lk_conv_nhwc_f16x2_vjp: the convolution, then (conv + add) * mult * scale split with the scale of the
        guaranteed bound max|in| * l1(W) (+ ...); the measured max|.| rides along as ``amax``"""
        N = x.shape[0]
        Co = wplanes.shape[2]
        from laplace_amd._lib import _one_scale

        _one_scale(x, "conv_nhwc_f16x2_vjp"), _one_scale(add, "conv_nhwc_f16x2_vjp")  # (as the library's wrapper)
        conv = self.conv_nhwc_f16x2(x, wplanes, wsexp, Ho, Wo, 1, torch.zeros(N, Ho, Wo, Co), 1, 0, 0, taps)
        in_amax = float(x.amax[0]) if getattr(x, "amax", None) is not None else 2.0 ** (15 - int(x.sexp[0]))
        bound = in_amax * float(w_l1[0])
        assert float(conv.abs().max()) <= bound * (1 + 1e-5) + 1e-30, "max|in| * l1(W) does not bound the convolution"
        v = conv
        if add is not None:
            v = v + add.float()
            bound += 2.0 ** (15 - int(add.sexp[0]))
        if mult is not None:
            mf = mult.float() if mult.dtype not in (torch.uint8, torch.bool) else (mult != 0).float()
            S = N // mf.shape[0]
            v = (v.reshape(S, *mf.shape) * mf).reshape(v.shape)
            if mult.dtype == torch.float32 and mult_amax is not None:
                bound *= float(mult_amax[0])
        if scale is not None:
            v = v * scale
            bound *= float(scale_amax[0])
        assert float(v.abs().max()) <= bound * (1 + 1e-6) + 1e-30, "the guaranteed bound of the fused epilogue does not hold"
        out = self._split(v, self._sexp_for(bound))
        out.amax = out.float().abs().max().reshape(1).float()
        return out

    def conv_nhwc_f16x2_vjp_strided(self, sources, Ho, Wo, os, taps, add=None, mult=None, mult_amax=None, scale=None,
                                    scale_amax=None, amax_word=None):
        """lk_conv_nhwc_f16x2_vjp_strided: every residue class of one or two strided convolutions' backward-data, then the
        fused epilogue with the scale of the guaranteed bound sum_i max|in_i| * l1(W_i) (+ ...)"""
        from laplace_amd._lib import LaplaceHipError

        x0, w0 = sources[0][0], sources[0][1]
        if len(sources) not in (1, 2) or any(tuple(s_[0].planes.shape) != tuple(x0.planes.shape) or s_[1].shape[2:] != w0.shape[2:]
                                             for s_ in sources):  # (as the library's wrapper: _lib.conv_nhwc_f16x2_vjp_strided)
            raise LaplaceHipError("conv_nhwc_f16x2_vjp_strided: one or two sources of the same shapes")
        N = sources[0][0].shape[0]
        Co = sources[0][1].shape[2]
        assert Ho % os == 0 and Wo % os == 0 and {(t[4], t[5]) for t in taps} == {(a, b) for a in range(os) for b in range(os)}
        v = torch.zeros(N, Ho, Wo, Co)
        bound = 0.0
        for i, (x, wplanes, wsexp, w_l1) in enumerate(sources):
            assert tuple(x.shape[1:3]) == (Ho // os, Wo // os)
            __import__("laplace_amd._lib", fromlist=["_one_scale"])._one_scale(x, "conv_nhwc_f16x2_vjp_strided")
            for oh0 in range(os):
                for ow0 in range(os):
                    ts = [(t[0], t[1], t[2]) for t in taps if t[3] == i and (t[4], t[5]) == (oh0, ow0)]
                    if ts:
                        self.conv_nhwc_f16x2(x, wplanes, wsexp, Ho // os, Wo // os, 1, v, os, oh0, ow0, ts, accumulate=True)
            in_amax = float(x.amax[0]) if getattr(x, "amax", None) is not None else 2.0 ** (15 - int(x.sexp[0]))
            bound += in_amax * float(w_l1[0])
        assert float(v.abs().max()) <= bound * (1 + 1e-5) + 1e-30, "sum of max|in| * l1(W) does not bound the convolutions"
        if add is not None:
            v = v + add.float()
            bound += 2.0 ** (15 - int(add.sexp[0]))
        if mult is not None:
            mf = mult.float() if mult.dtype not in (torch.uint8, torch.bool) else (mult != 0).float()
            S = N // mf.shape[0]
            v = (v.reshape(S, *mf.shape) * mf).reshape(v.shape)
            if mult.dtype == torch.float32 and mult_amax is not None:
                bound *= float(mult_amax[0])
        if scale is not None:
            v = v * scale
            bound *= float(scale_amax[0])
        assert float(v.abs().max()) <= bound * (1 + 1e-6) + 1e-30, "the guaranteed bound of the fused epilogue does not hold"
        out = self._split(v, self._sexp_for(bound))
        out.amax = out.float().abs().max().reshape(1).float()
        return out

    def vjp_nhwc_split(self, g, g_amax, g2, mult, mult_amax, scale, scale_amax, S, out_shape):
        bound = 0.0
        v = torch.zeros(out_shape)
        if g is not None:
            v = v + g
            bound += float(g_amax[0])
        if g2 is not None:
            __import__("laplace_amd._lib", fromlist=["_one_scale"])._one_scale(g2, "vjp_nhwc_split")
            v = v + g2.float()
            bound += 2.0 ** (15 - int(g2.sexp[0]))
        if mult is not None:
            mf = mult.float() if mult.dtype != torch.uint8 else (mult != 0).float()
            v = (v.reshape(S, *mf.shape) * mf).reshape(out_shape)
            if mult.dtype == torch.float32 and mult_amax is not None:
                bound *= float(mult_amax[0])
        if scale is not None:
            v = v * scale
            bound *= float(scale_amax[0])
        assert float(v.abs().max()) <= bound * (1 + 1e-6) + 1e-30, "the guaranteed bound of the VJP output does not hold"
        return self._split(v, self._sexp_for(bound))

    is_channels_last = staticmethod(lambda x: __import__("laplace_amd._lib", fromlist=["x"]).is_channels_last(x))

    def bn_act_forward_nhwc(self, x, x_amax, scale, shift, scale_amax, shift_amax, act, addend=None, addend_bound=None,
                            want_mask=True, want_split=True, x_mul=None, x_add=None, amax_words=None):
        """lk_bn_act_fwd_nhwc_f16x2: planes with one scale per image from the guaranteed per-image bound, measured maxima"""
        from laplace_amd._lib import SplitTensor

        B = x.shape[0]
        assert x_amax.numel() in (1, B) and (addend is None or addend_bound.numel() in (1, B))
        bx = x_amax.float().reshape(-1).expand(B).clone()
        if x_mul is not None:
            bx = bx * float(x_mul[0])
        if x_add is not None:
            bx = bx + float(x_add[0])
        assert bool((x.abs().reshape(B, -1).amax(1) <= bx * (1 + 1e-5) + 1e-30).all()), "the bound of the forward's input does not hold"
        bound = bx * float(scale_amax[0]) + float(shift_amax[0])
        y = x * scale + shift
        if addend is not None:
            y = y + addend
            bound = bound + addend_bound.float().reshape(-1).expand(B)
        mask = None
        if act == 1:
            y = y.clamp_min(0)
            mask = (y > 0).to(torch.uint8) if want_mask else None
        elif act == 2:
            y, bound = torch.tanh(y), torch.ones(B)
        amax = y.abs().reshape(B, -1).amax(1).float()
        assert bool((amax <= bound * (1 + 1e-6) + 1e-30).all()), "the guaranteed bound of the forward does not hold"
        split = None
        if want_split:
            s = torch.tensor([self._sexp_for(a) for a in bound.tolist()], dtype=torch.int32)
            ys = y.float() * torch.exp2(s.float()).reshape(B, 1, 1, 1)
            h = ys.half()
            l = (ys - h.float()).half()
            if amax_words is not None:
                amax_words.copy_(torch.maximum(amax_words, amax))
                amax = amax_words
            split = SplitTensor(torch.stack([h, l]), s, amax)
        return y.contiguous(), mask, split, bound.float()

    use_conv_bn_act = True

    def conv_bn_act_nhwc(self, x, wplanes, wsexp, w_l1, Ho, Wo, in_mul, taps, scale, shift, scale_amax, shift_amax, act,
                         addend=None, addend_bound=None, want_mask=True, want_split=True, amax_words=None, config=None,
                         y_out=None):
        """lk_conv_bn_act_nhwc_f16x2: by definition the convolution followed by lk_bn_act_fwd_nhwc_f16x2 with x_mul = w_l1"""
        assert x.amax is not None and x.amax.numel() in (1, x.shape[0]) and act in (0, 1)
        out = torch.zeros(x.shape[0], Ho, Wo, wplanes.shape[2])
        self.conv_nhwc_f16x2(x, wplanes, wsexp, Ho, Wo, in_mul, out, 1, 0, 0, taps)
        res = self.bn_act_forward_nhwc(out, x.amax, scale, shift, scale_amax, shift_amax, act, addend=addend,
                                       addend_bound=addend_bound, want_mask=want_mask, want_split=want_split, x_mul=w_l1,
                                       amax_words=amax_words)
        if y_out is not None:  # (where the caller wants y: a slot of a pixel-pair stack)
            y_out.copy_(res[0])
            res = (y_out,) + tuple(res[1:])
        return res

    def unsplit_transpose(self, x, S, B):
        N, H, W, C = x.shape
        return x.float().reshape(S, B, H * W, C).permute(1, 0, 3, 2).contiguous()

    def gram_tn_f16x2(self, x, alpha, out):
        __import__("laplace_amd._lib", fromlist=["_one_scale"])._one_scale(x, "gram_tn_f16x2")
        C = x.planes.shape[-1]
        X = x.float().reshape(-1, C)
        Gm = X.T @ X
        idx = torch.arange(C) // 32
        upper = idx[:, None] <= idx[None, :]
        out += alpha * Gm * upper
        return out

    def pack_upper(self, A, packed):
        i, j = torch.triu_indices(A.shape[0], A.shape[0])
        packed.copy_(A[i, j])

    def unpack_upper(self, packed, A):
        i, j = torch.triu_indices(A.shape[0], A.shape[0])
        A[i, j] = packed

    # Gram family
    def gram_tn(self, X, alpha, out, upper_only=False):
        out += alpha * (X.T @ X)
        return out

    def gram_nt_slab_bytes(self, nb_total, n, L) -> int:
        return n * n * 8  # one "slab" holding the running sum (a float64 view of the uint8 buffer)

    def gram_nt(self, X, alpha, out, upper_only=False, persist=None):
        if isinstance(X, (list, tuple)):
            X = torch.cat(list(X))
        G = torch.einsum("bil,bjl->ij", X, X)
        if persist is not None:  # accumulate unscaled partial sums; alpha is applied by gram_slabs_reduce
            n = G.shape[0]
            persist[: n * n * 8].view(torch.float64).view(n, n).add_(G.double())
            return out
        out += alpha * G
        return out

    def gram_slabs_reduce(self, slabs, n, L, alpha, out, upper_only=False):
        out += alpha * slabs[: n * n * 8].view(torch.float64).view(n, n).to(out.dtype)
        return out

    use_gram_conv16 = True

    def im2col_split(self, x, kernel_size, stride, padding, Kp, amax=None):
        """lk_im2col_split_f16x2: patch matrix [B * Ho * Wo, Kp] in (kh, kw, ci) column order, zero padded, one scale"""
        import torch.nn.functional as F_

        B, C = x.shape[0], x.shape[1]
        KH, KW = kernel_size
        cols = F_.unfold(x.float().contiguous(), kernel_size, 1, int(padding), int(stride))  # [B, C KH KW, L] in (ci, kh, kw) order
        L = cols.shape[2]
        cols = cols.reshape(B, C, KH * KW, L).permute(0, 3, 2, 1).reshape(B * L, KH * KW * C)
        if Kp > cols.shape[1]:
            cols = torch.cat([cols, cols.new_zeros(cols.shape[0], Kp - cols.shape[1])], 1)
        return self.split_f16x2(cols.contiguous(), amax=amax if amax is not None else self.absmax(x))

    def gram_conv(self, x, kernel_size, stride, padding, dilation, alpha, out, upper_only=False, native=False):
        cols = F.unfold(x, kernel_size, dilation=dilation, padding=padding, stride=stride)  # [B, D, L]
        G = alpha * torch.einsum("bil,bjl->ij", cols, cols)
        if native:
            Cin = x.shape[1]
            KK = G.shape[0] // Cin
            idx = torch.arange(Cin * KK).reshape(Cin, KK).T.reshape(-1)  # native (d, ci) -> unfold index
            G = G[idx][:, idx]
        out += G
        return out

    def permute_native_to_unfold(self, src, Cin, KK, dst, accumulate=False):
        idx = torch.arange(Cin * KK).reshape(KK, Cin).T.reshape(-1)  # unfold (ci, d) -> native index
        v = src[idx][:, idx]
        if accumulate:
            dst += v
        else:
            dst.copy_(v)
        return dst

    def symmetrize(self, C):
        C.copy_(torch.triu(C) + torch.triu(C, 1).T)
        return C

    def finalize_factors(self, items):
        for src, dst, scale, cin, kk in items:
            if not src.numel():
                continue
            full = torch.triu(src) + torch.triu(src, 1).T
            if kk > 1:
                assert dst is not None and scale is None
                self.permute_native_to_unfold(full, cin, kk, dst)
            else:
                if scale is not None:
                    full = full * (scale.reshape(-1, 1) * scale.reshape(1, -1))
                (src if dst is None else dst).copy_(full)

    def nchw_to_nhwc(self, x, out=None):
        if out is None:
            return x.permute(0, 2, 3, 1).contiguous()
        out.copy_(x.permute(0, 2, 3, 1))
        return out

    # diag / Jacobians
    def diag_ggn_linear(self, a, g, alpha, h_w, h_b=None):
        gsq = (g**2).sum(0)  # [B, Do]
        h_w += alpha * (gsq.T @ (a**2)).reshape(-1)
        if h_b is not None:
            h_b += alpha * gsq.sum(0)

    def jac_linear(self, a, g, Js, col0, bcol0=-1):
        S, B, Do = g.shape
        Di = a.shape[1]
        Js[:, :, col0:col0 + Do * Di] = torch.einsum("sbo,bi->bsoi", g, a).reshape(B, S, Do * Di)
        if bcol0 >= 0:
            Js[:, :, bcol0:bcol0 + Do] = g.permute(1, 0, 2)

    def jac_conv(self, x, g, kernel_size, stride, padding, dilation, Js, col0, bcol0=-1):
        S, B, Do = g.shape[:3]
        cols = F.unfold(x, kernel_size, dilation=dilation, padding=padding, stride=stride)  # [B, Dk, L]
        gl = g.reshape(S, B, Do, -1)
        J = torch.einsum("sbol,bkl->bsok", gl, cols)
        Dk = cols.shape[1]
        Js[:, :, col0:col0 + Do * Dk] = J.reshape(B, S, Do * Dk)
        if bcol0 >= 0:
            Js[:, :, bcol0:bcol0 + Do] = gl.sum(-1).permute(1, 0, 2)

    def sq_colsum(self, Js, col0, width, alpha, h):
        P = Js.shape[-1]
        h += alpha * (Js.reshape(-1, P)[:, col0:col0 + width] ** 2).sum(0)

    def bn_act_forward(self, x, scale, shift, relu, addend=None, want_mask=True):
        shape = (1, -1) + (1,) * (x.dim() - 2)
        y = x * scale.reshape(shape).to(x.dtype) + shift.reshape(shape).to(x.dtype)
        if addend is not None:
            y = y + addend
        if relu:
            y = y.clamp_min(0)
            return y, (y > 0 if want_mask else None)
        return y, None

    def vjp_scale_mask(self, g, S, mult, scale, hw, g2=None):
        out = g.reshape(S, -1)
        if g2 is not None:
            out = out + g2.reshape(S, -1)
        if mult is not None:
            out = out * mult.reshape(1, -1).to(g.dtype)
        if scale is not None:
            C = scale.numel()
            out = (out.reshape(S, -1, C, hw) * scale.reshape(1, 1, C, 1).to(g.dtype)).reshape(S, -1)
        return (out + 0).reshape(g.shape)

    def ll_ggn_full(self, phi, probs, has_bias, alpha, H):
        B, D = phi.shape
        pt = torch.cat([phi, torch.ones(B, 1, dtype=phi.dtype)], 1) if has_bias else phi
        Dt = pt.shape[1]
        C = probs.shape[1] if probs is not None else H.shape[0] // Dt
        if probs is None:
            Lam = torch.eye(C, dtype=phi.dtype).expand(B, C, C)
        else:
            Lam = torch.diag_embed(probs) - probs.unsqueeze(2) * probs.unsqueeze(1)
        Haug = alpha * torch.einsum("njk,na,nb->jakb", Lam, pt, pt).reshape(C * Dt, C * Dt)
        ref = torch.tensor([(j * D + a) if a < D else (C * D + j) for j in range(C) for a in range(Dt)])
        H[ref[:, None], ref[None, :]] += Haug
        return H

    # eigensolver
    def syevj(self, A, clamp=True, max_sweeps=0):
        """LAPACK for the eigenpairs, plus the parts of lk_syevj_f32's contract that are not arithmetic: the upper
        triangle only, non-finite entries read as 0, and the status word -- info[0] = 1 when the sweeps ran out or the
        matrix is outside the supported magnitude range (include/laplace_hip.h), info[1] = sweeps executed.  The sweep
        count is modelled, not computed: a matrix with no off-diagonal entry above the solver's convergence floor
        (1e-6 lambda_max) converges in its first sweep, any other needs a sweep that rotates and one that finds nothing
        left."""
        Au = torch.triu(A) + torch.triu(A, 1).T
        fp32 = A.dtype == torch.float32
        Au = torch.where(torch.isfinite(Au) & ((Au.abs() <= 3.0e38) | (not fp32)), Au, torch.zeros_like(Au))
        n = Au.shape[0]
        info = torch.zeros(2, dtype=torch.int32)
        amax = float(Au.abs().max()) if n else 0.0
        if fp32 and n and (float(Au.double().abs().sum(1).max()) >= 3.0e38 or 0.0 < amax < 2.0 ** -126):
            info[0] = 1  # out of range: reported, the outputs are finite placeholders
            return torch.zeros(n, dtype=A.dtype), torch.eye(n, dtype=A.dtype), info
        w, Q = torch.linalg.eigh(Au)
        scale = max(float(w.abs().max()), float(Au.diagonal().abs().max())) if n else 0.0
        off = float((Au - torch.diag(Au.diagonal())).abs().max()) if n else 0.0
        need = 1 if off <= 1e-6 * scale else 2
        done = need if max_sweeps <= 0 else min(need, int(max_sweeps))
        info[0], info[1] = (0 if done >= need else 1), done
        if clamp:
            w = w.clamp(min=0.0)
        return torch.nan_to_num(w), torch.nan_to_num(Q), info

    pixgram_max_hw = 25  # larger than the product's 16 so that the 5x5 test fixture exercises the pixel-pair path

    def pixgram_accumulate(self, x, alpha, Cp):
        X = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)
        Cp += alpha * torch.triu(X.T @ X)  # upper only, like the fused accumulators
        return Cp

    def pixgram_assemble(self, Cp, H, W, Cin, alpha, A_native):
        full = torch.triu(Cp) + torch.triu(Cp, 1).T
        Cp.copy_(full)
        C6 = full.reshape(H, W, Cin, H, W, Cin)
        for d in range(9):
            dy, dx = d // 3 - 1, d % 3 - 1
            for e in range(9):
                ey, ex = e // 3 - 1, e % 3 - 1
                blk = torch.zeros(Cin, Cin, dtype=Cp.dtype)
                for py in range(H):
                    for px in range(W):
                        ay, ax, by, bx = py + dy, px + dx, py + ey, px + ex
                        if 0 <= ay < H and 0 <= ax < W and 0 <= by < H and 0 <= bx < W:
                            blk += C6[ay, ax, :, by, bx, :]
                A_native[d * Cin:(d + 1) * Cin, e * Cin:(e + 1) * Cin] += alpha * blk
        return A_native

    _HALF = [(0, 0), (0, 1), (0, 2)] + [(1, dx) for dx in range(-2, 3)] + [(2, dx) for dx in range(-2, 3)]

    def pixpair_plan(self, H, W, Cin, dev):
        if Cin < 8 or Cin % 8:  # (the product needs Cin % 64 == 0; the emulation only mirrors the structure)
            return None
        slots, n = {}, 0
        for y in range(H):
            for x in range(W):
                for h, (dy, dx) in enumerate(self._HALF):
                    if 0 <= y + dy < H and 0 <= x + dx < W:
                        slots[(y * W + x, h)] = n
                        n += 1
        return (n, None, slots)

    def pixpair_accumulate(self, x, alpha, blocks, plan):
        return self.pixpair_accumulate_nhwc(x.permute(0, 2, 3, 1), alpha, blocks, plan)

    def pixpair_accumulate_nhwc(self, xh, alpha, blocks, plan):
        B, H, W, Cin = xh.shape
        xh = xh.reshape(B, H * W, Cin)
        blk = blocks.view(plan[0], Cin, Cin)
        for (q, h), slot in plan[2].items():
            dy, dx = self._HALF[h]
            q2 = q + dy * W + dx
            blk[slot] += alpha * xh[:, q, :].T @ xh[:, q2, :]
        return blocks

    use_pixpair16 = True
    use_pixpair13 = True

    def pixpair_accumulate_split(self, xs, alpha, blocks, plan):
        return self.pixpair_accumulate_nhwc(xs.float(), alpha, blocks, plan)

    def pixpair_assemble(self, blocks, plan, H, W, Cin, alpha, A_native, blocks2=None, upper_only=False):
        if blocks2 is not None:
            blocks = blocks + blocks2
        blk = blocks.view(plan[0], Cin, Cin)
        for d in range(9):
            dy, dx = d // 3 - 1, d % 3 - 1
            for e in range(9):
                ey, ex = e // 3 - 1, e % 3 - 1
                Dy, Dx = ey - dy, ex - dx
                flip = Dy < 0 or (Dy == 0 and Dx < 0)
                h = self._HALF.index((-Dy, -Dx) if flip else (Dy, Dx))
                acc = torch.zeros(Cin, Cin, dtype=blocks.dtype)
                for py in range(H):
                    for px in range(W):
                        ay, ax, by, bx = py + dy, px + dx, py + ey, px + ex
                        if 0 <= ay < H and 0 <= ax < W and 0 <= by < H and 0 <= bx < W:
                            q = (by * W + bx) if flip else (ay * W + ax)
                            b_ = blk[plan[2][(q, h)]]
                            acc += b_.T if flip else b_
                A_native[d * Cin:(d + 1) * Cin, e * Cin:(e + 1) * Cin] += alpha * acc
        return A_native

    def syevj_batched(self, mats, clamp=True, max_sweeps=0, streams=None):
        return [self.syevj(A, clamp, max_sweeps) for A in mats]

    # logdet
    def kron_logdet(self, l1, l2, delta, damping=False, want_grads=False):
        d = delta.reshape(())
        if l2 is None:
            M = l1 + d
            out = torch.log(M).sum().reshape(1)
            if not want_grads:
                return out, None, None, None
            return out, 1.0 / M, None, (1.0 / M).sum().reshape(1)
        if damping:
            sd = d.sqrt()
            return torch.log(torch.outer(l1 + sd, l2 + sd)).sum().reshape(1), None, None, None
        M = torch.outer(l1, l2) + d
        out = torch.log(M).sum().reshape(1)
        if not want_grads:
            return out, None, None, None
        inv = 1.0 / M
        return out, (inv * l2.view(1, -1)).sum(1), (inv * l1.view(-1, 1)).sum(0), inv.sum().reshape(1)

    # eigenvalue algebra of KronDecomposed._bmm (csrc/lk_gemm.hip)
    def kron_pow(self, l1, l2, delta, exponent, damping=False):
        """lk_kron_pow_f32: (l1 (x) l2 + delta)^e as [n1, n2]; damping: ((l1 + sqrt(delta)) (x) (l2 + sqrt(delta)))^e;
        l2 None: (l1 + delta)^e as [n1]"""
        d = delta.detach().reshape(-1)[0].to(l1.dtype)
        if l2 is None:
            return (l1 + d) ** exponent
        if damping:
            sd = d.sqrt()
            return torch.outer(l1 + sd, l2 + sd) ** exponent
        return (torch.outer(l1, l2) + d) ** exponent

    def kron_sandwich(self, W, col0, P, R, Q1, Q2, lam, out):
        """out[r, col0:col0+p] = vec(Q1 ((Q1^T W_r Q2) (.) lam) Q2^T), W_r = W[r, col0:col0+p] as [p_in, p_out];
        Q2 None: ((W_r Q1) (.) lam) Q1^T.  The other columns of ``out`` are not touched."""
        Wv, Ov = W.reshape(R, P), out.view(R, P)
        if Q2 is None:
            p = Q1.shape[0]
            Ov[:, col0:col0 + p] = ((Wv[:, col0:col0 + p] @ Q1) * lam.reshape(1, p)) @ Q1.T
            return out
        pi, po = Q1.shape[0], Q2.shape[0]
        Wr = Wv[:, col0:col0 + pi * po].reshape(R, pi, po)
        M = (Q1.T @ Wr @ Q2) * lam.reshape(1, pi, po)
        Ov[:, col0:col0 + pi * po] = (Q1 @ M @ Q2.T).reshape(R, pi * po)
        return out

    quadform_shared_max_outputs = 10

    def kron_quadform_shared(self, u, v, l1, l2, delta, fvar, seed_major=False):
        if seed_major:
            u = u.permute(1, 0, 2, 3)
        assert u.shape[1] <= self.quadform_shared_max_outputs, "the HIP kernel holds at most 10 outputs"
        M = torch.einsum("ncol,nil->ncoi", u, v)
        fvar += torch.einsum("ncoi,nkoi,oi->nck", M, M, 1.0 / (torch.outer(l1, l2) + delta.reshape(())))
        return fvar

    use_quad_planes = True

    def kron_quadform_shared_planes(self, u, v, l1, l2, delta, fvar, C):
        """lk_kron_quadform_shared_planes_f16x2: u SplitTensor [C * B, Do, L] (one scale), v SplitTensor [B, Dk, L]"""
        from laplace_amd._lib import _one_scale

        _one_scale(u, "kron_quadform_shared_planes (u)")
        CB, Do, L = u.shape
        B = v.shape[0]
        assert CB == C * B and v.shape[2] == L and L % 16 == 0 and Do % 32 == 0 and C <= self.quadform_shared_max_outputs
        uu = u.float().reshape(C, B, Do, L).permute(1, 0, 2, 3)
        M = torch.einsum("ncol,nil->ncoi", uu, v.float())
        fvar += torch.einsum("ncoi,nkoi,oi->nck", M, M, 1.0 / (torch.outer(l1, l2) + delta.reshape(())))
        return fvar

    def diag_quadform_shared(self, u, v, var_w, fvar):
        assert u.shape[1] <= self.quadform_shared_max_outputs, "the HIP kernel holds at most 10 outputs"
        M = torch.einsum("ncol,nil->ncoi", u, v)
        fvar += torch.einsum("ncoi,nkoi,oi->nck", M, M, var_w)
        return fvar

    def diag_ggn_shared(self, u, v, alpha, h):
        M = torch.einsum("nsol,nil->nsoi", u, v)
        h += alpha * (M * M).sum((0, 1)).reshape(-1)
        return h

    def kron_logdet_blocks(self, blocks, deltas, scale=None, want_grads=False):
        s = 1.0 if scale is None else scale.reshape(()).double()
        out = torch.zeros((), dtype=torch.float64)
        dd, ds = [], torch.zeros((), dtype=torch.float64)
        for ls, d in zip(blocks, deltas.double()):
            lam = ls[0].double() if len(ls) == 1 else torch.outer(ls[0].double(), ls[1].double())
            M = s * lam + d
            out = out + torch.log(M).sum()
            dd.append((1.0 / M).sum())
            ds = ds + (lam / M).sum()
        f32 = lambda t: t.to(torch.float32).reshape(-1)
        return (f32(out), f32(torch.stack(dd)) if want_grads else None,
                f32(ds) if want_grads and scale is not None else None)

    # predictive
    def kron_quadform_linear(self, u, v, l1, l2, delta, fvar, ub=None, lb=None, delta_b=None):
        w = torch.einsum("ni,oi->no", v**2, 1.0 / (torch.outer(l1, l2) + delta.reshape(())))
        fvar += torch.einsum("cno,kno,no->nck", u, u, w)
        if ub is not None:
            fvar += torch.einsum("cno,kno,o->nck", ub, ub, 1.0 / (lb + delta_b.reshape(())))
        return fvar

    def diag_quadform_linear(self, a, g, var_w, var_b, fvar):
        w = torch.einsum("ni,oi->no", a**2, var_w.reshape(g.shape[2], a.shape[1]))
        fvar += torch.einsum("cno,kno,no->nck", g, g, w)
        if var_b is not None:
            fvar += torch.einsum("cno,kno,o->nck", g, g, var_b)
        return fvar

    def diag_quadform_js(self, Js, var):
        return torch.einsum("ncp,p,nkp->nck", Js, var, Js)

    def jac_last_layer(self, phi, C, has_bias):
        B, D = phi.shape
        eye = torch.eye(C, dtype=phi.dtype)
        Js = (eye[None, :, :, None] * phi[:, None, None, :]).reshape(B, C, -1)
        return torch.cat([Js, eye.expand(B, C, C)], 2) if has_bias else Js

    def dense_quadform_ll(self, phi, Sigma, C, has_bias):
        B, D = phi.shape
        eye = torch.eye(C, dtype=phi.dtype)
        Js = (eye[None, :, :, None] * phi[:, None, None, :]).reshape(B, C, -1)
        if has_bias:
            Js = torch.cat([Js, eye.expand(B, C, C)], 2)
        return torch.einsum("ncp,pq,nkq->nck", Js, Sigma, Js)
