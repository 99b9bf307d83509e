"""``EmulatedAttnKernels`` plus the strided attention entry points of csrc/lk_attn.hip (lk_attn_fwd_strided_f32,
lk_attn_vjp_strided_f32) in stock torch, for the CPU test tier.

TEST INFRASTRUCTURE.  With this emulation the STRIDED branch of the sweep's nn.MultiheadAttention rule runs on the CPU: the
methods hold their operands to the device wrapper's contract (``[N, T, H, D]`` views whose rows of ``H D`` floats are contiguous
and one common row stride apart, nothing copied), log the ``data_ptr`` and the row stride of everything they were handed in
``seen`` so that a test can tell a slice of the packed projection from a copy, and write the cotangents into the caller's views -
every element, nothing beside them.  The arithmetic is that of `EmulatedAttnKernels` (``exp(s - lse)``)."""
import torch

from tests.emulated_attn_kernels import EmulatedAttnKernels


class EmulatedMhaKernels(EmulatedAttnKernels):
    @staticmethod
    def _row_stride(shape, *ts):
        N, T, H, D = shape
        lds = set()
        for t in ts:
            assert tuple(t.shape) == tuple(shape) and t.dtype == torch.float32, (tuple(t.shape), tuple(shape))
            sn, st, sh, sd = t.stride()
            assert (D == 1 or sd == 1) and (H == 1 or sh == D) and (N == 1 or sn == T * st), t.stride()
            lds.add(st if T > 1 or N > 1 else H * D)
        assert len(lds) == 1, f"operands with different row strides: {sorted(lds)}"
        ld = lds.pop()
        assert ld >= H * D and ld % 4 == 0 and all(t.data_ptr() % 16 == 0 for t in ts)
        return ld

    def attn_forward_strided(self, q, k, v, scale, causal):
        B, T, H, D = q.shape
        ldq = self._row_stride(q.shape, q, k, v)
        self.seen.append(("forward_strided", ldq, tuple(t.data_ptr() for t in (q, k, v))))
        qh, kh, vh = (t.transpose(1, 2) for t in (q, k, v))
        s = self._scores(qh, kh, scale, causal)
        lse = torch.logsumexp(s, dim=-1)
        o = (torch.exp(s - lse.unsqueeze(-1)) @ vh).transpose(1, 2).contiguous()
        return o, lse

    def attn_vjp_strided(self, go, q, k, v, o, lse, S, scale, causal, dq, dk, dv):
        B, T, H, D = q.shape
        ldq = self._row_stride(q.shape, q, k, v)
        ldd = self._row_stride((S * B, T, H, D), dq, dk, dv)
        assert self._row_stride(q.shape, o) == H * D and self._row_stride((S * B, T, H, D), go) == H * D
        assert tuple(lse.shape) == (B, H, T)
        self.seen.append(("vjp_strided", ldq, ldd, tuple(t.data_ptr() for t in (go, q, k, v, o, dq, dk, dv))))
        qh, kh, vh, oh = (t.transpose(1, 2) for t in (q, k, v, o))
        p = torch.exp(self._scores(qh, kh, scale, causal) - lse.unsqueeze(-1))
        g = go.transpose(1, 2).reshape(S, B, H, T, D)
        dS = p * (g @ vh.transpose(-1, -2) - (g * oh).sum(-1, keepdim=True))
        back = lambda t: t.reshape(S * B, H, T, D).transpose(1, 2)  # noqa: E731
        dq.copy_(back(scale * (dS @ kh)))
        dk.copy_(back(scale * (dS.transpose(-1, -2) @ qh)))
        dv.copy_(back(p.transpose(-1, -2) @ g))
