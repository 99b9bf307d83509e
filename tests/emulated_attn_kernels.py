"""``EmulatedKernels`` plus the attention entry points of csrc/lk_attn.hip in stock torch, for the CPU test tier.

TEST INFRASTRUCTURE.  The stock emulation deliberately has no attention methods: a sweep on it keeps an attention node on the
torch math of its rule.  With this one the KERNEL branch of the rule runs on the CPU - layout detection, the no-copy contract,
the layouts of what comes back.  As the device wrapper, the methods take operands in one of the two layouts as they are (the
``data_ptr`` of every operand they were handed is logged in ``seen``, so that a test can tell a view from a copy), keep ``lse``
instead of the probabilities, and return views in the operands' layout.  The arithmetic is blocked differently from
`laplace_amd.sweep.attn_forward_math` (``exp(s - lse)`` instead of a softmax), so that the two branches can be compared.
"""
import torch

from laplace_amd.sweep import attn_like, attn_operands
from tests.emulated_kernels import EmulatedKernels


class EmulatedAttnKernels(EmulatedKernels):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.seen = []  # (call, layout, data_ptrs of the operands as used)

    @staticmethod
    def _scores(q, k, scale, causal):
        s = (q @ k.transpose(-1, -2)) * scale
        if causal:
            T = q.shape[-2]
            s = s.masked_fill(~torch.ones(T, T, dtype=torch.bool, device=q.device).tril(), float("-inf"))
        return s

    def attn_forward(self, q, k, v, scale, causal):
        layout, (q, k, v) = attn_operands(q, k, v)
        self.seen.append(("forward", layout, tuple(t.data_ptr() for t in (q, k, v))))
        s = self._scores(q, k, scale, causal)
        lse = torch.logsumexp(s, dim=-1)
        o = attn_like(q.shape, layout, q)
        o.copy_(torch.exp(s - lse.unsqueeze(-1)) @ v)
        return o, lse

    def attn_vjp(self, go, q, k, v, o, lse, S, scale, causal):
        layout, (q, k, v, o) = attn_operands(q, k, v, o)
        self.seen.append(("vjp", layout, tuple(t.data_ptr() for t in (go, q, k, v, o))))
        B, H, T, D = q.shape
        assert tuple(go.shape) == (S * B, H, T, D) and tuple(lse.shape) == (B, H, T)
        p = torch.exp(self._scores(q, k, scale, causal) - lse.unsqueeze(-1))
        g = go.reshape(S, B, H, T, D)
        dS = p * (g @ v.transpose(-1, -2) - (g * o).sum(-1, keepdim=True))
        dq, dk, dv = (attn_like(go.shape, layout, go) for _ in range(3))
        dq.copy_((scale * (dS @ k)).reshape(go.shape))
        dk.copy_((scale * (dS.transpose(-1, -2) @ q)).reshape(go.shape))
        dv.copy_((p.transpose(-1, -2) @ g).reshape(go.shape))
        return dq, dk, dv

    def attn_variant(self, S, B, H, T, D, layout=0, causal=False):
        """the host-only launch plan of the library itself (no device call)"""
        from laplace_amd._lib import HipKernels

        return HipKernels().attn_variant(S, B, H, T, D, layout, causal)
