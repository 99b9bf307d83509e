"""TEST INFRASTRUCTURE: ``EmulatedKernels`` plus the sampled-heads kernel of the `nn` predictive (csrc/lk_nnhead.hip) in stock
torch for the CPU test tier, with the binding's argument checks; ``seen`` records the calls."""
import torch

from tests.emulated_kernels import EmulatedKernels


class EmulatedNnHeadKernels(EmulatedKernels):
    NN_HEAD_MAX_C = 1024

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.seen = []

    def nn_head(self, phi, theta, C, has_bias=True, mode="probs", softmax=False):
        (B, D), S = phi.shape, theta.shape[0]
        assert phi.dtype == theta.dtype == torch.float32 and phi.is_contiguous() and theta.is_contiguous()
        assert 1 <= C <= self.NN_HEAD_MAX_C and theta.shape[1] >= C * D + (C if has_bias else 0)
        self.seen.append((mode, B, C, D, S))
        f = torch.einsum("bd,scd->sbc", phi, theta[:, :C * D].reshape(S, C, D))
        if has_bias:
            f = f + theta[:, None, C * D:C * D + C]
        if mode == "moments":
            return f.mean(0), f.var(0)
        if mode == "samples":
            return f.softmax(-1) if softmax else f
        return f.softmax(-1).mean(0)
