"""``EmulatedMulKernels`` on top of ``EmulatedSliceKernels`` plus the squeeze-and-excitation gate kernels (csrc/lk_gate.hip) in stock
torch, for the CPU test tier.

TEST INFRASTRUCTURE.  The emulations below this one deliberately have no ``gate_reduce`` / ``gate_vjp``: a ``SplitSweep`` on them
keeps a model with a product on the NCHW sweep whatever ``nhwc_mul`` says.  Both methods state the kernels' rule through
tests/gate_fixtures.torch_math - a split cotangent enters as ``SplitTensor.float()`` forms it - with the binding's own checks on
what belongs together; ``mutant`` selects one of that function's MUTANTS for tests/test_gate_fixtures.py.  ``seen`` records the
calls (the product kernel's ``mul_vjp`` of the NCHW route among them).
"""
import torch

from laplace_amd._lib import SplitTensor
from tests import gate_fixtures as gf
from tests.emulated_mul_kernels import EmulatedMulKernels
from tests.emulated_slice_kernels import EmulatedSliceKernels


class EmulatedGateKernels(EmulatedMulKernels, EmulatedSliceKernels):
    mutant = None

    @staticmethod
    def _g(g):
        if isinstance(g, SplitTensor):
            assert g.sexp.numel() == 1 and not g.chunked and g.planes.is_contiguous()
            return g.float(), "split"
        assert g.dtype == torch.float32 and g.is_contiguous()
        return g, "f32"

    def gate_reduce(self, g, x, S):
        gv, form = self._g(g)
        S = int(S)
        assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4 and gv.dim() == 4
        B, H, W, C = (int(d) for d in x.shape)
        assert S >= 1 and tuple(gv.shape) == (S * B, H, W, C)
        self.seen.append(("gate_reduce", form, S, B, H * W, C))
        c = dict(kind="reduce", S=S, B=B, P=H * W, C=C)
        ds = gf.torch_math(c, dict(g=gv.reshape(S, B, H * W, C), x=x.reshape(B, H * W, C)), self.mutant)
        return ds.reshape(S * B, C).contiguous()

    def gate_vjp(self, g, gate, r, S, amax=None):
        gv, form = self._g(g)
        S = int(S)
        assert gate.dtype == torch.float32 and gate.is_contiguous() and gate.dim() == 2 and gv.dim() == 4
        N, H, W, C = (int(d) for d in gv.shape)
        B = int(gate.shape[0])
        assert S >= 1 and N == S * B and gate.shape[1] == C
        assert r is None or (r.dtype == torch.float32 and r.is_contiguous() and tuple(r.shape) == (N, C))
        assert amax is None or (amax.numel() == 1 and amax.element_size() == 4)
        self.seen.append(("gate_vjp", form, S, B, H * W, C, r is not None, amax is not None))
        c = dict(kind="vjp", S=S, B=B, P=H * W, C=C)
        dx = gf.torch_math(c, dict(g=gv.reshape(S, B, H * W, C), gate=gate, r=None if r is None else r.reshape(S, B, C)),
                           self.mutant).reshape(N, H, W, C).contiguous()
        if amax is not None and dx.numel():
            amax.copy_(torch.maximum(amax.reshape(1), dx.abs().max().reshape(1).float()))
        return dx

    def gate_variant(self, vjp, S, B, P, C, aligned=True):
        """the host-only launch plan of the library itself (no device call)"""
        from laplace_amd._lib import HipKernels

        return HipKernels().gate_variant(vjp, S, B, P, C, aligned)
