"""TEST INFRASTRUCTURE: ``EmulatedKernels`` plus the joint-covariance kernels of an nn.Linear layer (csrc/lk_joint.hip) in stock
torch for the CPU test tier; ``seen`` records the calls."""
import torch

from tests.emulated_kernels import EmulatedKernels


class EmulatedJointKernels(EmulatedKernels):
    JOINT_MAX_C = 4

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.seen = []

    def _joint(self, mode, u, v, w, ub, bw, cov):
        (C, B, Do), N = u.shape, cov.shape[0]
        assert 1 <= C <= self.JOINT_MAX_C and cov.shape == (B * C, B * C) and u.dtype == v.dtype == torch.float32
        self.seen.append((mode, B, C, Do, v.shape[1]))
        cov += torch.einsum("cno,kmo,ni,mi,oi->ncmk", u, u, v, v, w).reshape(N, N)
        if ub is not None:
            cov += torch.einsum("cno,kmo,o->ncmk", ub, ub, bw).reshape(N, N)
        return cov

    def kron_joint_linear(self, u, v, l1, l2, delta, cov, ub=None, lb=None, delta_b=None):
        bw = None if ub is None else 1.0 / (lb + delta_b.reshape(()))
        return self._joint("kron", u, v, 1.0 / (torch.outer(l1, l2) + delta.reshape(())), ub, bw, cov)

    def diag_joint_linear(self, a, g, var_w, var_b, cov):
        return self._joint("diag", g, a, var_w.reshape(g.shape[2], a.shape[1]), None if var_b is None else g, var_b, cov)
