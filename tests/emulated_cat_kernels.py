"""``EmulatedPoolKernels`` plus channel concatenation on NHWC maps (csrc/lk_cat.hip) in stock torch, for the CPU test tier.

TEST INFRASTRUCTURE.  The stock emulation (tests/emulated_kernels.py) and the pooling one deliberately have no concatenation
methods: a ``SplitSweep`` on them keeps a model with a ``torch.cat`` on the NCHW sweep.  ``cat_vjp`` states the kernel's rule in
torch: the fp32 value of every part as ``SplitTensor.float()`` forms it, summed left to right in the listed order, and only then
the slice.  Two MUTANTS for tests/test_cat_fixtures.py: ``ignore_c0`` reads the slice at channel 0, ``reverse_sum`` sums right to
left.  ``seen`` records the calls.
"""
import torch

from laplace_amd._lib import SplitTensor
from tests.emulated_pool_kernels import EmulatedPoolKernels


def part_value(p):
    """fp32 value of a cotangent part: an fp32 tensor as it is, a split tensor as ``SplitTensor.float()`` forms it"""
    return p.float() if isinstance(p, SplitTensor) else p


def cat_vjp_math(parts, c0, Cs, ignore_c0=False, reverse_sum=False):
    """``sum_p value_p[..., c0:c0 + Cs]`` in fp32, left to right in the listed order (the rule of lk_cat_vjp_nhwc_f32)"""
    vals = [part_value(p)[..., (0 if ignore_c0 else c0):(0 if ignore_c0 else c0) + Cs] for p in parts]
    if reverse_sum:
        vals = vals[::-1]
    acc = vals[0]
    for v in vals[1:]:
        acc = acc + v
    return acc.contiguous()


class EmulatedCatKernels(EmulatedPoolKernels):
    CAT_MAX_PARTS = 4
    ignore_c0 = False
    reverse_sum = False

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.seen = []

    def cat_forward(self, sources_nhwc):
        sources = list(sources_nhwc)
        assert sources and all(x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous() for x in sources)
        assert all(x.shape[:3] == sources[0].shape[:3] for x in sources)
        self.seen.append(("forward", tuple(int(x.shape[3]) for x in sources)))
        return torch.cat(sources, 3)

    def cat_vjp(self, parts, c0, Cs, amax=None):
        parts = list(parts)
        assert 1 <= len(parts) <= self.CAT_MAX_PARTS, len(parts)
        for p in parts:
            assert tuple(p.shape) == tuple(parts[0].shape) and len(p.shape) == 4
            if isinstance(p, SplitTensor):
                assert p.sexp.numel() == 1 and not p.chunked and p.planes.is_contiguous()
            else:
                assert p.dtype == torch.float32 and p.is_contiguous()
        assert Cs >= 1 and c0 >= 0 and c0 + Cs <= parts[0].shape[3]
        self.seen.append(("vjp", tuple("split" if isinstance(p, SplitTensor) else "f32" for p in parts), int(c0), int(Cs),
                          amax is not None))
        dx = cat_vjp_math(parts, c0, Cs, self.ignore_c0, self.reverse_sum)
        if amax is not None and dx.numel():
            amax.copy_(torch.maximum(amax.reshape(1), dx.abs().max().reshape(1).float()))
        return dx

    def cat_variant(self, nparts, split_mask, R, Ct, c0, Cs, aligned=True):
        """the host-only launch plan of the library itself (no device call)"""
        from laplace_amd._lib import HipKernels

        return HipKernels().cat_variant(nparts, split_mask, R, Ct, c0, Cs, aligned)
