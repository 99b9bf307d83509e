"""Shapes, inputs and float64 references for the norm-tap Jacobian kernel of the NHWC split-fp16 sweep (csrc/lk_normtap.hip) and
the end-to-end fixtures of ``SplitSweep.nhwc_norm_taps`` - shared by tests/test_normtap_fixtures.py (CPU: the table reaches every
path, the references bite) and tests/test_gpu_normtap.py (the device).

A case is a dict: ``Ch`` channels, ``L`` positions, ``S`` seeds, ``B`` samples, ``off`` (1: every buffer starts one element past an
aligned address, fp32 and fp16 alike), ``sexp`` (the scale exponent of the split cotangent), ``affine`` (``mu`` / ``rstd`` given) and
``wcol`` / ``bcol`` (is the column block written).  Every channel count is crossed with the six position counts around the lane
rows ``R`` of ITS launch; ``S``, ``B``, ``off``, ``sexp``, ``affine`` and the column blocks rotate through their values.

``plan(c)`` mirrors the launcher's host arithmetic (vector class, channel lanes, lane rows, seeds per pass) so that the table can
be written without the library; tests/test_normtap_fixtures.py holds it against ``lk_normtap_variant`` for every case.

The error bounds are the arithmetic's, not measured: a term ``g * xhat`` carries at most four roundings (``float(h) + float(l)``,
``x - mu``, ``* rstd``, the product) and the ``L`` terms are added in some order, so
``|Jw - ref| <= (L + 8) 2^-24 sum_l |g| |xhat|`` and, with one rounding per term, ``|Jb - ref| <= (L + 2) 2^-24 sum_l |g|``; the
power-of-two scale is exact.
"""
import torch
from torch import nn

U = 2.0 ** -24
P_EXTRA = 5  # columns of Js beyond the two blocks (P > 2 Ch): they must keep their fill
CHANNELS = (1, 3, 4, 8, 12, 68, 72, 520)


def plan(Ch, off=0):
    """``(vec, channel lanes, lane rows R, seeds per pass SC, channel tiles)`` as csrc/lk_normtap.hip's launcher derives them"""
    vec = 8 if Ch % 8 == 0 and not off else (4 if Ch % 4 == 0 and not off else 1)
    cv, cap = Ch // vec, (64 if vec == 1 else 32)
    cxw = 1
    while cxw < cv and cxw < cap:
        cxw *= 2
    return vec, cxw, 256 // cxw, (4 if vec == 8 else 8), -(-cv // cxw)


def _case(Ch, L, S, B=1, off=0, sexp=12, affine=True, wcol=True, bcol=True):
    return dict(Ch=Ch, L=L, S=S, B=B, off=off, sexp=sexp, affine=affine, wcol=wcol, bcol=bcol)


CASES = []
_n = 0
for _i, _ch in enumerate(CHANNELS):
    for _j in range(6):
        _off = int(_n % 4 == 3)
        _, _, _R, _SC, _ = plan(_ch, _off)
        _L = (1, 2, _R - 1, _R, _R + 1, 2 * _R + 3)[_j]
        _S = (1, 2, 9, 17, _SC - 1, _SC, _SC + 1)[_n % 7]
        _cols = ((True, True), (True, False), (False, True), (True, True))[_n % 4 if _n % 8 < 4 else 0]
        CASES.append(_case(_ch, _L, _S, B=(1, 3)[(_i + _j) % 2], off=_off, sexp=(-3, 0, 12)[_n % 3], affine=_n % 5 != 0,
                           wcol=_cols[0], bcol=_cols[1]))
        _n += 1
CASES += [
    # an unaligned base with channel counts that would otherwise take the wide loads
    _case(8, 5, 9, B=3, off=1), _case(12, 7, 5, B=1, off=1, affine=False), _case(72, 19, 2, B=3, off=1, sexp=0),
    _case(520, 3, 3, B=1, off=1, sexp=-3),
    # two channel lanes (the table's channel counts leave that depth of the shuffle tree out)
    _case(16, 131, 2, B=3, sexp=0),
    # enough (sample, channel tile) pairs that the seeds stay in one slice: the seed loop ends one short of, at and one past SC
    _case(8, 2, 3, B=512), _case(8, 2, 4, B=512, affine=False), _case(8, 2, 5, B=512, sexp=0),
    _case(4, 2, 7, B=512), _case(4, 2, 8, B=512), _case(4, 2, 9, B=512, sexp=0), _case(3, 2, 9, B=512, off=1),
    # half as many: two slices of 5 and 4 seeds (split AND more than one pass in a slice, with a remainder)
    _case(8, 3, 9, B=256), _case(72, 2, 9, B=256, sexp=-3),
]


def case_id(c):
    return (f"Ch{c['Ch']}-L{c['L']}-S{c['S']}-B{c['B']}-e{c['sexp']}" + ("" if c["affine"] else "-noaffine")
            + ("" if c["wcol"] else "-now") + ("" if c["bcol"] else "-nob") + ("-unaligned" if c["off"] else ""))


def columns(c):
    """``(P, wcol0, bcol0)``: the bias block first, a gap, the weight block, a tail - or -1 for an absent block"""
    Ch = c["Ch"]
    return 2 * Ch + P_EXTRA, (Ch + 2 if c["wcol"] else -1), (1 if c["bcol"] else -1)


def make_inputs(c, gen):
    """``(g, x, mu, rstd)`` on the CPU: the cotangent ``[S*B, L, Ch]`` as a ONE-scale split tensor with scale exponent ``c['sexp']``
    (full-mantissa values, cut with the emulation's ``split``), fp32 ``x`` ``[B, L, Ch]``, and ``mu``, ``rstd`` ``[Ch]`` or None"""
    from tests.emulated_kernels import EmulatedKernels

    S, B, L, Ch = c["S"], c["B"], c["L"], c["Ch"]
    g32 = torch.randn(S * B, L, Ch, generator=gen)
    g32 = g32 / g32.abs().max() * 1.5 * 2.0 ** (14 - c["sexp"])  # max|g| 2^sexp in [2^14, 2^15)
    assert EmulatedKernels._sexp_for(g32.abs().max()) == c["sexp"]
    g = EmulatedKernels._split(g32, c["sexp"])
    x = torch.randn(B, L, Ch, generator=gen) * 2.0 + 0.5
    mu = rstd = None
    if c["affine"]:
        mu = torch.randn(Ch, generator=gen) * 0.5
        rstd = torch.rsqrt(torch.rand(Ch, generator=gen) + 0.5)
    return g, x, mu, rstd


def make_integer_inputs(c, gen):
    """integer-valued planes with a zero low plane, integer ``x``, ``mu = 0`` and ``rstd = 1`` (or null): every product and every
    partial sum is an integer below 2^24, so any summation order gives the same bits"""
    from laplace_amd._lib import SplitTensor

    S, B, L, Ch = c["S"], c["B"], c["L"], c["Ch"]
    h = torch.randint(-8, 9, (S * B, L, Ch), generator=gen).half()
    g = SplitTensor(torch.stack([h, torch.zeros_like(h)]), torch.tensor([c["sexp"]], dtype=torch.int32))
    x = torch.randint(-8, 9, (B, L, Ch), generator=gen).float()
    mu, rstd = (torch.zeros(Ch), torch.ones(Ch)) if c["affine"] else (None, None)
    return g, x, mu, rstd


def planes_value(planes, sexp):
    """``(h.double() + l.double()) * 2^-sexp``: what the split tensor holds, exactly"""
    return (planes[0].detach().cpu().double() + planes[1].detach().cpu().double()) * 2.0 ** -int(sexp.reshape(-1)[0])


def reference(c, planes, sexp, x, mu, rstd):
    """``(Jw, Jb, bound_w, bound_b)`` in float64, each ``[B, S, Ch]``, from the SAME planes and the SAME fp32 ``x``, ``mu``, ``rstd``"""
    S, B, L, Ch = c["S"], c["B"], c["L"], c["Ch"]
    g = planes_value(planes, sexp).reshape(S, B, L, Ch)
    xhat = x.detach().cpu().double().reshape(B, L, Ch)
    if mu is not None:
        xhat = (xhat - mu.detach().cpu().double()) * rstd.detach().cpu().double()
    Jw = (g * xhat).sum(2).permute(1, 0, 2)
    Jb = g.sum(2).permute(1, 0, 2)
    bw = (L + 8) * U * (g.abs() * xhat.abs()).sum(2).permute(1, 0, 2)
    bb = (L + 2) * U * g.abs().sum(2).permute(1, 0, 2)
    return Jw, Jb, bw, bb


# ---- end-to-end fixtures --------------------------------------------------------------------------------------------------------
# Every normalisation parameter is tracked.  The golden model ``normbn`` (tests/norm_fixtures.py) has 4-channel convolutions, which
# the implicit-GEMM kernels do not cover: it stays on the NCHW sweep whatever the switch says, and the tests hold its numbers
# against the goldens on that route.  ``bnres32`` is the same architecture at 32 channels, which the NHWC walk admits.
#   bnres32:  conv 3 -> 32 (bias), torchvision-style BatchNorm residual block (in-place add / ReLU), pool, linear
#   bn2stage: ResNet stem and two BasicBlocks (32 -> 32, 32 -> 64 stride 2 with a 1x1 down-sampling branch) with ReLU at 8 x 8:
#             a tapped BatchNorm behind a tapped stride-1, a strided 3x3 and a strided 1x1 convolution, and behind the stem
#   gnblock:  the same stem and one BasicBlock with GroupNorm(4, 32) and tracked affine parameters
# A ReLU mask is a step function: the float64 pre-activations must stay clear of zero (a property of the seed, asserted by
# tests/test_normtap_fixtures.py), or two correct passes may differ by O(1).
E2E = ("bnres32", "bn2stage", "gnblock")
E2E_SEED = {"bnres32": 11, "bn2stage": 12, "gnblock": 13}
E2E_CLASSES = 3
RELU_MARGIN = 1e-5  # fp32 moves a pre-activation of these nets (values of order 1) by a few 1e-7: none can change sides


class _Stages(nn.Module):
    def __init__(self, norm, blocks):
        super().__init__()
        from laplace_amd.nets import BasicBlock, norm_layer

        self.act = torch.relu
        self.conv1 = nn.Conv2d(3, 32, 3, 1, 1, bias=False)
        self.bn1 = nn.GroupNorm(4, 32) if norm == "gn" else norm_layer(norm, 32)
        cin, layers = 32, []
        for cout, stride in blocks:
            layers.append(BasicBlock(cin, cout, stride, torch.relu, norm))
            cin = cout
        self.layers = nn.Sequential(*layers)
        if norm == "gn":
            for m in self.layers.modules():
                if isinstance(m, nn.GroupNorm):
                    m.num_groups = 4
        self.pool, self.fc = nn.AdaptiveAvgPool2d(1), nn.Linear(cin, E2E_CLASSES)

    def forward(self, x):
        x = self.act(self.bn1(self.conv1(x)))
        return self.fc(torch.flatten(self.pool(self.layers(x)), 1))


def e2e_fixture(name):
    """``(float64 CPU model in eval mode, every parameter tracked, X [4, 3, 8, 8], y [4])``"""
    from tests.norm_fixtures import _BNResBlock, _stir

    prev = torch.random.get_rng_state()
    torch.manual_seed(E2E_SEED[name])
    try:
        if name == "bnres32":
            m = nn.Sequential(nn.Conv2d(3, 32, 3, padding=1), _BNResBlock(32), nn.AdaptiveAvgPool2d(1), nn.Flatten(),
                              nn.Linear(32, E2E_CLASSES))
        elif name == "bn2stage":
            m = _Stages("bn", ((32, 1), (64, 2)))
        else:
            m = _Stages("gn", ((32, 1),))
        m = _stir(m).double()
        X = torch.randn(4, 3, 8, 8, dtype=torch.float64)
        y = torch.randint(E2E_CLASSES, (4,))
    finally:
        torch.random.set_rng_state(prev)
    return m, X, y


NORMS = (nn.BatchNorm2d, nn.GroupNorm)


def e2e_taps(model):
    """the modules a sweep taps: Linear and convolution layers, and the normalisation layers behind them"""
    return {n: m for n, m in model.named_modules() if isinstance(m, (nn.Conv2d, nn.Linear) + NORMS)}


def norm_names(model):
    return [n for n, m in model.named_modules() if isinstance(m, NORMS)]


def blocks(model):
    """(name, first column, one past the last) of every tracked parameter in the order of the Jacobian's columns"""
    out, at = [], 0
    for n, p in model.named_parameters():
        if p.requires_grad:
            out.append((n, at, at + p.numel()))
            at += p.numel()
    return out


def e2e_relu_margin(name):
    """smallest |pre-activation| of a ReLU in the float64 forward, and how many were looked at"""
    m, X, _ = e2e_fixture(name)
    margin, seen = [float("inf")], [0]

    def noting(z):
        margin[0] = min(margin[0], z.detach().abs().min().item())
        seen[0] += z.numel()
        return torch.relu(z)

    hooks = [mod.register_forward_pre_hook(lambda mod_, i: (noting(i[0]), None)[1]) for mod in m.modules() if isinstance(mod, nn.ReLU)]
    for mod in m.modules():
        if getattr(mod, "act", None) is torch.relu:
            mod.act = noting
    with torch.no_grad():
        m(X)
    for h in hooks:
        h.remove()
    return margin[0], seen[0]


def resnet18_fixture():
    """``(fp32 model, X [2, 3, 16, 16], y)``: ``nets.ResNet18`` with tracked BatchNorm and a smooth activation (two separately
    executed passes are compared), stirred statistics"""
    from laplace_amd.nets import ResNet18
    from tests.norm_fixtures import _stir

    prev = torch.random.get_rng_state()
    torch.manual_seed(21)
    try:
        m = _stir(ResNet18(num_classes=4, freeze_bn=False, act=torch.tanh))
        X, y = torch.randn(2, 3, 16, 16), torch.randint(4, (2,))
    finally:
        torch.random.set_rng_state(prev)
    return m.eval(), X, y
