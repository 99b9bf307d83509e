"""Shapes, inputs and float64 references for the depthwise-convolution kernels (csrc/lk_dwconv.hip) - shared by
tests/test_dwconv_fixtures.py (CPU: the table reaches every path, the references bite) and tests/test_gpu_dwconv.py (the device).

A case is a dict: window ``k``, stride ``s``, padding ``p`` (pairs), map ``H`` x ``W`` x ``C``, ``B`` images, ``S`` seeds, ``off`` (1: every
buffer starts one element past an aligned address, fp32 and fp16 alike) and ``bias`` (the forward adds one).  Every geometry of
GEOMETRIES is crossed with the five channel counts (6 takes the scalar path, 68 has more channel vectors than a wave has lanes);
``B``, ``S``, ``off`` and ``bias`` rotate through their values, so that every geometry meets both batch sizes and both alignments and
every value of ``S`` appears with every tap class and stride kind.

The error bounds are derived, not measured.  ``gamma(n) = n u / (1 - n u)``, ``u = 2^-24``, ``T = kh kw``: a ``T``-term fp32 sum of
products in any order, with or without FMA, differs from the exact value by at most ``gamma(T) sum |w| |operand|``; one more
rounding forms ``float(h) + float(l)`` (backward) and one adds the bias (forward), the power-of-two scale is exact, and an
underflowing term loses at most ``2^-126``:  ``|got - ref| <= gamma(T + 2) * sum |w| |operand| + T * 2^-126``.  The bias is one of
the summed terms (operand ``|bias|`` with weight 1): the rounding of the last addition is relative to the whole sum, bias
included, so no fp32 kernel could meet a bound that left it out where the bias dominates a 1 x 1 window.
"""
import torch
import torch.nn.functional as F
from torch import nn

U = 2.0 ** -24  # unit roundoff of fp32
SEEDS_PER_PASS = 4  # DW_SC of csrc/lk_dwconv.hip (tests/test_dwconv_fixtures.py reads it back through lk_dwconv_variant)


def gamma(n):
    return n * U / (1 - n * U)


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _case(k, s, p, hw, C=8, B=1, S=2, off=0, bias=False):
    return dict(k=_pair(k), s=_pair(s), p=_pair(p), H=_pair(hw)[0], W=_pair(hw)[1], C=C, B=B, S=S, off=off, bias=bias)


GEOMETRIES = [  # (window, stride, padding, map): why
    ((3, 3), 1, 1, (5, 7)),  # the common geometry
    ((3, 3), 2, 1, (8, 8)),  # stride with (H + 2p - k) % s != 0: the last row and column are reached by fewer taps
    ((3, 3), 2, 0, (8, 8)),  # row and column 7 receive NO tap: dx must be 0 there
    ((3, 3), 2, 1, (7, 5)),  # odd map under stride
    ((5, 5), 1, 2, (6, 6)),  # tap class 1
    ((5, 5), 2, 2, (9, 7)),  # tap class 1 with stride
    ((3, 5), (1, 2), (1, 2), (6, 9)),  # rectangular window, mixed strides
    ((2, 2), 2, 0, (6, 6)),  # even window, no overlap
    ((2, 2), 1, 1, (4, 4)),  # even window with padding
    ((1, 1), 1, 0, (3, 3)),  # a per-channel scale
    ((3, 3), 1, 1, (1, 1)),  # the map is smaller than the window
    ((3, 3), 3, 1, (7, 7)),  # stride equals window
]
_CS, _BS = (4, 6, 8, 12, 68), (1, 3)
_SS = (1, 2, 9, 17, SEEDS_PER_PASS - 1, SEEDS_PER_PASS, SEEDS_PER_PASS + 1)

CASES = []
for _i, (_k, _s, _p, _hw) in enumerate(GEOMETRIES):
    for _j, _c in enumerate(_CS):
        _n = _i * len(_CS) + _j
        CASES.append(_case(_k, _s, _p, _hw, C=_c, B=_BS[(_i + _j) % 2], S=_SS[_n % len(_SS)], off=int(_n % 4 == 3),
                           bias=_n % 2 == 0))
CASES += [
    # an unaligned base with a channel count that would otherwise take the wide loads, both tap classes, with and without stride
    _case(3, 1, 1, (5, 7), C=8, B=3, S=9, off=1, bias=True), _case(3, 2, 1, 8, C=12, B=1, S=17, off=1),
    _case(5, 1, 2, 6, C=4, B=3, S=2, off=1), _case(5, 2, 2, (9, 7), C=68, B=1, S=5, off=1, bias=True),
    # enough lanes that the seeds stay in one slice: the seed loop ends one short of, at, and one past the seeds per pass
    _case(3, 1, 1, 32, C=256, B=2, S=SEEDS_PER_PASS - 1, bias=True),
    _case(3, 2, 1, 32, C=256, B=2, S=SEEDS_PER_PASS),
    _case(5, 1, 2, 32, C=256, B=2, S=SEEDS_PER_PASS + 1),
    # half as many lanes: two slices of 5 and 4 seeds (split AND more than one pass, with a remainder, in both slices)
    _case(3, 2, 1, 32, C=256, B=1, S=9, bias=True),
]


def case_id(c):
    g = f"k{c['k'][0]}x{c['k'][1]}s{c['s'][0]}x{c['s'][1]}p{c['p'][0]}x{c['p'][1]}"
    return f"{g}-{c['H']}x{c['W']}x{c['C']}-B{c['B']}-S{c['S']}" + ("-bias" if c["bias"] else "") + ("-unaligned" if c["off"] else "")


def out_hw(c):
    return ((c["H"] + 2 * c["p"][0] - c["k"][0]) // c["s"][0] + 1, (c["W"] + 2 * c["p"][1] - c["k"][1]) // c["s"][1] + 1)


def taps(c):
    return c["k"][0] * c["k"][1]


def strided(c):
    return c["s"] != (1, 1)


def make_inputs(c, gen):
    """``(x [B, H, W, C], w_tap [T, C], bias [C] or None, g)`` on the CPU: fp32 ``randn``, and the cotangent ``[S*B, OH, OW, C]`` as a
    ONE-scale split tensor cut from ``randn`` with the emulation's ``split``"""
    from tests.emulated_kernels import EmulatedKernels

    OH, OW = out_hw(c)
    x = torch.randn(c["B"], c["H"], c["W"], c["C"], generator=gen)
    w_tap = torch.randn(taps(c), c["C"], generator=gen)
    bias = torch.randn(c["C"], generator=gen) if c["bias"] else None
    g32 = torch.randn(c["S"] * c["B"], OH, OW, c["C"], generator=gen)
    g = EmulatedKernels._split(g32, EmulatedKernels._sexp_for(g32.abs().max()))
    return x, w_tap, bias, g


def _weight64(c, w_tap):
    """``[C, 1, kh, kw]`` float64 from the SAME fp32 ``w_tap``"""
    return w_tap.detach().cpu().double().t().reshape(c["C"], 1, *c["k"])


def forward_reference(c, x, w_tap, bias):
    """``(y, bound)`` in float64, ``[B, OH, OW, C]``, from the same fp32 operands"""
    x64, w64 = x.detach().cpu().double().permute(0, 3, 1, 2), _weight64(c, w_tap)
    b64 = None if bias is None else bias.detach().cpu().double()
    y = F.conv2d(x64, w64, b64, c["s"], c["p"], 1, c["C"])
    mag = F.conv2d(x64.abs(), w64.abs(), None if b64 is None else b64.abs(), c["s"], c["p"], 1, c["C"])
    T = taps(c)
    return y.permute(0, 2, 3, 1), gamma(T + 2) * mag.permute(0, 2, 3, 1) + T * 2.0 ** -126


def planes_value(planes, sexp):
    """``(h.double() + l.double()) * 2^-sexp``: what the split tensor holds, exactly"""
    return (planes[0].detach().cpu().double() + planes[1].detach().cpu().double()) * 2.0 ** -int(sexp.reshape(-1)[0])


def backward_reference(c, planes, sexp, w_tap):
    """``(dx, bound)`` in float64, ``[S, B, H, W, C]``, from the SAME planes and ``w_tap``: the SCATTER definition of the transposed
    convolution - every output pixel adds ``w[dy, dx] * g`` to the input pixel its tap ``(dy, dx)`` read - written independently
    of the gather formula of the kernel"""
    S, B, (OH, OW), (kh, kw), (sh, sw), (ph, pw) = c["S"], c["B"], out_hw(c), c["k"], c["s"], c["p"]
    g64 = planes_value(planes, sexp).reshape(S * B, OH, OW, c["C"])
    w64 = w_tap.detach().cpu().double()

    def scatter(g_, w_):
        out = torch.zeros(S * B, c["H"] + 2 * ph, c["W"] + 2 * pw, c["C"], dtype=torch.float64)
        for dy in range(kh):
            for dx in range(kw):
                out[:, dy:dy + (OH - 1) * sh + 1:sh, dx:dx + (OW - 1) * sw + 1:sw, :] += w_[dy * kw + dx] * g_
        return out[:, ph:ph + c["H"], pw:pw + c["W"], :].reshape(S, B, c["H"], c["W"], c["C"])

    T = taps(c)
    return scatter(g64, w64), gamma(T + 2) * scatter(g64.abs(), w64.abs()) + T * 2.0 ** -126


# ---- end-to-end fixtures ------------------------------------------------------------------------------------------------------------
# (a) MobileNetV1(width=0.25) cut to its first six blocks, tanh: generic real weights, nothing decides.
# (b) the same with ReLU.  A ReLU mask decides: an fp32 forward may put a pre-activation on the other side of zero than the float64
#     reference does, and the cotangents of the two passes then differ by O(1) for a reason that is no fault of the code under
#     test.  The fixture has 2.7e5 pre-activations per minibatch; no seed keeps that many generic reals 1e-3 of the map's maximum
#     clear of zero.  So, as tests/pool_fixtures.py does, the maps that decide lie on a dyadic lattice: inputs are multiples of 1/8,
#     filters have two entries of +-1 (BatchNorm: zero mean, running_var + eps = 1), and the BatchNorm offset is half the lattice
#     step of its map, so that no pre-activation is closer to zero than that.  Every such layer halves the step, and the gap
#     must stay above 1e-3 of the map's maximum, so only the first three ReLU layers (stem, depthwise 1, pointwise 1: the masks
#     the first depthwise backward-data feeds and is fed by) carry signed filters; the filters behind them are non-negative (two
#     entries of +1, BatchNorm weight 1/2) with a positive offset, which keeps every pre-activation at least the offset above zero.
#     The fixture's SEED picks the filters; tests/test_dwconv_fixtures.py asserts the gaps on the float64 forward.
# (c) two MobileNetV2 inverted residuals (32 channels, identity shortcuts; the first without expansion, so that the ADD join's
#     cotangent lands beside a depthwise backward-data) with ReLU6: the generic-activation multiplier.  The same lattice, with
#     offsets 1/2, 1/4, 1/8, 1/16 in front of its four ReLU6 layers and a BatchNorm weight of 2 in the stem so that the upper
#     clamp is active too: no pre-activation lies closer than the offset to 0 or to 6.
E2E_CLASSES = 10
GAP = 1e-3  # of the map's maximum
RELU_SCALE = 0.125
E2E = ("v1-tanh", "v1-relu", "v2-relu6")
E2E_SEED = {"v1-tanh": 1, "v1-relu": 2, "v2-relu6": 3}


def _filters_(w, gen, signed=True, nonzero=2):
    """every filter: ``nonzero`` entries of +-1 (``signed``) or +1, zeros elsewhere"""
    w.data.zero_()
    flat = w.data.view(w.shape[0], -1)
    for o in range(flat.shape[0]):
        at = torch.randperm(flat.shape[1], generator=gen)[:nonzero]
        flat[o, at] = (torch.randint(2, (nonzero,), generator=gen) * 2 - 1).to(flat.dtype) if signed else 1.0


def _lattice_bn_(bn, weight, offset):
    bn.eps = 2.0 ** -10  # (running_var + eps is exactly 1 in fp32 and in float64)
    bn.running_mean.zero_(), bn.running_var.fill_(1.0 - 2.0 ** -10)
    bn.weight.data.fill_(weight), bn.bias.data.fill_(offset)


def _cut_mobilenet_v1(act, gen):
    from laplace_amd.nets import MobileNetV1

    m = MobileNetV1(E2E_CLASSES, width=0.25, act=act)
    m.layers = m.layers[:6]
    m.fc = nn.Linear(m.layers[-1][3].out_channels, E2E_CLASSES)
    m = m.double().eval()
    bns = [mod for mod in m.modules() if isinstance(mod, nn.BatchNorm2d)]
    if act is nn.Tanh:
        for bn in bns:
            bn.running_mean.normal_(0, 0.3, generator=gen), bn.running_var.uniform_(0.5, 2.0, generator=gen)
        return m
    convs = [mod for mod in m.modules() if isinstance(mod, nn.Conv2d)]
    for i, (conv, bn) in enumerate(zip(convs, bns)):
        if i < 3:
            _filters_(conv.weight, gen), _lattice_bn_(bn, 1.0, RELU_SCALE * 2.0 ** -(i + 1))
        else:
            _filters_(conv.weight, gen, signed=False), _lattice_bn_(bn, 0.5, RELU_SCALE * 0.125)
    return m


class TwoInvertedResiduals(nn.Module):
    def __init__(self):
        from laplace_amd.nets import InvertedResidual

        super().__init__()
        self.stem = nn.Sequential(nn.Conv2d(3, 32, 3, 1, 1, bias=False), nn.BatchNorm2d(32), nn.ReLU6())
        self.layers = nn.Sequential(InvertedResidual(32, 32, 1, 1), InvertedResidual(32, 32, 1, 2))
        self.pool, self.fc = nn.AdaptiveAvgPool2d(1), nn.Linear(32, E2E_CLASSES)

    def forward(self, x):
        return self.fc(torch.flatten(self.pool(self.layers(self.stem(x))), 1))


def _two_inverted_residuals(gen):
    m = TwoInvertedResiduals().double().eval()
    step = 0.5
    for mod in m.modules():
        if isinstance(mod, nn.Conv2d):
            _filters_(mod.weight, gen)
    for seq in (m.stem, m.layers[0].block, m.layers[1].block):
        mods = list(seq)
        for i, mod in enumerate(mods):
            if isinstance(mod, nn.BatchNorm2d):
                acted = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU6)
                _lattice_bn_(mod, 2.0 if seq is m.stem else 1.0, step if acted else 0.0)
                step = step / 2 if acted else step
    return m


def e2e_fixture(name, freeze_depthwise=False):
    """``(float64 CPU model in eval mode with frozen BatchNorm, X [8, 3, 16, 16], y [8])``"""
    seed = E2E_SEED[name]
    gen = torch.Generator().manual_seed(seed)
    prev = torch.random.get_rng_state()
    torch.manual_seed(seed)  # (the layers this function does not fill keep their constructor's values, which draw from here)
    try:
        m = _two_inverted_residuals(gen) if name == "v2-relu6" else _cut_mobilenet_v1(nn.Tanh if name == "v1-tanh" else nn.ReLU, gen)
    finally:
        torch.random.set_rng_state(prev)
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.weight.requires_grad_(False), mod.bias.requires_grad_(False)
        if freeze_depthwise and isinstance(mod, nn.Conv2d) and mod.groups != 1:
            mod.weight.requires_grad_(False)
    if name == "v1-tanh":
        X = torch.randn(8, 3, 16, 16, generator=gen).double()
    else:
        X = torch.randint(-2, 3, (8, 3, 16, 16), generator=gen).double() * (RELU_SCALE if name == "v1-relu" else 1.0)
    y = torch.randint(E2E_CLASSES, (8,), generator=gen)
    return m, X, y


def e2e_taps(model):
    """the modules a sweep taps: Linear and convolution layers with a tracked weight"""
    return {n: m for n, m in model.named_modules() if isinstance(m, (nn.Conv2d, nn.Linear)) and m.weight.requires_grad}


def depthwise_names(model):
    return [n for n, m in model.named_modules() if isinstance(m, nn.Conv2d) and m.groups != 1]


def e2e_gaps(name):
    """smallest distance of a ReLU / ReLU6 pre-activation from a decision point (0, and 6 for ReLU6) in the float64 forward, as a
    fraction of its map's maximum, and the number of pre-activations that were looked at"""
    m, X, _ = e2e_fixture(name)
    gap, seen, hooks = [float("inf")], [0], []

    def pre(mod, inp):
        z = inp[0].detach()
        d = z.abs().min()
        if isinstance(mod, nn.ReLU6):
            d = torch.minimum(d, (z - 6.0).abs().min())
        gap[0] = min(gap[0], (d / z.abs().max()).item())
        seen[0] += z.numel()

    for mod in m.modules():
        if isinstance(mod, (nn.ReLU, nn.ReLU6)):
            hooks.append(mod.register_forward_pre_hook(pre))
    with torch.no_grad():
        m(X)
    for h in hooks:
        h.remove()
    return gap[0], seen[0]
