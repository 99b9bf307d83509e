"""Shapes, inputs and float64 references for the pooling kernels (csrc/lk_pool.hip) - shared by tests/test_pool_fixtures.py
(CPU: the table reaches every path, the references bite) and tests/test_gpu_pool.py (the device).

A case is a dict: ``kind`` "max" / "avg", window ``k``, stride ``s``, padding ``p`` (pairs), map ``H`` x ``W`` x ``C``, ``B`` images,
``S`` seeds, ``off`` (1: every buffer starts one element past an aligned address), ``inp`` (how the map is filled) and, for the
average, ``cip`` (count_include_pad) and ``div`` (divisor_override).  The shapes are the smallest at which a path can go wrong:
the last row and column in no window (7 x 7 under (2, 2, 0)), odd and even edges with padding and corner pixels in four windows
((3, 2, 1) on 5 x 5 and 6 x 6), nine windows per pixel ((3, 1, 1)), a rectangular window with different strides, a stride larger
than the window, one window over the whole map, channel counts that are and are not multiples of four, more than one workgroup,
and the seed loop's remainder below, at and above the seeds per pass - with and without the seeds split over grid.y.
"""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24  # unit roundoff of fp32
SEEDS_PER_PASS = 4  # POOL_SC of csrc/lk_pool.hip (tests/test_pool_fixtures.py reads it back through lk_pool_variant)


def _case(kind, k, s, p, hw, C=8, B=1, S=2, off=0, inp="rand", cip=True, div=None):
    pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)  # noqa: E731
    return dict(kind=kind, k=pair(k), s=pair(s), p=pair(p), H=pair(hw)[0], W=pair(hw)[1], C=C, B=B, S=S, off=off, inp=inp,
                cip=cip, div=div)


GEOMETRIES = [  # (window, stride, padding, map)
    (2, 2, 0, 4), (2, 2, 0, 7), (3, 2, 1, 5), (3, 2, 1, 6), (3, 1, 1, 4), ((2, 3), (2, 1), (1, 1), (5, 4)), (2, 3, 0, 8),
    (8, 8, 0, 8)]
_CS, _BS, _SS, _INPUTS = (4, 6, 8, 12, 68), (1, 3), (1, 2, 9, 17), ("rand", "relu", "neg", "const")

CASES = []
for _i, (_k, _s, _p, _hw) in enumerate(GEOMETRIES):
    # every geometry as a max pool with every input kind, and as an average; C, B, S and the alignment rotate through their values
    for _j, _inp in enumerate(_INPUTS):
        _n = _i * 4 + _j
        CASES.append(_case("max", _k, _s, _p, _hw, C=_CS[_n % 5], B=_BS[_n % 2], S=_SS[(_n // 2) % 4], off=int(_n % 7 == 3),
                           inp=_inp))
    CASES.append(_case("avg", _k, _s, _p, _hw, C=_CS[(_i + 2) % 5], B=_BS[_i % 2], S=_SS[_i % 4], off=int(_i % 3 == 1),
                       cip=_i % 2 == 0, div=5 if _i == 4 else None))
CASES += [
    # an unaligned base with a channel count that would otherwise take 16-byte loads, both kinds, selection and summing
    _case("max", 2, 2, 0, 4, C=8, B=3, S=9, off=1, inp="relu"), _case("max", 3, 2, 1, 6, C=12, B=1, S=17, off=1, inp="relu"),
    _case("avg", 3, 2, 1, 5, C=4, B=3, S=2, off=1, cip=False), _case("avg", 2, 2, 0, 4, C=8, B=1, S=9, off=1),
    _case("avg", 3, 1, 1, 4, C=68, B=3, S=17, cip=False), _case("avg", 8, 8, 0, 8, C=6, B=1, S=1, div=3),
    # enough lanes that the seeds stay in one slice: the seed loop ends one short of, at, and one past the seeds per pass
    _case("max", 2, 2, 0, 32, C=256, B=2, S=SEEDS_PER_PASS - 1, inp="relu"),
    _case("max", 3, 2, 1, 32, C=256, B=2, S=SEEDS_PER_PASS, inp="relu"),
    _case("avg", 2, 2, 0, 32, C=256, B=2, S=SEEDS_PER_PASS + 1),
    # half as many lanes: two slices of 5 and 4 seeds (split AND a remainder in both slices)
    _case("max", 3, 2, 1, 32, C=256, B=1, S=9, inp="relu"),
]


def case_id(c):
    g = f"k{c['k'][0]}x{c['k'][1]}s{c['s'][0]}x{c['s'][1]}p{c['p'][0]}x{c['p'][1]}"
    extra = "" if c["kind"] == "max" else f"-cip{int(c['cip'])}" + (f"-div{c['div']}" if c["div"] else "")
    return f"{c['kind']}-{g}-{c['H']}x{c['W']}x{c['C']}-B{c['B']}-S{c['S']}-{c['inp']}{extra}" + ("-unaligned" if c["off"] else "")


def out_hw(c):
    return ((c["H"] + 2 * c["p"][0] - c["k"][0]) // c["s"][0] + 1, (c["W"] + 2 * c["p"][1] - c["k"][1]) // c["s"][1] + 1)


def covering_windows(c):
    """most windows that share a pixel"""
    return math.ceil(c["k"][0] / c["s"][0]) * math.ceil(c["k"][1] / c["s"][1])


def selection(c):
    return c["k"][0] <= c["s"][0] and c["k"][1] <= c["s"][1]


def make_input(c, gen, device="cpu"):
    """fp32 NHWC map ``[B, H, W, C]``"""
    shape = (c["B"], c["H"], c["W"], c["C"])
    x = torch.randn(*shape, generator=gen, device=device)
    if c["inp"] == "relu":
        return torch.relu(x)  # (exact zero ties in most windows)
    if c["inp"] == "neg":
        return -x.abs() - 0.5  # (a padding tap that took part would win with 0)
    if c["inp"] == "const":
        return torch.full(shape, 1.25, device=device)
    return x


def codes_to_flat_index(c, arg):
    """window-local tap codes ``[B, OH, OW, C]`` -> what ``max_pool2d(return_indices=True)`` reports: ``h * W + w``, as
    ``[B, C, OH, OW]`` int64"""
    OH, OW = out_hw(c)
    code = arg.to(torch.int64).cpu()
    h0 = (torch.arange(OH) * c["s"][0] - c["p"][0]).view(1, OH, 1, 1)
    w0 = (torch.arange(OW) * c["s"][1] - c["p"][1]).view(1, 1, OW, 1)
    h, w = h0 + code // c["k"][1], w0 + code % c["k"][1]
    return (h * c["W"] + w).permute(0, 3, 1, 2)


def forward_reference(c, x):
    """float64 torch on the CPU from the same fp32 map -> dict: ``y`` ``[B, OH, OW, C]``; max: ``idx`` (flat indices, NCHW);
    average: ``bound`` = (taps + 1) u sum|taps| / div, which holds for any summation order"""
    x64 = x.detach().cpu().double().permute(0, 3, 1, 2)
    if c["kind"] == "max":
        y, idx = F.max_pool2d(x64, c["k"], c["s"], c["p"], return_indices=True)
        return {"y": y.permute(0, 2, 3, 1), "idx": idx}
    args = (c["k"], c["s"], c["p"], False, c["cip"], c["div"])
    return {"y": F.avg_pool2d(x64, *args).permute(0, 2, 3, 1),
            "bound": (c["k"][0] * c["k"][1] + 1) * U * F.avg_pool2d(x64.abs(), *args).permute(0, 2, 3, 1)}


def vjp_reference(c, g, idx=None):
    """``(dx, bound)`` in float64, ``[S, B, H, W, C]``, from the fp32 cotangent ``g`` ``[S, B, OH, OW, C]`` (and the flat indices of
    the forward reference).  ``bound`` is None on a max pool's selection shapes (the result is a copy: compared with
    ``torch.equal``), else m u sum|terms| (max) / (m + 1) u sum|terms| (average, one more for the division) with m the most
    windows that share a pixel - it holds for any order of the sum."""
    S, B, (OH, OW) = c["S"], c["B"], out_hw(c)
    g64 = g.detach().cpu().double().reshape(S * B, OH, OW, c["C"]).permute(0, 3, 1, 2)
    m = covering_windows(c)
    if c["kind"] == "max":
        flat = idx.unsqueeze(0).expand(S, *idx.shape).reshape(S * B, c["C"], -1)

        def scatter(t):
            out = torch.zeros(S * B, c["C"], c["H"] * c["W"], dtype=torch.float64)
            return out.scatter_add_(2, flat, t.reshape(S * B, c["C"], -1)).reshape(S * B, c["C"], c["H"], c["W"])

        dx, bound = scatter(g64), None if selection(c) else m * U * scatter(g64.abs())
    else:
        def back(t):
            x = torch.zeros(S * B, c["C"], c["H"], c["W"], dtype=torch.float64, requires_grad=True)
            y = F.avg_pool2d(x, c["k"], c["s"], c["p"], False, c["cip"], c["div"])
            return torch.autograd.grad(y, x, t)[0]

        dx, bound = back(g64), (m + 1) * U * back(g64.abs())
    shape = (S, B, c["H"], c["W"], c["C"])
    return dx.permute(0, 2, 3, 1).reshape(shape), None if bound is None else bound.permute(0, 2, 3, 1).reshape(shape)


def kernel_kind(K, c):
    return K.POOL_MAX if c["kind"] == "max" else K.POOL_AVG


# ---- end-to-end fixtures: a small ImageNet-stem ResNet and a small VGG-shaped stack ------------------------------------------------
# A max pool decides like a ReLU mask: an fp32 forward may pick another element of a near-tied window, or put a pre-activation
# on the other side of zero, than the float64 reference does, and the cotangents of the two passes then differ by O(1) for a
# reason that is no fault of the code under test.  With thousands of windows and pre-activations per minibatch no choice of seed
# keeps generic real-valued maps clear of near ties, so the maps that DECIDE are put on a coarse dyadic lattice: integer inputs,
# convolution weights with two entries of +-1 per filter, BatchNorm with zero mean and running_var + eps = 1, and an offset of
# half the lattice step in front of every ReLU (no pre-activation is zero).  Values of one window are then equal - an exact tie,
# which fp32 reproduces because sums of small dyadic numbers are exact in it, and which the tie rule decides - or at least a
# lattice step apart.  tests/test_pool_fixtures.py asserts both gaps on the float64 forward of every fixture.
# The ReLU fixtures carry a common factor of 1/8 on the input and on every offset: a ReLU network is positively homogeneous, so no
# decision and no relative gap changes, and the activations (sums of up to four lattice values per layer) stay of order one -
# the Kronecker factors' eigenvalues then stay in the range where an fp32 eigensolver (which resolves them to 1e-7 of the
# largest) sees the prior precision of the predictive test, as with the other end-to-end fixtures of this suite.
E2E_CLASSES = 5
GAP = 1e-3  # of the map's maximum
RELU_SCALE = 0.125


def _ternary_(w, gen, nonzero=2):
    """every filter: ``nonzero`` entries of +-1, zeros elsewhere"""
    w.data.zero_()
    flat = w.data.view(w.shape[0], -1)
    for o in range(flat.shape[0]):
        at = torch.randperm(flat.shape[1], generator=gen)[:nonzero]
        flat[o, at] = (torch.randint(2, (nonzero,), generator=gen) * 2 - 1).to(flat.dtype)


def _lattice_bn_(bn, weight, offset):
    bn.eps = 2.0 ** -10  # (running_var + eps is exactly 1 in fp32 and in float64)
    bn.running_mean.zero_(), bn.running_var.fill_(1.0 - 2.0 ** -10)
    bn.weight.data.fill_(weight), bn.bias.data.fill_(offset)
    bn.weight.requires_grad_(False), bn.bias.requires_grad_(False)


class StemResNet(torch.nn.Module):
    """``ResNet18(stem="imagenet")`` with 32 channels and one block: 7 x 7 stride-2 convolution, BatchNorm, activation,
    ``MaxPool2d(3, 2, 1)``, a ``BasicBlock`` (whose first 3 x 3 convolution reads the pooled map), global average, Linear"""

    def __init__(self, act):
        from laplace_amd.nets import BasicBlock

        super().__init__()
        nn = torch.nn
        self.act = act
        self.conv1, self.bn1, self.maxpool = nn.Conv2d(3, 32, 7, 2, 3, bias=False), nn.BatchNorm2d(32), nn.MaxPool2d(3, 2, 1)
        self.layers = nn.Sequential(BasicBlock(32, 32, 1, act))
        self.pool, self.fc = nn.AdaptiveAvgPool2d(1), nn.Linear(32, E2E_CLASSES)

    def forward(self, x):
        x = self.maxpool(self.act(self.bn1(self.conv1(x))))
        return self.fc(torch.flatten(self.pool(self.layers(x)), 1))


def _stem_resnet(act, gen):
    m = StemResNet(act).double().eval()
    tanh = act is torch.tanh
    _ternary_(m.conv1.weight, gen)
    # (tanh: a step of 1/2 keeps neighbouring lattice values apart behind the saturating activation; the block behind a tanh
    # reads generic reals and decides nothing)
    _lattice_bn_(m.bn1, 0.5 if tanh else 1.0, 0.25 if tanh else 0.5 * RELU_SCALE)
    blk = m.layers[0]
    if tanh:
        for bn in (blk.bn1, blk.bn2):
            bn.running_mean.normal_(0, 0.3, generator=gen), bn.running_var.uniform_(0.5, 2.0, generator=gen)
            bn.weight.requires_grad_(False), bn.bias.requires_grad_(False)
    else:
        _ternary_(blk.conv1.weight, gen), _ternary_(blk.conv2.weight, gen)
        _lattice_bn_(blk.bn1, 1.0, 0.25 * RELU_SCALE), _lattice_bn_(blk.bn2, 1.0, 0.125 * RELU_SCALE)
    return m


class PoolStack(torch.nn.Module):
    """A VGG-shaped stack: 3 x 3 convolutions (with bias), activation, ``MaxPool2d(2)`` where ``cfg`` says ``"M"``, then a flatten
    head (pool - flatten - Linear).  ``act`` is the activation module's class."""

    def __init__(self, num_classes, cfg, in_hw, act=torch.nn.ReLU):
        super().__init__()
        nn = torch.nn
        layers, cin, hw = [], 3, in_hw
        for v in cfg:
            if v == "M":
                layers.append(nn.MaxPool2d(2))
                hw //= 2
            else:
                layers += [nn.Conv2d(cin, v, 3, 1, 1), act()]
                cin = v
        self.features = nn.Sequential(*layers)
        self.flatten = nn.Flatten()
        self.fc = nn.Linear(cin * hw * hw, num_classes)

    def forward(self, x):
        return self.fc(self.flatten(self.features(x)))


def _small_vgg(act_cls, hw, gen):
    m = PoolStack(E2E_CLASSES, cfg=(32, "M", 32, "M"), in_hw=hw, act=act_cls).double().eval()
    convs = [mod for mod in m.features if isinstance(mod, torch.nn.Conv2d)]
    _ternary_(convs[0].weight, gen)
    if act_cls is torch.nn.Tanh:
        # (the second stage reads tanh values: with ONE entry of +-1 per filter its map still takes few distinct values, the
        # tanh of the lattice up to sign, which lie far apart)
        convs[0].weight.data.mul_(0.5), convs[0].bias.data.fill_(0.25)
        _ternary_(convs[1].weight, gen, nonzero=1), convs[1].bias.data.zero_()
    else:
        convs[0].bias.data.fill_(0.5 * RELU_SCALE)
        _ternary_(convs[1].weight, gen), convs[1].bias.data.fill_(0.25 * RELU_SCALE)
    return m


#: name -> (network, activation, input size, batch, seed)
E2E = {
    "resnet-relu-16": ("resnet", "relu", 16, 3, 1), "resnet-relu-32": ("resnet", "relu", 32, 2, 2),
    "resnet-tanh-16": ("resnet", "tanh", 16, 3, 3), "resnet-tanh-32": ("resnet", "tanh", 32, 2, 4),
    "vgg-relu-16": ("vgg", "relu", 16, 3, 5), "vgg-relu-32": ("vgg", "relu", 32, 2, 6),
    "vgg-tanh-16": ("vgg", "tanh", 16, 3, 7), "vgg-tanh-32": ("vgg", "tanh", 32, 2, 8),
}

#: the fixtures in which every map that DECIDES holds dyadic numbers, whose sums are exact in fp32 in any order: exact ties stay
#: exact under every convolution algorithm, a library's transform-domain ones included.  The second pool of the tanh VGG reads a
#: convolution of tanh values: its ties survive arithmetic that treats equal inputs equally (the NHWC kernels: one product per
#: filter and a sum of zeros), not a library convolution that mixes neighbouring pixels before it multiplies.
E2E_EXACT = tuple(n for n in sorted(E2E) if not n.startswith("vgg-tanh"))


def e2e_fixture(name, act=None):
    """``(float64 CPU model, X, y)``; ``act``: the function a ResNet applies instead of its activation (the gap check's probe)"""
    net, kind, hw, B, seed = E2E[name]
    gen = torch.Generator().manual_seed(seed)
    prev = torch.random.get_rng_state()
    torch.manual_seed(seed)  # (the layers this function does not fill keep their constructor's values, which draw from here)
    try:
        if net == "resnet":
            fn = torch.relu if kind == "relu" else torch.tanh
            m = _stem_resnet(fn, gen)
            if act is not None:
                m.act = m.layers[0].act = act
        else:
            m = _small_vgg(torch.nn.ReLU if kind == "relu" else torch.nn.Tanh, hw, gen)
    finally:
        torch.random.set_rng_state(prev)
    X = torch.randint(-2, 3, (B, 3, hw, hw), generator=gen).double() * (RELU_SCALE if kind == "relu" else 1.0)
    y = torch.randint(E2E_CLASSES, (B,), generator=gen)
    return m, X, y


def e2e_taps(model):
    return {n: m for n, m in model.named_modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear))}


def window_gap(z, pool):
    """smallest distance between the two largest DISTINCT values of a window, over all windows of ``pool`` on the map ``z``
    ``[B, C, H, W]``, as a fraction of max|z| (inf: no window holds two distinct values)"""
    k, s, p = (pool.kernel_size, pool.stride, pool.padding)
    pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)  # noqa: E731
    (kh, kw), (sh, sw), (ph, pw) = pair(k), pair(s), pair(p)
    zp = F.pad(z, (pw, pw, ph, ph), value=float("-inf"))
    win = zp.unfold(2, kh, sh).unfold(3, kw, sw).reshape(*z.shape[:2], -1, kh * kw)  # [B, C, windows, taps]
    top = win.max(-1, keepdim=True).values
    second = torch.where(win < top, win, torch.full_like(win, float("-inf"))).max(-1, keepdim=True).values
    gap = (top - second)[torch.isfinite(second)]
    return (gap.min() / z.abs().max()).item() if gap.numel() else float("inf")


def e2e_gaps(name):
    """``(smallest window gap, smallest |ReLU pre-activation|)`` of the float64 forward, each as a fraction of its map's maximum,
    and the number of pooling windows and pre-activations that were looked at"""
    gaps, seen = {"window": float("inf"), "relu": float("inf")}, {"window": 0, "relu": 0}

    def note_relu(z):
        gaps["relu"] = min(gaps["relu"], (z.detach().abs().min() / z.detach().abs().max()).item())
        seen["relu"] += z.numel()

    def noting_relu(z):
        note_relu(z)
        return torch.relu(z)

    m, X, _ = e2e_fixture(name, noting_relu if E2E[name][:2] == ("resnet", "relu") else None)
    hooks = []
    for mod in m.modules():
        if isinstance(mod, torch.nn.MaxPool2d):
            def pre(mod_, inp):
                gaps["window"] = min(gaps["window"], window_gap(inp[0].detach(), mod_))
                seen["window"] += inp[0].numel() // (mod_.stride if isinstance(mod_.stride, int) else mod_.stride[0]) ** 2

            hooks.append(mod.register_forward_pre_hook(pre))
        elif isinstance(mod, torch.nn.ReLU):
            hooks.append(mod.register_forward_pre_hook(lambda mod_, inp: note_relu(inp[0])))
    with torch.no_grad():
        m(X)
    for h in hooks:
        h.remove()
    return gaps, seen
