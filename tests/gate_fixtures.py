"""Shapes, inputs, references and acceptance criteria for the squeeze-and-excitation gate kernels (csrc/lk_gate.hip) and the small
SE networks of the end-to-end tests - shared by tests/test_gate_fixtures.py (CPU: the table reaches every path, the criteria bite),
tests/emulated_gate_kernels.py (the kernel emulation states its rule through `torch_math`), tests/test_sweep_gate.py and
tests/test_gpu_gate.py (the device).

A kernel case is a dict: ``kind`` (``"reduce"``: ``ds[s, b, c] = sum_p g[s, b, p, c] x[b, p, c]``; ``"vjp"``: ``dx[s, b, p, c] =
g[s, b, p, c] gate[b, c] + r[s, b, c]``), seeds ``S``, samples ``B``, positions ``P``, channels ``C``, ``split`` (``g`` is a
one-scale split tensor read as it lies), ``off`` (1: every buffer starts one element past an aligned address, which forces the 4-byte
path), ``r`` and ``amax`` (the VJP's optional operands) and ``wide`` (an element offset passes 2^31: checked by shape only, never
run).  The shapes are the smallest at which a path can go wrong.  A workgroup is ``lanes`` lanes across the channel vectors (the
power of two at or above C / 4 - C on the 4-byte path -, at most 64) times ``256 / lanes`` position groups; x of the reduce stays in
registers up to 16 positions per thread:
P in {1, 2, 3, 16, 49, 64} and 1024, the resident limit and the first P past it on both paths (C = 32: 8 lanes x 32 groups, 512
positions with 16-byte loads; 32 lanes x 8 groups, 128 with 4-byte ones), C in {1, 3, 4, 8, 32, 36, 64, 260} (36: nine vectors on 16
lanes; 260: 65 vectors, a second channel tile with one live lane), B in {0, 1, 2, 5}, S in {1, 3, 9} (few samples: the seeds go over
grid.y), a unit count one past a full stride of the grid (2048 workgroups), positions that do not fill the last position group or
the last chunk of the VJP (8 positions per thread).
"""
import torch
from torch import nn

from tests.mul_fixtures import E2E_CLASSES, _seeded, full_mantissa, rel, run_curvature_checks, se_fixture, taps  # noqa: F401

MAX_BLOCKS = 2048  # STREAM_MAX_BLOCKS of csrc/lk_stream.h
RESIDENT_POSITIONS = 16  # GATE_NV: positions of x a thread keeps in registers
VJP_POSITIONS = 8  # GATE_PP: positions a thread of the VJP walks per unit


def _case(kind, S, B, P, C, split=False, off=0, r=True, amax=True, wide=False):
    return dict(kind=kind, S=S, B=B, P=P, C=C, split=bool(split), off=off, r=bool(r) and kind == "vjp",
                amax=bool(amax) and kind == "vjp", wide=wide)


def _both(S, B, P, C, **kw):
    """the reduce and the VJP of a shape, with g as fp32 and as a split tensor"""
    return [_case(k, S, B, P, C, split=sp, **kw) for k in ("reduce", "vjp") for sp in (False, True)]


CASES = [
    # every P of the list at C = 32 (eight lanes of four channels, 32 position groups)
    *[c for P in (1, 2, 3, 16, 49, 64) for c in _both(3, 2, P, 32)],
    # every C of the list at P = 16 (1, 3: one and four scalar lanes; 36: nine vectors on 16 lanes; 260: two channel tiles)
    *[c for C in (1, 3, 4, 8, 36, 64, 260) for c in _both(3, 2, 16, C)],
    # a base one element past alignment: the 4-byte path on multiples of four
    *[c for (P, C) in ((16, 32), (49, 64), (3, 260)) for c in _both(3, 2, P, C, off=1)],
    # the resident limit of x and the first P past it, on both paths; P = 1024 (re-read per seed)
    *[_case("reduce", 3, 2, P, 32, split=sp) for P in (512, 513) for sp in (False, True)],
    *[_case("reduce", 3, 2, P, 32, split=sp, off=1) for P in (128, 129) for sp in (False, True)],
    *_both(9, 1, 1024, 32), _case("reduce", 3, 1, 1024, 3),
    # B in {1, 2, 5} and S in {1, 3, 9}; few samples: the seeds go over grid.y
    *_both(1, 1, 49, 8), *_both(9, 5, 16, 36), *_both(1, 5, 3, 4), *_both(9, 1, 64, 64, off=1),
    # samples enough to fill the chip: all seeds in one grid.y slice
    _case("reduce", 3, 513, 2, 4), _case("reduce", 3, 513, 3, 3, split=True),
    # the VJP's optional operands: r and the amax word, present and null
    *[_case("vjp", 3, 2, P, C, split=sp, r=r, amax=a) for (P, C) in ((49, 32), (16, 3)) for sp in (False, True)
      for (r, a) in ((False, True), (True, False), (False, False))],
    # positions one past a full chunk of the VJP (8 lanes x 32 groups x 8 positions = 256 per chunk at C = 32; 4 x 8 = 32 at C = 260)
    _case("vjp", 3, 2, 257, 32), _case("vjp", 1, 1, 33, 260, split=True),
    # one unit past a full stride of the grid (2048 workgroups), on both paths
    *[_case(k, 1, MAX_BLOCKS + 1, 1, C, split=sp) for k in ("reduce", "vjp") for (C, sp) in ((1, False), (4, True))],
    _case("reduce", 1, 1025, 2, 260), _case("vjp", 1, 1025, 2, 260, split=True),  # (1025 samples x 2 channel tiles = 2050)
    # no samples: LK_OK before any device call
    *_both(3, 0, 16, 32),
    # an element offset passes 2^31 (by shape only)
    _case("reduce", 9, 128, 1 << 12, 512, wide=True), _case("vjp", 9, 128, 1 << 12, 512, split=True, wide=True),
    _case("vjp", 3, 1 << 20, 1, 1023, wide=True),
]


def case_id(c):
    return (f"{c['kind']}-S{c['S']}-B{c['B']}-P{c['P']}-C{c['C']}-{'split' if c['split'] else 'f32'}"
            + ("" if c["kind"] == "reduce" else f"-r{int(c['r'])}-amax{int(c['amax'])}") + ("-unaligned" if c["off"] else "")
            + ("-wide" if c["wide"] else ""))


def split_g(g):
    """``g`` as a one-scale split tensor by the project's own split (the emulation of lk_split_f16x2: the scale from max|g|)"""
    from tests.emulated_kernels import EmulatedKernels

    return EmulatedKernels._split(g, EmulatedKernels._sexp_for(g.abs().max() if g.numel() else 0.0))


def make_inputs(c, gen):
    """``dict(g, x | gate, r)`` of a case on the CPU: ``g`` ``[S, B, P, C]`` fp32 - for a split case the fp32 reconstruction of the
    :class:`SplitTensor` ``g_split`` of full-mantissa values -, ``x`` ``[B, P, C]`` (reduce) or ``gate`` ``[B, C]`` and ``r``
    ``[S, B, C]`` or ``None`` (VJP)"""
    S, B, P, C = c["S"], c["B"], c["P"], c["C"]
    g = full_mantissa((S, B, P, C), gen)
    out = {}
    if c["split"]:
        out["g_split"] = split_g(g.reshape(S * B, P, 1, C))
        g = out["g_split"].float().reshape(S, B, P, C)
    out["g"] = g
    if c["kind"] == "reduce":
        out["x"] = full_mantissa((B, P, C), gen)
    else:
        out["gate"] = full_mantissa((B, C), gen)
        out["r"] = full_mantissa((S, B, C), gen) if c["r"] else None
    return out


def reference(c, inp):
    """fp64: the exact result ``out`` and the magnitude ``mag`` the bound is relative to (reduce: ``sum_p |g x|``; VJP:
    ``|g gate| + |r|``)"""
    g = inp["g"].double()
    if c["kind"] == "reduce":
        prod = g * inp["x"].double()
        return dict(out=prod.sum(2), mag=prod.abs().sum(2))
    prod = g * inp["gate"].double()[None, :, None, :]
    if inp["r"] is None:
        return dict(out=prod, mag=prod.abs())
    r = inp["r"].double()[:, :, None, :]
    return dict(out=prod + r, mag=prod.abs() + r.abs())


MUTANTS = ("wrong-sample", "dropped-positions", "dropped-channels", "fp16-sum", "wrong-seed-r", "undivided-r")


def torch_math(c, inp, mutant=None):
    """the rule of lk_gate_reduce_nhwc_f32 / lk_gate_vjp_nhwc_f32 in torch fp32: ``ds`` ``[S, B, C]`` or ``dx`` ``[S, B, P, C]``.
    MUTANTS: ``"wrong-sample"`` takes ``x`` / ``gate`` of seed ``s`` from ``s`` samples on; ``"dropped-positions"`` leaves the last
    ``P % 4`` positions out (missing from the sum, NaN in ``dx``); ``"dropped-channels"`` leaves the last ``C % 4`` channels NaN;
    ``"fp16-sum"`` accumulates the sum over the positions in fp16; ``"wrong-seed-r"`` adds ``r`` of the next seed;
    ``"undivided-r"`` adds ``r`` once per position, i.e. ``P r``."""
    S, B, P, C = c["S"], c["B"], c["P"], c["C"]
    g = inp["g"]
    per_sample = inp["x"] if c["kind"] == "reduce" else inp["gate"]
    ps = per_sample.unsqueeze(0).expand(S, *per_sample.shape)
    if mutant == "wrong-sample" and B:
        ps = torch.stack([per_sample.roll(-s, 0) for s in range(S)])
    if c["kind"] == "reduce":
        prod = g * ps
        if mutant == "dropped-positions":
            prod = prod[:, :, :P - P % 4]
        out = prod.half().sum(2, dtype=torch.float16).float() if mutant == "fp16-sum" else prod.sum(2)
    else:
        out = g * ps[:, :, None, :]
        if inp["r"] is not None:
            r = inp["r"].roll(-1, 0) if mutant == "wrong-seed-r" else inp["r"]
            out = out + (r * P if mutant == "undivided-r" else r)[:, :, None, :]
        if mutant == "dropped-positions" and P % 4:
            out[:, :, P - P % 4:] = float("nan")
    if mutant == "dropped-channels" and C % 4:
        out[..., C - C % 4:] = float("nan")
    return out


def violations(c, out, ref, inp):
    """what the output of a case breaks of the device test's criteria (an empty list: none).  VJP without ``r``: the fp32 product -
    the exact fp64 product rounded once - bit for bit; with ``r``: within ``2^-23 (|g gate| + |r|)`` of the exact value (a fused
    or a separate multiply-add: two roundings of at most half an ulp of values no larger than that magnitude).  Reduce: within
    ``(P + 1) 2^-24 sum_p |g x|`` of the exact sum (a sum of P products in any order, products fused into it or not; P <= 4096)."""
    bad = []
    out = out.detach().cpu().reshape(ref["out"].shape)
    if c["kind"] == "vjp" and inp["r"] is None:
        if not torch.equal(out, ref["out"].float()):
            bad.append("dx is not the fp32 product g * gate")
        return bad
    assert c["P"] <= 4096
    factor = 2.0 ** -23 if c["kind"] == "vjp" else (c["P"] + 1) * 2.0 ** -24
    err = (out.double() - ref["out"]).abs()
    if not bool((err <= factor * ref["mag"]).all()):  # (a NaN fails)
        worst = float((err / ref["mag"]).nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0
        bad.append(f"{'dx' if c['kind'] == 'vjp' else 'ds'} off by {worst:.3e} of the magnitude (bound {factor:.3e})")
    return bad


def worst_ratio(c, out, ref, inp):
    """largest error / bound of a case (0 where the criterion is bit equality or there is no element)"""
    if c["kind"] == "vjp" and inp["r"] is None or not ref["out"].numel():
        return 0.0
    factor = 2.0 ** -23 if c["kind"] == "vjp" else (c["P"] + 1) * 2.0 ** -24
    err = (out.detach().cpu().reshape(ref["out"].shape).double() - ref["out"]).abs()
    return float((err / (factor * ref["mag"])).max())


# ---- end-to-end fixtures ---------------------------------------------------------------------------------------------------------
# `se_net()`: the SEResNetSmall of tests/mul_fixtures.se_fixture at widths 32 / 64 (what the split sweep's convolutions take), one
# block per stage, 8 x 8 inputs, B = 2, tanh: gate convolutions 32 -> 8 -> 32 on 8 x 8 maps and 64 -> 16 -> 64 on 4 x 4 maps.
# `linear_gate_net()`: a gate spelled with Linear layers (flatten - Linear - Tanh - Linear - Sigmoid - view(-1, C, 1, 1)) on a
# ReLU-free stack of convolutions.  Smooth activations only: nothing is decided by a sign.
def se_net():
    return se_fixture(widths=(32, 64), depth=1, B=2, hw=8)


class LinearGateNet(nn.Module):
    """conv - BN - tanh, a Linear-spelled squeeze-and-excitation gate (``gate_first``: written as the left operand), conv - tanh,
    global average - flatten - Linear"""

    def __init__(self, classes=E2E_CLASSES, c=32, reduction=4, gate_first=False):
        super().__init__()
        self.c, self.gate_first = c, gate_first
        self.conv1, self.bn1, self.act1 = nn.Conv2d(3, c, 3, 1, 1, bias=False), nn.BatchNorm2d(c), nn.Tanh()
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc1, self.act, self.fc2, self.gate = nn.Linear(c, c // reduction), nn.Tanh(), nn.Linear(c // reduction, c), nn.Sigmoid()
        self.conv2, self.act2 = nn.Conv2d(c, c, 3, 1, 1), nn.Tanh()
        self.head_pool, self.fc = nn.AdaptiveAvgPool2d(1), nn.Linear(c, classes)
        for p in (self.bn1.weight, self.bn1.bias):
            p.requires_grad_(False)

    def forward(self, x):
        h = self.act1(self.bn1(self.conv1(x)))
        s = self.gate(self.fc2(self.act(self.fc1(torch.flatten(self.pool(h), 1))))).view(-1, self.c, 1, 1)
        h = s * h if self.gate_first else h * s
        return self.fc(torch.flatten(self.head_pool(self.act2(self.conv2(h))), 1))


def linear_gate_net(gate_first=False, B=2, hw=8, seed=43):
    """``(float64 CPU model, X, y)``: a :class:`LinearGateNet`, deterministic"""
    m = _seeded(seed, lambda: LinearGateNet(gate_first=gate_first))
    gen = torch.Generator().manual_seed(seed)
    return m, torch.randn(B, 3, hw, hw, generator=gen).double(), torch.randint(E2E_CLASSES, (B,), generator=gen)
