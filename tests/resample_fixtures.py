"""TEST INFRASTRUCTURE for the static separable resampling rule (nn.Upsample / F.interpolate, F.pad and the padding modules): the
case table and the stated reference of csrc/lk_resample.hip, and the end-to-end fixtures - a tiny FPNSmall in both modes and a tiny
TCNSmall with its unit-height 2-D twin, on which the fp64 oracle's KFAC runs.

A case is an operation of torch (``op`` "interpolate" / "pad" with its keyword arguments) on planes of extent ``H x W`` (``k = 1``:
a 1-D operation, ``H = 1``), ``P`` planes.  The kernel's operands are the cotangent ``g [P][OH][OW]`` and the TRANSPOSED tap lists of
the two axes; the reference is the fp64 sum with the SAME fp32 tables, and the bound is element-wise
``(n + 3) 2^-24 sum |wh ww g|`` with ``n`` the element's tap count: two roundings from the products, ``n - 1`` from the additions,
the rest slack for second order - it holds for any summation order, either factoring and fused multiply-adds.
"""
import torch
import torch.nn.functional as F
from torch import nn

from laplace_amd import sweep as sw

CAP = 16  # LK_RESAMPLE_MAX_TAPS
GAP = 1e-3  # of the map's maximum (that of tests/pool_fixtures.py): how far a ReLU pre-activation stays from zero


def _interp(mode, H, W, P=6, k=2, off=0, huge=False, **kw):
    vals = dict(size=None, scale_factor=None, mode=mode, align_corners=None, recompute_scale_factor=None, antialias=False)
    vals.update(kw)
    return dict(op="interpolate", kw=vals, H=H, W=W, P=P, k=k, off=off, huge=huge)


def _pad(pad, mode, H, W, P=6, k=2, off=0, value=None, huge=False):
    return dict(op="pad", kw=dict(pad=tuple(pad), mode=mode, value=value), H=H, W=W, P=P, k=k, off=off, huge=huge)


CASES = [
    _interp("nearest", 3, 5, scale_factor=2),  # the scalar path (W = 5)
    _interp("bilinear", 4, 8, scale_factor=2, align_corners=False),  # the vector path (W = 8, aligned)
    _interp("bilinear", 4, 8, scale_factor=2, align_corners=False, off=1),  # the same from a pointer offset by one float
    _interp("bilinear", 4, 8, scale_factor=2, align_corners=True),
    _interp("bilinear", 5, 7, size=(8, 9), align_corners=False),  # a non-integer ratio, spelled with size
    _interp("bilinear", 5, 8, scale_factor=1.5, align_corners=False),  # ... and with a non-integer scale_factor
    _interp("bicubic", 6, 8, scale_factor=2, align_corners=False),  # up to 8 taps with the clamped edges: the table walk
    _interp("bicubic", 5, 5, size=(7, 9), align_corners=True),
    _interp("area", 8, 8, size=(3, 5)),  # down-sampling
    _interp("bilinear", 9, 12, size=(4, 5), align_corners=False, antialias=True),
    _interp("nearest-exact", 3, 4, size=(7, 9)),
    _interp("linear", 1, 8, k=1, scale_factor=2, align_corners=False),  # 1-D: H = 1
    _interp("nearest", 1, 7, k=1, size=(12,)),
    _interp("nearest", 4, 4, P=1, scale_factor=2),  # one plane
    _interp("nearest", 2, 2, P=9 * 2 * 3, scale_factor=2),  # the seeds split over grid.y
    _interp("nearest", 32, 32, P=576, scale_factor=2),  # many planes of a whole map
    _pad((1, 1, 1, 1), "constant", 724, 725, P=1),  # one lane past a full stride of grid.x (2048 workgroups of 256 threads)
    _pad((2, 1, 1, 2), "reflect", 4, 5),
    _pad((2, 3, 1, 0), "replicate", 3, 8),  # the edge input is read by pad + 1 outputs
    _pad((1, 2, 2, 1), "circular", 4, 4),
    _pad((-1, 2, 1, -1), "constant", 5, 6, value=0.5),  # a value and a cropping pad: the cropped border is untapped
    _pad((-2, -1, 0, 0), "constant", 3, 8),
    _pad((4, 0), "constant", 1, 9, k=1),  # the causal pad of a temporal convolution network
    _pad((3, 0), "reflect", 1, 8, k=1),
    _pad((0, 2), "replicate", 1, 5, k=1, off=3),
]
# the tap-count sweep: x t nearest gives every input t taps per axis (1, 2, cap - 1, cap)
CASES += [_interp("nearest", 1, 5, k=1, scale_factor=t) for t in (1, 2, CAP - 1, CAP)]
CASES += [_interp("nearest", 2, 4, scale_factor=CAP, P=2)]  # cap x cap taps of one element
# past 2^31 lanes of one plane, on the scalar and on the vector path: through lk_resample_variant only, never run
CASES += [_pad((0, 0, 0, 0), "constant", 1 << 16, (1 << 15) + 1, P=1, huge=True),
          _pad((0, 0, 0, 0), "constant", 1 << 16, 1 << 17, P=1, huge=True)]
OVER_CAP = _interp("nearest", 1, 3, k=1, scale_factor=CAP + 1)  # one tap more than the kernel serves: the matmul form


def case_id(c):
    kw = c["kw"]
    if c["op"] == "pad":
        what = f"pad{'x'.join(str(p) for p in kw['pad'])}-{kw['mode']}" + ("-value" if kw["value"] else "")
    else:
        what = kw["mode"] + (f"-size{'x'.join(str(s) for s in kw['size'])}" if kw["size"] is not None else f"-x{kw['scale_factor']}")
        what += {None: "", True: "-ac1", False: "-ac0"}[kw["align_corners"]] + ("-aa" if kw["antialias"] else "")
    return f"{what}-{c['H']}x{c['W']}-P{c['P']}" + (f"-off{c['off']}" if c["off"] else "") + ("-huge" if c["huge"] else "")


def runnable(cases=None):
    return [c for c in (CASES if cases is None else cases) if not c["huge"]]


def apply(c, x):
    """torch's own operation of a case on ``x`` ``[N, C, H, W]`` (``k = 1``: ``[N, C, W]``)"""
    fn = F.interpolate if c["op"] == "interpolate" else F.pad
    return fn(x, **c["kw"])


def out_extent(c):
    if c["huge"]:
        return c["H"], c["W"]
    shape = (1, 1, c["W"]) if c["k"] == 1 else (1, 1, c["H"], c["W"])
    y = apply(c, torch.zeros(shape))
    return (1, y.shape[-1]) if c["k"] == 1 else tuple(y.shape[-2:])


def tables(c, dtype=torch.float32, **override):
    """``sweep.resample_tables`` of a case (``override``: keyword arguments replaced - the align_corners mutant)"""
    kw = {**c["kw"], **override}
    return sw.resample_tables(c["op"], kw, (c["H"], c["W"]), out_extent(c), c["k"], torch.zeros(1, dtype=dtype))


def dense_operator(c, dtype=torch.float64):
    """``[OH OW, H W]``: the case's operation on the full ``H W`` basis, ``op(basis) - op(zeros)``"""
    H, W = c["H"], c["W"]
    eye = torch.eye(H * W, dtype=dtype).reshape(H * W, 1, *((W,) if c["k"] == 1 else (H, W)))
    y = apply(c, eye) - apply(c, torch.zeros_like(eye))
    return y.reshape(H * W, -1).t()


def dense_transposed(axis, OL):
    """``[L, OL]`` fp64 from the transposed tap lists ``(ptr, idx, w)`` of an axis: exactly the fp32 weights"""
    ptr, idx, w = (t.cpu() for t in axis[:3])
    L = ptr.numel() - 1
    T = torch.zeros(L, OL, dtype=torch.float64)
    rows = torch.repeat_interleave(torch.arange(L), (ptr[1:] - ptr[:-1]).long())
    n = rows.numel()
    T[rows, idx[:n].long()] = w[:n].double()
    return T


def tap_counts(axis):
    ptr = axis[0].cpu().long()
    return ptr[1:] - ptr[:-1]


def vjp_reference(g, axis_h, axis_w, mutant=None, into=None):
    """``(dx [P, H, W] fp64, bound, untapped mask)`` for ``g [P, OH, OW]``: the fp64 sum with the fp32 tables, the element-wise
    bound ``(n + 3) 2^-24 sum |wh ww g|`` and the inputs no output reads (they must receive ``+0.0``).  Mutants: ``"drop-edge"``
    (the first tap of the first input and the last tap of the last input of each axis - the clamped border - is dropped where the
    list holds more than one), ``"no-zero"`` (an untapped input keeps what ``into`` held: the zero write skipped)."""
    OH, OW = g.shape[-2:]
    Th, Tw = dense_transposed(axis_h, OH), dense_transposed(axis_w, OW)
    if mutant == "drop-edge":
        for T in (Th, Tw):
            for row, pick in ((0, 0), (T.shape[0] - 1, -1)):
                nz = T[row].nonzero().flatten()
                if nz.numel() > 1:
                    T[row, nz[pick]] = 0.0
    gd = g.double().cpu()
    dx = Th @ gd @ Tw.t()
    n = tap_counts(axis_h).reshape(-1, 1) * tap_counts(axis_w).reshape(1, -1)
    bound = (n + 3).double() * 2.0 ** -24 * (Th.abs() @ gd.abs() @ Tw.abs().t())
    untapped = (n == 0).expand_as(dx[0]).clone()
    if mutant == "no-zero":
        dx = torch.where(untapped, into.double().cpu(), dx)
    return dx, bound, untapped


def make_g(c, gen, OH=None, OW=None):
    OH, OW = out_extent(c) if OH is None else (OH, OW)
    return torch.rand(c["P"], OH, OW, generator=gen) * 2 - 1


# ---- end-to-end fixtures ---------------------------------------------------------------------------------------------------------
E2E_CLASSES = 3


def _relu_gap(model, X):
    """the smallest |pre-activation| of any ReLU over its map's max |.|"""
    gaps, hooks = [], []
    for mod in model.modules():
        if isinstance(mod, nn.ReLU):
            hooks.append(mod.register_forward_hook(lambda m, i, o: gaps.append((i[0].abs().min() / i[0].abs().max()).item())))
    with torch.no_grad():
        model(X)
    for h in hooks:
        h.remove()
    return min(gaps) if gaps else float("inf")


def relu_gap(fixture):
    return _relu_gap(fixture[0], fixture[2])


def _calibrated(build, make_x, seed):
    """the first seed (deterministic) whose fp64 forward keeps every ReLU pre-activation `GAP` clear of zero"""
    from tests.conv1d_fixtures import _seeded

    gen = torch.Generator().manual_seed(seed)
    for attempt in range(256):
        m = _seeded(seed + 100 * attempt, build)
        X = make_x(gen)
        if _relu_gap(m, X) >= 2 * GAP:
            return m, X
    raise AssertionError("no seed keeps the ReLUs of the fixture clear of a near tie")


def fpn_fixture(mode="nearest", seed=51, B=3):
    """``(float64 CPU model, the same model, X [B, 3, 8, 8], the same, y)``: a tiny FPNSmall - widths 4 / 6 / 8, 4 pyramid channels,
    ReLU, maps of 8x8, 4x4 and 2x2 - in the layout of tests/conv1d_fixtures.py (a 2-D network is its own twin)"""
    from laplace_amd.nets import FPNSmall

    m, X = _calibrated(lambda: FPNSmall(E2E_CLASSES, (4, 6, 8), 4, mode), lambda gen: torch.randn(B, 3, 8, 8, generator=gen).double(), seed)
    y = torch.randint(E2E_CLASSES, (B,), generator=torch.Generator().manual_seed(seed))
    return m, m, X, X, y


def tcn_fixture(seed=53, B=3, L=8):
    """``(float64 CPU model, its 2-D twin, X [B, 2, L], X of the twin, y)``: a tiny TCNSmall - 4 channels, kernel 3, dilations
    1 / 2 / 1 (the second block pads by reflection), ReLU"""
    from laplace_amd.nets import TCNSmall
    from tests.conv1d_fixtures import twin_of

    build = lambda dims: TCNSmall(E2E_CLASSES, 2, 4, 3, (1, 2, 1), nn.ReLU, 1, dims)  # noqa: E731
    m, X = _calibrated(lambda: build(1), lambda gen: torch.randn(B, 2, L, generator=gen).double(), seed)
    y = torch.randint(E2E_CLASSES, (B,), generator=torch.Generator().manual_seed(seed))
    return m, twin_of(m, lambda: build(2)), X, X.unsqueeze(2), y


FIXTURES = {"fpn-nearest": fpn_fixture, "fpn-bilinear": lambda: fpn_fixture("bilinear"), "tcn": tcn_fixture}
