"""KFAC-reduce on the device (csrc/lk_kfacreduce.hip): the position sum and the patch mean through the C ABI against fp64 sums of
the same inputs, and ``kfac_approx="reduce"`` end to end against ``oracle.kfac_ggn(..., kfac_approx="reduce")``.  -m gpu only.

Bounds.  A sum of n fp32 terms in ANY order errs by at most (n - 1) u sum|x| to first order, u = 2^-24; the kernels add the
rounding of the split reconstruction (exact: two halves and a power of two), of ``alpha`` / 1/L and second-order terms, which 8 u
covers: |y - ref| <= (L + 8) 2^-24 alpha sum_l |x_l|.  |x| is drawn from [0.5, 2], so one dropped or doubled position (>= 0.5
alpha) is far outside (the bound is below 0.15 alpha at L = 1100).  Factors: the project's 1e-4 |b| + 1e-6 max|b|.
Worst error / bound per case: profiles/kfac_reduce_instances.md.
"""
import copy
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
PAD = 64  # guard band, floats
WORST = {}
# layout 0 splits a row over 256 / lanes position groups (4 .. 256), layout 1 over up to 256 lanes of 1 or 4 elements
LS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1100]


@pytest.fixture(autouse=True, scope="module")
def _report():
    yield
    if WORST:
        try:
            with open(os.path.join(ROOT, "profiles", "kfac_reduce_instances.md"), "w") as fh:
                fh.write("# Worst error / bound ratios of tests/test_gpu_kfac_reduce.py (a ratio below 1 passes)\n\n| check | ratio |\n|---|---|\n")
                for k in sorted(WORST):
                    fh.write(f"| {k} | {WORST[k]:.3e} |\n")
        except OSError:  # (a read-only checkout: the figures stay in the test's output)
            pass


def _hold(key, got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"{key}: {ratio:.3e}")
    assert bool((err <= bound).all()), f"{key}: error / bound {ratio:.3e}"


def _draw(gen, *shape):
    return ((torch.rand(*shape, generator=gen, dtype=torch.float64) * 1.5 + 0.5)
            * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)).float()


def _banded(n):
    buf = torch.full((n + 2 * PAD,), 7.0, device=DEV)
    return buf, buf[PAD:PAD + n]


def _bands_intact(buf, n):
    return bool((buf[:PAD] == 7.0).all()) and bool((buf[PAD + n:] == 7.0).all())


# every (D, R) on aligned bases, and one shape with the base one element on (the 4-byte / 2-byte path of a wide shape)
SHAPES = [(D, R, 0) for D in (1, 3, 4, 68) for R in (1, 3)] + [(68, 3, 1)]


@pytest.mark.parametrize("D,R,off", SHAPES)
@pytest.mark.parametrize("source", ["f32", "planes"])
@pytest.mark.parametrize("layout", [0, 1])
def test_position_sum(layout, source, D, R, off):
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    gen = torch.Generator().manual_seed(1000 * layout + 10 * D + R)
    st = K._stream(torch.device(DEV))
    alpha = 0.3
    for L in LS:
        shape = (R, L, D) if layout == 0 else (R, D, L)
        x = _draw(gen, *shape)
        if source == "planes":  # value = (p0 + p1) 2^-3, the reference from the planes themselves
            p0 = (x * 8).half()
            planes = torch.stack([p0, (x * 8 - p0.float()).half()])
            val = (planes[0].double() + planes[1].double()) / 8
            hold = torch.zeros(2, x.numel() + 8, dtype=torch.float16, device=DEV)
            hold[:, off:off + x.numel()] = planes.reshape(2, -1).to(DEV)
            sexp = torch.tensor([3], dtype=torch.int32, device=DEV)
            src = (hold[0, off:].data_ptr(), hold[1, off:].data_ptr(), sexp.data_ptr())
            fn = K.lib.lk_possum_f16x2
        else:
            val = x.double()
            hold = torch.zeros(x.numel() + 8, device=DEV)
            hold[off:off + x.numel()] = x.reshape(-1).to(DEV)
            src = (hold[off:].data_ptr(),)
            fn = K.lib.lk_possum_f32
        dim = 1 if layout == 0 else 2
        ref, bound = alpha * val.sum(dim), (L + 8) * U * alpha * val.abs().sum(dim)
        buf, y = _banded(R * D)
        assert fn(*src, R, L, D, layout, alpha, y.data_ptr(), st) == 0, K.lib.lk_last_error()
        first = y.clone()
        assert fn(*src, R, L, D, layout, alpha, y.data_ptr(), st) == 0
        assert torch.equal(first, y), f"two equal calls differ at L = {L}"
        assert _bands_intact(buf, R * D), f"a guard band was written at L = {L}"
        _hold(f"possum layout {layout} {source} D={D} R={R} off={off}", y.reshape(R, D), ref, bound)


# (kernel, stride, padding, dilation, maps)
SQUARE = [(1, 1), (5, 7), (8, 8)]
GEOMETRIES = {
    "3x3 s1 p1": ((3, 3), (1, 1), (1, 1), (1, 1), SQUARE),
    "3x3 s2 p1": ((3, 3), (2, 2), (1, 1), (1, 1), SQUARE),  # (8 x 8: the last row and column are unused)
    "1x1 s2": ((1, 1), (2, 2), (0, 0), (1, 1), SQUARE),
    "7x7 s2 p3": ((7, 7), (2, 2), (3, 3), (1, 1), SQUARE),
    "5x5 d2 p4": ((5, 5), (1, 1), (4, 4), (2, 2), SQUARE),
    "1x3": ((1, 3), (1, 1), (0, 1), (1, 1), SQUARE),
    "3x1": ((3, 1), (1, 1), (1, 0), (1, 1), SQUARE),
    "3x3 p2": ((3, 3), (1, 1), (2, 2), (1, 1), SQUARE),  # (taps wholly outside the map)
    "conv1d k5 s2 p2": ((1, 5), (1, 2), (0, 2), (1, 1), [(1, 1), (1, 7), (1, 8)]),  # the unit-height lift
    "16x16 H=300": ((16, 16), (1, 1), (0, 0), (1, 1), [(300, 16)]),  # (channels-last, C = 4: 75 KiB of LDS, above the static limit)
}


def _patch_case(K, key, x, cl, geo, order):
    ks, st, pd, dl = geo
    B, C, H, W = x.shape
    cols = F.unfold(x.double(), ks, dilation=dl, padding=pd, stride=st)
    Lp = cols.shape[2]
    ref, mass = cols.mean(2), F.unfold(x.double().abs(), ks, dilation=dl, padding=pd, stride=st).mean(2)
    if not order:  # native: (kh, kw, ci)
        ref, mass = (t.reshape(B, C, -1).transpose(1, 2).reshape(B, -1) for t in (ref, mass))
    xd = (x.permute(0, 2, 3, 1) if cl else x).contiguous().to(DEV)
    buf, out = _banded(ref.numel())
    args = (xd.data_ptr(), B, C, H, W, int(cl), *ks, *st, *pd, *dl, int(order), out.data_ptr(), K._stream(xd.device))
    assert K.lib.lk_patch_mean_f32(*args) == 0, K.lib.lk_last_error()
    first = out.clone()
    assert K.lib.lk_patch_mean_f32(*args) == 0
    assert torch.equal(first, out) and _bands_intact(buf, ref.numel())
    _hold(key, out.reshape(ref.shape), ref, (Lp + 8) * U * mass)


@pytest.mark.parametrize("order", [0, 1], ids=["native", "unfold"])
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_patch_mean(name, cl, order):
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    *geo, maps = GEOMETRIES[name]
    gen = torch.Generator().manual_seed(len(name) + 2 * cl + order)
    for H, W in maps:
        for B, C in ([(3, 4)] if H == 300 else [(3, 1), (3, 3), (1, 4), (3, 32), (3, 68)]):
            _patch_case(K, f"patch mean {name} {'nhwc' if cl else 'nchw'} {'unfold' if order else 'native'}",
                        _draw(gen, B, C, H, W), cl, geo, order)


def test_patch_mean_refuses_what_does_not_fit():
    """H * kw floats a channel beyond the 160 KiB of LDS: the error code, and nothing is written"""
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    x = torch.ones(1, 2600, 16, 1, device=DEV)  # NHWC memory of a [1, 1, 2600, 16] map
    buf, out = _banded(16 * 16)
    rc = K.lib.lk_patch_mean_f32(x.data_ptr(), 1, 1, 2600, 16, 1, 16, 16, 1, 1, 0, 0, 1, 1, 0, out.data_ptr(), K._stream(x.device))
    assert rc == -1 and b"do not fit the LDS" in K.lib.lk_last_error()
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
    assert K.patch_mean_variant((1, 1, 2600, 16), True, (16, 16), (1, 1), (0, 0), (1, 1)) is None


class _Tiny(nn.Module):
    """a ResNet whose channel counts make it eligible for the NHWC split-fp16 sweep (G from SplitTensors)"""

    def __init__(self):
        super().__init__()
        from laplace_amd.nets import BasicBlock

        self.conv1 = nn.Conv2d(3, 32, 3, 1, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(32)
        self.layers = nn.Sequential(BasicBlock(32, 32, 1), BasicBlock(32, 64, 2))
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(64, 5)

    def forward(self, x):
        x = torch.relu(self.bn1(self.conv1(x)))
        return self.fc(torch.flatten(self.pool(self.layers(x)), 1))


def _fixture(name):
    if name != "tiny":
        from oracle.fixtures import make_fixture

        m64, X64, y, _ = make_fixture(name)
        return m64, X64, y
    torch.manual_seed(5)
    m64 = _Tiny().double().eval()
    for mod in m64.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.3), mod.running_var.uniform_(0.5, 2.0)
            mod.weight.requires_grad_(False), mod.bias.requires_grad_(False)
    return m64, torch.randn(6, 3, 8, 8, dtype=torch.float64), torch.randint(5, (6,))


def _hold_factors(key, kfacs, ref):
    assert len(kfacs) == len(ref)
    for F_, R_ in zip(kfacs, ref):
        for a, b in zip(F_, R_):
            _hold(key, a, b, 1e-4 * b.abs() + 1e-6 * b.abs().max())


@pytest.mark.parametrize("name,route", [("conv", "nchw"), ("conv", "tape"), ("resnetish", "nchw"), ("resnetish", "tape"),
                                        ("seqlin", "nchw"), ("seqlin", "tape"), ("tiny", "split")])
def test_reduce_factors_against_the_oracle(name, route):
    from laplace_amd import HipGGN
    from oracle import curvature_oracle as co

    m64, X64, y = _fixture(name)
    b = HipGGN(copy.deepcopy(m64).float().to(DEV), "classification")
    b.use_split_sweep, b.use_sweep = route == "split", route != "tape"
    N = X64.shape[0]
    loss, kron = b.kron(X64.float().to(DEV), y.to(DEV), N, kfac_approx="reduce")
    if route == "split":
        assert getattr(b._tape().sweep, "split_ok", False), "the model did not take the NHWC split-fp16 sweep"
    loss_ref, ref = co.kfac_ggn(m64, X64, y, N, "classification", kfac_approx="reduce")
    _hold_factors(f"factors {name} {route}", kron.kfacs, ref)
    assert abs(loss.item() - loss_ref.item()) <= 1e-4 * abs(loss_ref.item())
    shared = {t.name for t in b._tape().taps if t.kind == "conv2d"}
    assert b.reduce_route and shared <= set(b.reduce_route), (shared, b.reduce_route)
    assert set(b.reduce_route.values()) == {"kernel"}, b.reduce_route


def test_fit_with_reduce_sums_the_minibatches():
    from torch.utils.data import DataLoader, TensorDataset

    from laplace_amd.laplace import HipLaplace
    from oracle import curvature_oracle as co

    m64, X64, y = _fixture("conv")
    la = HipLaplace(copy.deepcopy(m64).float().to(DEV), "classification", "all", "kron", kfac_approx="reduce")
    la.fit(DataLoader(TensorDataset(X64.float(), y), batch_size=5))
    _, ref = co.kfac_ggn(m64, X64, y, X64.shape[0], "classification", kfac_approx="reduce")
    _hold_factors("factors conv fit of two minibatches", la.H_facs.kfacs, ref)  # (la.H is the eigendecomposition by now)
    with pytest.raises(ValueError):
        HipLaplace(copy.deepcopy(m64).float().to(DEV), "classification", "all", "kron", kfac_approx="shrink")
