"""1-D convolutional networks on the device (-m gpu): the kernels of csrc/lk_reduce.hip alone, through the C ABI, against the stated
references of tests/conv1d_fixtures.py, and a tiny ResNet1d and TextCNN through ``HipGGN`` / ``HipLaplace`` against the fp64 oracle
(the KFAC factors against the oracle run on the unit-height 2-D twin).

Kernel level.  The shape table is tests/conv1d_fixtures.CASES (tests/test_conv1d_fixtures.py proves on the CPU that it reaches every
path of ``lk_reduce_variant`` and that the references tell a last-maximum kernel, a first-index ``amax`` and a skipped zero fill).
``y``, ``idx``, ``cnt`` and the first-mode ``dx`` are ``torch.equal`` with the reference (the zeros of ``dx`` are ``+0.0`` by bit
pattern); the even-mode ``dx`` lies within ``2^-23 |g / cnt|`` of the fp64 quotient - one fp32 division that need not be correctly
rounded.  Every output starts as NaN inside guard bands that keep their fill; a second run gives the same bits.

End to end: the checks of the CPU tier (tests/test_sweep_conv1d.py) on the device, with the kernels on and off.  The worst
error / bound ratios go to profiles/conv1d_instances.md.  ``LK_TEST_DEVICE=cpu`` rehearses this file's host logic on the emulation.
"""
import ctypes
import os

import pytest
import torch

from tests import conv1d_fixtures as cf

pytestmark = pytest.mark.gpu
DEV = os.environ.get("LK_TEST_DEVICE", "cuda")
PAD = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}


@pytest.fixture(autouse=True, scope="module")
def _kernels():
    if DEV != "cpu":
        yield
    else:
        from laplace_amd import _lib
        from tests.emulated_reduce_kernels import EmulatedReduceKernels

        prev = _lib.set_kernels_for_testing(EmulatedReduceKernels())
        yield
        _lib.set_kernels_for_testing(prev)
    if WORST and DEV != "cpu":
        path = os.path.join(ROOT, "profiles", "conv1d_instances.md")
        try:
            with open(path, "w") as fh:
                fh.write("# Worst error / bound ratios of tests/test_gpu_conv1d.py (a ratio below 1 passes)\n\n| check | ratio |\n|---|---|\n")
                for k in sorted(WORST):
                    fh.write(f"| {k} | {WORST[k]:.3e} |\n")
        except OSError:  # (a read-only checkout: the figures stay in the test's output)
            pass


def _worst(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))
    print(f"{key}: {ratio:.3e}")


class _Banded:
    """``numel`` elements inside guard bands of ``PAD`` elements of NaN (float) / -7 (int32), compared by bit pattern; ``off``: the
    interior starts ``off`` elements past a 16-byte aligned address; the interior starts as NaN / -1 unless ``init`` is given"""

    def __init__(self, shape, off, dtype=torch.float32, init=None):
        n = 1
        for d in shape:
            n *= d
        fill = float("nan") if dtype == torch.float32 else -7
        self.buf = torch.full((2 * PAD + n + 8,), fill, dtype=dtype, device=DEV)
        self.lo, self.hi = PAD + off, PAD + off + n
        self.t = self.buf[self.lo:self.hi].view(*shape)
        if n:
            self.t.fill_(float("nan") if dtype == torch.float32 else -1)
        self.bands = torch.cat([self.buf[:self.lo], self.buf[self.hi:]]).view(torch.int32).clone()
        if init is not None and n:
            self.t.copy_(init)

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + self.lo * 4)

    def bands_intact(self):
        return torch.equal(torch.cat([self.buf[:self.lo], self.buf[self.hi:]]).view(torch.int32), self.bands)


def _forward(c, x, y, idx, cnt):
    from laplace_amd._lib import get_kernels

    K, o, L, i = get_kernels(), c["outer"], c["L"], c["inner"]
    if DEV == "cpu":
        for dst, src in zip((y, idx, cnt), K.maxred_forward(x.t.contiguous(), o, L, i)):
            dst.t.copy_(src)
        return
    rc = K.lib.lk_maxred_fwd_f32(x.ptr(), o, L, i, y.ptr(), idx.ptr(), cnt.ptr(), K._stream(x.buf.device))
    assert rc == 0, K.lib.lk_last_error()


def _vjp(c, g, dx, idx=None, x=None, y=None, cnt=None):
    from laplace_amd._lib import get_kernels

    K, S, o, L, i = get_kernels(), c["S"], c["outer"], c["L"], c["inner"]
    if DEV == "cpu":
        t = lambda b: None if b is None else b.t.contiguous()
        dx.t.copy_(K.maxred_vjp(t(g), S, o, L, i, idx=t(idx), x=t(x), y=t(y), cnt=t(cnt)))
        return
    p = lambda b: None if b is None else b.ptr()
    rc = K.lib.lk_maxred_vjp_f32(g.ptr(), p(idx), p(x), p(y), p(cnt), S, o, L, i, dx.ptr(), K._stream(g.buf.device))
    assert rc == 0, K.lib.lk_last_error()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("c", cf.runnable(), ids=cf.case_id)
def test_kernels_against_the_stated_references(c):
    gen = torch.Generator().manual_seed(11 + cf.CASES.index(c))
    S, o, L, i, off = c["S"], c["outer"], c["L"], c["inner"], c["off"]
    x = cf.make_x(c, gen)
    g = torch.randn(S, o, i, generator=gen) + 0.05
    want_y, want_idx, want_cnt = cf.forward_reference(x)
    xd, gd = _Banded((o, L, i), off, init=x), _Banded((S, o, i), off, init=g)
    y, idx, cnt = _Banded((o, i), off), _Banded((o, i), off, torch.int32), _Banded((o, i), off, torch.int32)
    _forward(c, xd, y, idx, cnt)
    assert torch.equal(y.t.cpu(), want_y), "y"
    assert torch.equal(idx.t.cpu(), want_idx), "idx"
    assert torch.equal(cnt.t.cpu(), want_cnt), "cnt"
    assert y.bands_intact() and idx.bands_intact() and cnt.bands_intact() and xd.bands_intact()
    # first maximum: bit for bit, the zeros +0.0
    first = cf.vjp_reference(g, x, even=False)
    dx = _Banded((S, o, L, i), off)
    _vjp(c, gd, dx, idx=idx)
    got = dx.t.cpu()
    assert torch.equal(got, first.float()), "first-mode dx"
    assert not _bits(got)[first == 0].any(), "the zeros of dx are +0.0"
    assert dx.bands_intact() and gd.bands_intact() and idx.bands_intact()
    # even split: within one fp32 division of the fp64 quotient
    even = cf.vjp_reference(g, x, even=True)
    dx2 = _Banded((S, o, L, i), off)
    _vjp(c, gd, dx2, x=xd, y=y, cnt=cnt)
    got2 = dx2.t.cpu()
    bound = cf.even_bound(g, x).expand_as(even)
    err = (got2.double() - even).abs()
    assert not torch.isnan(got2).any() and bool((err <= bound).all()), "even-mode dx"
    assert not _bits(got2)[even == 0].any(), "the zeros of dx are +0.0"
    if err.numel() and bool((bound > 0).any()):
        _worst("even-mode dx / (2^-23 |g / cnt|)", (err[bound > 0] / bound[bound > 0]).max().item())
    assert dx2.bands_intact() and xd.bands_intact() and y.bands_intact() and cnt.bands_intact()
    # a second run: the same bits
    y2, idx2, cnt2 = _Banded((o, i), off), _Banded((o, i), off, torch.int32), _Banded((o, i), off, torch.int32)
    _forward(c, xd, y2, idx2, cnt2)
    dx3, dx4 = _Banded((S, o, L, i), off), _Banded((S, o, L, i), off)
    _vjp(c, gd, dx3, idx=idx2)
    _vjp(c, gd, dx4, x=xd, y=y2, cnt=cnt2)
    for a, b in ((y, y2), (idx, idx2), (cnt, cnt2), (dx, dx3), (dx2, dx4)):
        assert torch.equal(_bits(a.t), _bits(b.t))


def test_a_nan_in_a_row_gives_nan():
    c = cf._case(3, 65, 1, 1)
    x = cf.make_x(c, torch.Generator().manual_seed(3))
    x[1, 40, 0] = float("nan")
    for inner, xs in ((1, x), (4, x.expand(3, 65, 4).contiguous())):
        c = cf._case(3, 65, inner, 1)
        y, idx, cnt = _Banded((3, inner), 0), _Banded((3, inner), 0, torch.int32), _Banded((3, inner), 0, torch.int32)
        _forward(c, _Banded((3, 65, inner), 0, init=xs), y, idx, cnt)
        got = y.t.cpu()
        assert torch.isnan(got[1]).all() and torch.equal(got[[0, 2]], xs.amax(1)[[0, 2]])


# ---- end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cf.FIXTURES))
@pytest.mark.parametrize("kernels_on", [True, False], ids=["kernels", "torch-math"])
def test_fixture_matches_the_oracle_on_the_device(name, kernels_on, monkeypatch):
    from laplace_amd.sweep import SeedBatchedSweep

    monkeypatch.setattr(SeedBatchedSweep, "use_reduce_kernels", kernels_on)
    out = cf.run_curvature_checks(DEV, cf.FIXTURES[name](), kron=name != "resnet1d-dw")
    tape = out["backend"]._tape()
    assert getattr(tape, "sweep_reason", None) is None, tape.sweep_reason
    assert any(s not in (None, False) for s in tape.sweeps.values()), "no sweep was built"
    for k, v in out["ratios"].items():
        _worst(f"{name} ({'kernels' if kernels_on else 'torch math'}): {k}", v)


def test_the_hook_route_serves_the_fixtures_too():
    def no_sweep(b):
        b.use_sweep = False

    for name in sorted(cf.FIXTURES):
        out = cf.run_curvature_checks(DEV, cf.FIXTURES[name](), configure=no_sweep, kron=name != "resnet1d-dw")
        assert not out["backend"]._tape().sweeps
        for k, v in out["ratios"].items():
            _worst(f"{name} (autograd tape): {k}", v)
