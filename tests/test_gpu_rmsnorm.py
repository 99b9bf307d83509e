"""nn.RMSNorm, negation and difference in the seed-batched reverse sweep, on the device (-m gpu): the forward and VJP kernels alone
(csrc/lk_rmsnorm.hip through the C ABI) against float64 evaluated from the same fp32 inputs, and the sweep, ``HipGGN`` and the Kron
predictive on a small LLaMA network against the fp64 oracle, with the kernels on and off.

The kernel bounds hold for ANY summation order.  With u = 2^-24 and N = D:
    |d rstd| <= rstd (N/2 + 5) u            |d y| <= |y| ((N/2 + 5) u + 2 u)
    |d dx|   <= u rstd (4 |t| + (N + 8) |xh| mean_row|t xh|)          on the fp32 rstd the forward wrote
(tests/rmsnorm_fixtures.py derives them and states them in code; tests/test_rmsnorm_fixtures.py shows on the CPU that an fp32
evaluation sits below them and that LayerNorm's centred variance and its ``- mean_row(t)`` term sit far above).  The shape table is
tests/rmsnorm_fixtures.CASES; the same CPU file proves that it reaches every launch variant.  ``LK_TEST_DEVICE=cpu`` rehearses this
file's host logic on the kernel emulation.
"""
import copy
import ctypes
import os

import pytest
import torch
from torch import nn

from tests import rmsnorm_fixtures as rf

pytestmark = pytest.mark.gpu
DEV = os.environ.get("LK_TEST_DEVICE", "cuda")
PAD, FILL = 64, 7.5


@pytest.fixture(autouse=True, scope="module")
def _kernels():
    if DEV != "cpu":
        yield
        return
    from laplace_amd import _lib
    from tests.emulated_rmsnorm_kernels import EmulatedRmsNormKernels

    prev = _lib.set_kernels_for_testing(EmulatedRmsNormKernels())
    yield
    _lib.set_kernels_for_testing(prev)


# ---- 1. the kernels alone ---------------------------------------------------------------------------------------------------------
class _Banded:
    """``numel`` floats inside guard bands of ``PAD`` floats; ``off``: the interior starts one float past a 16-byte boundary.  An
    output (no ``init``) is pre-filled with NaN: an element the kernel leaves out fails every bound"""

    def __init__(self, shape, off, init=None):
        n = 1
        for d in shape:
            n *= d
        self.buf = torch.full((2 * PAD + n + 4,), FILL, device=DEV)
        self.lo, self.hi = PAD + off, PAD + off + n
        self.t = self.buf[self.lo:self.hi].view(*shape)
        self.t.copy_(init) if init is not None else self.t.fill_(float("nan"))

    def bands_intact(self):
        return bool((self.buf[:self.lo] == FILL).all()) and bool((self.buf[self.hi:] == FILL).all())


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _forward(c, x, w, y, rstd):
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    if DEV == "cpu":
        for dst, src in zip((y, rstd), K.rmsnorm_forward(x.t.contiguous(), None if w is None else w.t.contiguous(), rf.EPS)):
            dst.t.copy_(src)
        return
    rc = K.lib.lk_rmsnorm_fwd_f32(_p(x.t), _p(None if w is None else w.t), c["rows"], c["D"], rf.EPS, _p(y.t), _p(rstd.t),
                                  K._stream(x.t.device))
    assert rc == 0, K.lib.lk_last_error()


def _vjp(c, g, x, rstd, w, dx, amax):
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    if DEV == "cpu":
        dx.t.copy_(K.rmsnorm_vjp(g.t.reshape(-1, c["D"]).contiguous(), x.t.contiguous(), rstd.t.contiguous(),
                                 None if w is None else w.t.contiguous(), c["S"], amax=amax).reshape(dx.t.shape))
        return
    rc = K.lib.lk_rmsnorm_vjp_f32(_p(g.t), _p(x.t), _p(rstd.t), _p(None if w is None else w.t), c["S"], c["rows"], c["D"], _p(dx.t),
                                  _p(amax), K._stream(g.t.device))
    assert rc == 0, K.lib.lk_last_error()


def _ratio(got, want, bound):
    err = (got.double().cpu() - want).abs()
    return (err / bound.clamp_min(1e-300)).max().item(), bool((err <= bound).all())


@pytest.mark.parametrize("c", rf.CASES, ids=rf.case_id)
def test_kernels_against_float64(c):
    """forward on rows drawn as ``randn + 3``, then the VJP on the forward's own fp32 ``rstd``: every element within its bound (a
    NaN left in an output fails); the guard bands around ``y``, ``rstd`` and ``dx`` keep their fill; ``amax`` is ``max|dx|`` bit for
    bit; a second run gives the same bits."""
    gen = torch.Generator().manual_seed(1000 + rf.CASES.index(c))
    x0, g0, w0 = rf.make_inputs(c, gen)
    off, shape = c["off"], (c["rows"], c["D"])
    x, g = _Banded(shape, off, x0), _Banded((c["S"],) + shape, off, g0)
    w = None if w0 is None else _Banded((c["D"],), off, w0)
    y, rstd = _Banded(shape, off), _Banded((c["rows"],), off)
    _forward(c, x, w, y, rstd)
    ref = rf.forward_reference(x0, w0)
    worst = {}
    for name, got in (("y", y), ("rstd", rstd)):
        worst[name], ok = _ratio(got.t, ref[name], ref["b_" + name])
        assert ok, f"{name}: {worst[name]:.3f} of its bound"
        assert got.bands_intact(), f"{name}: written outside its extent"
    dx, amax = _Banded((c["S"],) + shape, off), torch.zeros(1, device=DEV)
    _vjp(c, g, x, rstd, w, dx, amax)
    want, bound = rf.vjp_reference(g0, x0, rstd.t.cpu(), w0)
    worst["dx"], ok = _ratio(dx.t, want, bound)
    print(f"{rf.case_id(c)}: worst |err| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert ok, f"dx: {worst['dx']:.3f} of its bound"
    assert dx.bands_intact(), "dx: written outside its extent"
    assert x.bands_intact() and g.bands_intact() and torch.equal(x.t.cpu(), x0) and torch.equal(g.t.cpu(), g0)  # (inputs untouched)
    assert torch.equal(amax.view(torch.int32), dx.t.abs().max().reshape(1).view(torch.int32)), "amax is not max|dx|"
    dx2, amax2 = _Banded((c["S"],) + shape, off), torch.zeros(1, device=DEV)
    _vjp(c, g, x, rstd, w, dx2, amax2)
    assert torch.equal(dx.buf, dx2.buf) and torch.equal(amax, amax2), "two runs on the same input differ"
    y2, rstd2 = _Banded(shape, off), _Banded((c["rows"],), off)
    _forward(c, x, w, y2, rstd2)
    assert torch.equal(y.buf, y2.buf) and torch.equal(rstd.buf, rstd2.buf), "two runs of the forward differ"


def test_no_rows_return_clean_and_the_binding():
    """``rows == 0`` touches nothing; ``amax = null``; the Python binding allocates what the C ABI takes and agrees with torch"""
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    c = dict(S=3, rows=0, D=8, w="none", off=0)
    x, g, y, rstd, dx = (_Banded(s, 0, torch.zeros(s)) for s in ((1, 8), (3, 1, 8), (1, 8), (1,), (3, 1, 8)))
    for b in (y, rstd, dx):
        b.t.fill_(FILL)
    if DEV != "cpu":  # (the C ABI itself: the binding below never gets that far with an empty matrix on the emulation)
        _forward(c, x, None, y, rstd)
        _vjp(c, g, x, rstd, None, dx, None)
    assert all(bool((b.buf == FILL).all()) for b in (y, rstd, dx))
    e = K.rmsnorm_forward(torch.empty(0, 8, device=DEV), None, 1e-6)
    assert e[0].shape == (0, 8) and e[1].shape == (0,)
    assert K.rmsnorm_vjp(torch.empty(0, 8, device=DEV), torch.empty(0, 8, device=DEV), e[1], None, 3).shape == (0, 8)
    gen = torch.Generator().manual_seed(2)
    c = dict(S=3, rows=10, D=192, w="rand", off=0)
    x0, g0, w0 = rf.make_inputs(c, gen)
    x, g, w = x0.to(DEV), g0.to(DEV), w0.to(DEV)
    y, rstd = K.rmsnorm_forward(x, w, 1e-6)
    dx = K.rmsnorm_vjp(g.reshape(-1, 192), x, rstd, w, 3)
    assert rf.violations(c, y, rstd, dx, x, g, w, 1e-6) == []
    m = nn.RMSNorm(192, eps=1e-6).double()
    with torch.no_grad():
        m.weight.copy_(w0.double())
    xr = x0.double().requires_grad_(True)
    out = m(xr)
    assert rf.rel(y, out) < 1e-5
    for s in range(3):
        (want,) = torch.autograd.grad(out, xr, g0[s].double(), retain_graph=True)
        assert rf.rel(dx.reshape(3, 10, 192)[s], want) < 1e-5
    if DEV != "cpu":
        from laplace_amd._lib import LaplaceHipError

        with pytest.raises(LaplaceHipError, match="amax is one 32-bit device word"):
            K.rmsnorm_vjp(g.reshape(-1, 192), x, rstd, w, 3, amax=torch.zeros(2, device=DEV))


# ---- 2. end to end -----------------------------------------------------------------------------------------------------------------
def test_llama_curvature_matches_the_oracle_with_the_kernels_on_and_off(monkeypatch):
    """jacobians, diag, a two-minibatch kron fit and the Kron predictive of the small LLaMA network at the project's tolerances; the
    RMSNorm kernels ran (on), did not (off), and the two routes agree within the same tolerances"""
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep import SeedBatchedSweep
    from tests.slice_fixtures import run_curvature_checks

    K, calls = get_kernels(), []
    fwd, vjp = K.rmsnorm_forward, K.rmsnorm_vjp
    monkeypatch.setattr(K, "rmsnorm_forward", lambda *a, **kw: (calls.append("fwd"), fwd(*a, **kw))[1], raising=False)
    monkeypatch.setattr(K, "rmsnorm_vjp", lambda *a, **kw: (calls.append("vjp"), vjp(*a, **kw))[1], raising=False)
    fixture = rf.llama_fixture()
    on = run_curvature_checks(DEV, fixture, want_split=False)
    assert "fwd" in calls and "vjp" in calls
    calls.clear()
    monkeypatch.setattr(SeedBatchedSweep, "use_rmsnorm_kernels", False)
    off = run_curvature_checks(DEV, fixture, want_split=False)
    assert not calls
    for k in ("Js", "f", "h", "f_var"):
        assert rf.rel(on[k], off[k]) < 1e-4, k
    for a, b in zip(on["kfacs"], off["kfacs"]):
        assert rf.rel(a, b) < 1e-4


def test_tracked_rmsnorm_weights_against_the_oracle():
    from laplace_amd import HipGGN
    from oracle import curvature_oracle as co

    m64, X64, y = rf.llama_fixture(track_norm=True)
    model, X = copy.deepcopy(m64).float().to(DEV), X64.float().to(DEV)
    backend = HipGGN(model, "classification")
    tape = backend._tape()
    assert [t.name for t in tape.norm_taps] == ["blocks.0.norm1", "blocks.0.norm2", "norm"] and tape.unserved == []
    Js64, f64 = co.jacobians(m64, X64)
    Js, f = backend.jacobians(X)
    assert rf.rel(f, f64) < 1e-5 and rf.rel(Js, Js64) < 1e-4, (rf.rel(f, f64), rf.rel(Js, Js64))
    for t in tape.norm_taps:
        cols = slice(t.w_off, t.w_off + 32)
        assert rf.rel(Js[..., cols], Js64[..., cols]) < 1e-4, t.name
    assert getattr(tape, "sweep_reason", None) is None and tape.sweeps.get(frozenset({"norm"})) not in (None, False)
    _, h = backend.diag(X, y.to(DEV))
    assert rf.rel(h, co.ggn_diag(Js64, co.functional_hessian(f64, "classification"))) < 1e-4
    with pytest.raises(NotImplementedError, match="KFAC supports nn.Linear / nn.Conv2d parameters only"):
        backend.kron(X, y.to(DEV), N=len(X))


class _ConvRms(nn.Module):
    def __init__(self):
        super().__init__()
        self.c0, self.c1, self.fc = nn.Conv2d(3, 32, 3, 1, 1), nn.Conv2d(32, 32, 3, 1, 1), nn.Linear(32, 3)
        self.norm = nn.RMSNorm(32)

    def forward(self, x):
        h = torch.tanh(self.c1(torch.tanh(self.c0(x))))
        return self.fc(self.norm(h.mean((2, 3))))


def test_a_conv_rmsnorm_model_reaches_the_nchw_sweep_with_the_named_reason():
    from laplace_amd import HipGGN
    from oracle import curvature_oracle as co

    torch.manual_seed(14)
    m64 = _ConvRms().double().eval()
    m64.norm.weight.requires_grad_(False)
    X64, y = torch.randn(4, 3, 8, 8, dtype=torch.float64), torch.arange(4) % 3
    backend = HipGGN(copy.deepcopy(m64).float().to(DEV), "classification")
    Js, f = backend.jacobians(X64.float().to(DEV))
    tape = backend._tape()
    assert getattr(tape, "sweep_reason", None) is None and tape.sweep not in (None, False)
    assert not tape.sweep.split_ok and tape.sweep.split_reason == "norm: RMSNorm has no NHWC rule"
    Js64, f64 = co.jacobians(m64, X64)
    assert rf.rel(f, f64) < 1e-4 and rf.rel(Js, Js64) < 1e-4, (rf.rel(f, f64), rf.rel(Js, Js64))
