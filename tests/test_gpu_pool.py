"""Max and average pooling of the NHWC split-fp16 sweep on the device (-m gpu): the kernels alone (csrc/lk_pool.hip through the C
ABI) against float64 torch on the CPU evaluated from the same fp32 inputs, and a small ImageNet-stem ResNet and a small VGG-shaped
stack through ``HipGGN`` and the Kron GLM predictive against float64 autograd and the oracle.

Kernel level.  The shape table is tests/pool_fixtures.CASES (tests/test_pool_fixtures.py proves on the CPU that it reaches every
launch path and that the references tell the tie rule).  Max forward: ``torch.equal`` on ``y``, and the tap codes converted to
flat indices ``torch.equal`` to ``return_indices=True``.  Max VJP: ``torch.equal`` on selection shapes; on summing shapes
``|dx - ref| <= m 2^-24 sum|terms|`` with m the most windows that share a pixel.  Average: the same form of bound with the tap /
window count + 1 for the division.  All of them hold for any summation order.  Guard bands round ``y``, ``arg`` and ``dx`` keep
their fill, ``amax`` is ``max|dx|`` bit for bit, and a second run gives the same bits.

End to end: tests/pool_fixtures.E2E - the fixtures whose float64 forward keeps every pooling window and every ReLU decision
clear of a near tie (asserted on the CPU in tests/test_pool_fixtures.py) - at the project's 1e-4 relative per block, as
tests/test_gpu_norm_sweep.py does for GroupNorm models.  ``LK_TEST_DEVICE=cpu`` rehearses this file's host logic on the kernel
emulation.
"""
import copy
import ctypes
import os

import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from oracle import curvature_oracle as co
from tests import pool_fixtures as pf

pytestmark = pytest.mark.gpu
DEV = os.environ.get("LK_TEST_DEVICE", "cuda")
PAD = 64


@pytest.fixture(autouse=True, scope="module")
def _kernels():
    if DEV != "cpu":
        yield
        return
    from laplace_amd import _lib
    from tests.emulated_pool_kernels import EmulatedPoolKernels

    prev = _lib.set_kernels_for_testing(EmulatedPoolKernels())
    yield
    _lib.set_kernels_for_testing(prev)


def rel(a, b):
    from tests.parity_log import record_error

    a, b = a.double().cpu(), b.double().cpu()
    return record_error((a - b).abs().max().item() / (b.abs().max().item() + 1e-300))


def check(got, want, tol=1e-4, what=""):
    e = rel(got, want)
    print(f"{what}: {e:.3e}")
    assert e < tol, f"{what}: rel err {e:.3e}"


# ---- 1. the kernels alone ---------------------------------------------------------------------------------------------------------
class _Banded:
    """``numel`` elements inside guard bands of ``PAD`` elements; ``off``: the interior starts one element past an aligned address
    (4 bytes past 16 for fp32, 1 byte past 4 for the code bytes)"""

    def __init__(self, shape, off, dtype=torch.float32, init=None):
        n = 1
        for d in shape:
            n *= d
        self.fill = 7.5 if dtype == torch.float32 else 201
        self.buf = torch.full((2 * PAD + n + 4,), self.fill, dtype=dtype, device=DEV)
        self.lo, self.hi = PAD + off, PAD + off + n
        self.t = self.buf[self.lo:self.hi].view(*shape)
        if init is not None:
            self.t.copy_(init)

    def bands_intact(self):
        return bool((self.buf[:self.lo] == self.fill).all()) and bool((self.buf[self.hi:] == self.fill).all())


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _geo(c):
    return (*c["k"], *c["s"], *c["p"], int(c["cip"]), int(c["div"] or 0))


def _forward(c, x, y, arg):
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    kind = pf.kernel_kind(K, c)
    if DEV == "cpu":
        got = K.pool_forward(x.t, kind, c["k"], c["s"], c["p"], c["cip"], c["div"])
        y.t.copy_(got[0])
        if arg is not None:
            arg.t.copy_(got[1])
        return
    rc = K.lib.lk_pool_fwd_nhwc_f32(kind, _p(x.t), c["B"], c["H"], c["W"], c["C"], *_geo(c), _p(y.t),
                                    _p(None if arg is None else arg.t), K._stream(x.t.device))
    assert rc == 0, K.lib.lk_last_error()


def _vjp(c, g, arg, dx, amax):
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    kind = pf.kernel_kind(K, c)
    if DEV == "cpu":
        dx.t.copy_(K.pool_vjp(g.t.reshape(c["S"] * c["B"], *g.t.shape[2:]), None if arg is None else arg.t, c["S"],
                              (c["H"], c["W"]), kind, c["k"], c["s"], c["p"], c["cip"], c["div"], amax=amax).reshape(dx.t.shape))
        return
    rc = K.lib.lk_pool_vjp_nhwc_f32(kind, _p(g.t), _p(None if arg is None else arg.t), c["S"], c["B"], c["H"], c["W"], c["C"],
                                    *_geo(c), _p(dx.t), _p(amax), K._stream(g.t.device))
    assert rc == 0, K.lib.lk_last_error()


def _within(got, want, bound, what):
    err = (got.double().cpu() - want).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    excess = (err - bound).max().item()
    print(f"{what}: worst |err| / bound {ratio:.3f}")
    assert excess <= 0.0, f"{what}: error exceeds the bound by {excess:.3e} ({ratio:.3f} of it)"


@pytest.mark.parametrize("c", pf.CASES, ids=pf.case_id)
def test_kernels_against_float64(c):
    gen = torch.Generator().manual_seed(11 + pf.CASES.index(c))
    off, (OH, OW), is_max = c["off"], pf.out_hw(c), c["kind"] == "max"
    x = _Banded((c["B"], c["H"], c["W"], c["C"]), off, init=pf.make_input(c, gen))
    y = _Banded((c["B"], OH, OW, c["C"]), off)
    arg = _Banded((c["B"], OH, OW, c["C"]), off, torch.uint8) if is_max else None
    _forward(c, x, y, arg)
    ref = pf.forward_reference(c, x.t)
    assert y.bands_intact(), "y: written outside its extent"
    if is_max:
        assert arg.bands_intact(), "arg: written outside its extent"
        assert torch.equal(y.t.double().cpu(), ref["y"]), "y is not the window maximum"
        assert torch.equal(pf.codes_to_flat_index(c, arg.t), ref["idx"]), "arg is not the first maximum in row-major order"
    else:
        _within(y.t, ref["y"], ref["bound"], "y")

    g = _Banded((c["S"], c["B"], OH, OW, c["C"]), off, init=torch.randn(c["S"], c["B"], OH, OW, c["C"], generator=gen))
    dx, amax = _Banded((c["S"], c["B"], c["H"], c["W"], c["C"]), off), torch.zeros(1, device=DEV)
    _vjp(c, g, arg, dx, amax)
    want, bound = pf.vjp_reference(c, g.t, ref.get("idx"))
    assert dx.bands_intact(), "dx: written outside its extent"
    if bound is None:
        assert torch.equal(dx.t.cpu(), want.float()), "dx is not the selected cotangent"
    else:
        _within(dx.t, want, bound, "dx")
    assert torch.equal(amax.view(torch.int32), dx.t.abs().max().reshape(1).view(torch.int32)), "amax is not max|dx|"
    dx2, amax2 = _Banded((c["S"], c["B"], c["H"], c["W"], c["C"]), off), torch.zeros(1, device=DEV)
    _vjp(c, g, arg, dx2, amax2)
    assert torch.equal(dx.buf, dx2.buf) and torch.equal(amax, amax2), "two runs on the same input differ"


def test_vjp_without_an_amax_word_and_the_binding():
    """``amax = null``; the Python binding allocates what the C ABI takes, and refuses shapes that do not belong together"""
    from laplace_amd._lib import LaplaceHipError, get_kernels

    K = get_kernels()
    c = next(c for c in pf.CASES if c["kind"] == "max" and c["k"] == (3, 3) and c["s"] == (2, 2) and c["H"] == 6 and not c["off"])
    gen = torch.Generator().manual_seed(2)
    x = pf.make_input(c, gen).to(DEV)
    y, arg = K.pool_forward(x, K.POOL_MAX, 3, 2, 1)
    ref = pf.forward_reference(c, x)
    assert torch.equal(y.double().cpu(), ref["y"]) and torch.equal(pf.codes_to_flat_index(c, arg), ref["idx"])
    g = torch.randn(c["S"], c["B"], *y.shape[1:], generator=gen).to(DEV)
    dx = K.pool_vjp(g.reshape(-1, *y.shape[1:]), arg, c["S"], (c["H"], c["W"]), K.POOL_MAX, 3, 2, 1)
    want, bound = pf.vjp_reference(c, g, ref["idx"])
    _within(dx.reshape(want.shape), want, bound, "dx")
    ya, none = K.pool_forward(x, K.POOL_AVG, (3, 3), None, (1, 1), count_include_pad=False)  # (stride None: the window)
    assert none is None and tuple(ya.shape) == (c["B"], 2, 2, c["C"])
    if DEV != "cpu":
        with pytest.raises(LaplaceHipError):
            K.pool_vjp(g.reshape(-1, *y.shape[1:]), arg, c["S"], (c["H"] + 2, c["W"]), K.POOL_MAX, 3, 2, 1)
        with pytest.raises(LaplaceHipError, match="amax is one 32-bit device word"):
            K.pool_vjp(g.reshape(-1, *y.shape[1:]), arg, c["S"], (c["H"], c["W"]), K.POOL_MAX, 3, 2, 1, amax=torch.zeros(2, device=DEV))
        with pytest.raises(LaplaceHipError):
            K.pool_forward(x, K.POOL_MAX, 9, 1, 4)  # (the C ABI's own refusal reaches the caller)


# ---- 2. the pooled workloads, small ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=sorted(pf.E2E))
def e2e(request):
    """(name, fp64 CPU model, X, y, seeds, fp64 per-tap inputs and cotangents, oracle Jacobians and factors) - computed once per
    fixture and left unchanged"""
    from tests.norm_sweep_fixtures import autograd_reference

    name = request.param
    m64, X, y = pf.e2e_fixture(name)
    seeds = torch.randn(4, X.shape[0], pf.E2E_CLASSES, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    taps = pf.e2e_taps(m64)
    f, ins, grads = autograd_reference(m64, taps, X, seeds)
    Js, _ = co.jacobians(m64, X)
    loss, kf = co.kfac_ggn(m64, X, y, X.shape[0], "classification")
    return dict(name=name, m64=m64, X=X, y=y, seeds=seeds, f=f.detach(), ins=ins, grads=grads, Js=Js, loss=loss, kf=kf)


def test_e2e_taps_of_the_split_sweep_against_float64_autograd(e2e):
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep_nhwc import SplitSweep

    model = copy.deepcopy(e2e["m64"]).float().to(DEV)
    taps = pf.e2e_taps(model)
    sw = SplitSweep(model, taps, kernels=get_kernels)
    assert sw.split_ok, sw.split_reason
    f = sw.forward(e2e["X"].float().to(DEV))
    grads = sw.backward(e2e["seeds"].float().to(DEV))
    check(f, e2e["f"], what="f")
    for n in taps:
        check(sw.taps[n]["a"], e2e["ins"][n], what=f"{n}: a")
        assert tuple(grads[n].shape) == tuple(e2e["grads"][n].shape), n
        check(grads[n], e2e["grads"][n], what=f"{n}: cotangent")


def _factors(kron, kf_ref, what):
    for i, (F_, G_) in enumerate(zip(kron.kfacs, kf_ref)):
        for j, (a, ref) in enumerate(zip(F_, G_)):
            check(a, ref, what=f"{what}: block {i} factor {j}")


def test_e2e_jacobians_kron_and_predictive_against_the_oracle(e2e):
    from laplace_amd import HipGGN
    from laplace_amd.laplace import HipLaplace
    from laplace_amd.sweep_nhwc import SplitSweep

    m64, X, y = e2e["m64"], e2e["X"], e2e["y"]
    model = copy.deepcopy(m64).float().to(DEV)
    Xd, yd = X.float().to(DEV), y.to(DEV)
    b = HipGGN(model, "classification")
    Js, f = b.jacobians(Xd)
    check(f, e2e["f"], what="f")
    check(Js, e2e["Js"], what="jacobians")
    loss, kron = b.kron(Xd, yd, N=X.shape[0])
    sweep = b._tape().sweep
    assert isinstance(sweep, SplitSweep) and sweep.split_ok, getattr(sweep, "split_reason", None)
    check(loss, e2e["loss"], what="loss")
    _factors(kron, e2e["kf"], "kron")  # (block 2: the 3 x 3 convolution behind the pool, A factor from the pooled map)
    la = HipLaplace(model, "classification", "all", "kron", prior_precision=0.5)
    la.fit(DataLoader(TensorDataset(Xd, yd), batch_size=X.shape[0]))
    _, f_var = la._glm_predictive_distribution(Xd)
    Qs, ls = co.kron_decompose(e2e["kf"])
    check(f_var, co.functional_variance_kron(e2e["Js"], Qs, ls, 0.5), what="Kron GLM predictive variance")


@pytest.mark.parametrize("e2e", pf.E2E_EXACT, indirect=True)
def test_the_switch_gives_the_default_results(e2e, monkeypatch):
    """``SplitSweep.nhwc_pool = False`` (the NCHW sweep, the route of these models before lk_pool.hip) against the same oracle at
    the same tolerance as the default route above - on the fixtures whose ties survive the library's convolutions
    (tests/pool_fixtures.E2E_EXACT)"""
    from laplace_amd import HipGGN
    from laplace_amd.sweep_nhwc import SplitSweep

    monkeypatch.setattr(SplitSweep, "nhwc_pool", False)
    m64, X, y = e2e["m64"], e2e["X"], e2e["y"]
    b = HipGGN(copy.deepcopy(m64).float().to(DEV), "classification")
    Js, f = b.jacobians(X.float().to(DEV))
    loss, kron = b.kron(X.float().to(DEV), y.to(DEV), N=X.shape[0])
    sweep = b._tape().sweep
    assert not getattr(sweep, "split_ok", False) and "has no NHWC rule" in sweep.split_reason
    check(Js, e2e["Js"], what="jacobians")
    check(loss, e2e["loss"], what="loss")
    _factors(kron, e2e["kf"], "kron (nhwc_pool = False)")
