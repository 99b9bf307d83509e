"""Channel concatenation of the NHWC split-fp16 sweep on the device (-m gpu): the kernels alone (csrc/lk_cat.hip through the C ABI)
bit for bit against torch on the CPU evaluated from the same inputs, and two small DenseNets through ``SplitSweep``, ``HipGGN`` and
the Kron GLM predictive against float64 autograd and the oracle.

Kernel level.  The shape table is tests/cat_fixtures.CASES (tests/test_cat_fixtures.py proves on the CPU that it reaches every
launch path and that the reference tells a kernel that ignores ``c0`` or sums in another order).  Forward: ``torch.equal`` with
``torch.cat``.  VJP: ``torch.equal`` with the fp32 sum of ``part.float()[..., c0:c0 + Cs]`` in the listed order - the scale of a
split part is a power of two, so its product is exact and a fused multiply-add cannot change a bit.  Guard bands round ``dst`` keep
their fill, ``amax`` is ``max|dst|`` bit for bit, and a call without an ``amax`` word gives the same ``dst``.

End to end: tests/cat_fixtures.e2e_fixture - two blocks of two layers, growth 32, 8 x 8 inputs, B = 4, five classes; tanh, and
ReLU on the lattice whose float64 forward keeps every pre-activation clear of zero (asserted on the CPU in
tests/test_cat_fixtures.py) - at the project's 1e-4 relative per block, as tests/test_gpu_pool.py.  ``LK_TEST_DEVICE=cpu``
rehearses this file's host logic on the kernel emulation.
"""
import copy
import ctypes
import os

import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from oracle import curvature_oracle as co
from tests import cat_fixtures as cf

pytestmark = pytest.mark.gpu
DEV = os.environ.get("LK_TEST_DEVICE", "cuda")
PAD = 64


@pytest.fixture(autouse=True, scope="module")
def _kernels():
    if DEV != "cpu":
        yield
        return
    from laplace_amd import _lib
    from tests.emulated_cat_kernels import EmulatedCatKernels

    prev = _lib.set_kernels_for_testing(EmulatedCatKernels())
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
    (4 bytes past 16 for fp32, 2 bytes past 8 for the planes)"""

    def __init__(self, shape, off, dtype=torch.float32, init=None):
        n = 1
        for d in shape:
            n *= d
        self.fill = 7.5
        self.buf = torch.full((2 * PAD + n + 8,), self.fill, dtype=dtype, device=DEV)
        self.lo, self.hi = PAD + off, PAD + off + n
        self.t = self.buf[self.lo:self.hi].view(*shape)
        if init is not None and n:
            self.t.copy_(init)

    def ptr(self):
        """address of the interior (of the allocation plus the offset: an empty view reports a null data_ptr)"""
        return ctypes.c_void_p(self.buf.data_ptr() + self.lo * self.buf.element_size())

    def bands_intact(self):
        return bool((self.buf[:self.lo] == self.fill).all()) and bool((self.buf[self.hi:] == self.fill).all())


def _device_parts(c, parts):
    """the parts of a case in banded device buffers: per part ``_Banded`` (fp32) or ``(hi, lo, sexp tensor)``"""
    out = []
    for p in parts:
        if torch.is_tensor(p):
            out.append(_Banded(p.shape, c["off"], init=p))
        else:
            out.append((_Banded(p[0].shape, c["off"], torch.float16, init=p[0]), _Banded(p[1].shape, c["off"], torch.float16, init=p[1]),
                        torch.tensor([p[2]], dtype=torch.int32, device=DEV)))
    return out


def _vjp(c, dparts, dst, amax):
    from laplace_amd._lib import SplitTensor, get_kernels

    K, n = get_kernels(), len(dparts)
    if DEV == "cpu":
        ops = [p.t.reshape(1, 1, *p.t.shape) if isinstance(p, _Banded) else
               SplitTensor(torch.stack([p[0].t, p[1].t]).reshape(2, 1, 1, c["R"], c["Ct"]), p[2]) for p in dparts]
        if c["R"]:
            dst.t.copy_(K.cat_vjp(ops, c["c0"], c["Cs"], amax=amax).reshape(dst.t.shape))
        return
    arrays = [(ctypes.c_void_p * n)() for _ in range(4)]
    for j, p in enumerate(dparts):
        if isinstance(p, _Banded):
            arrays[0][j] = p.ptr()
        else:
            arrays[1][j], arrays[2][j], arrays[3][j] = p[0].ptr(), p[1].ptr(), p[2].data_ptr()
    rc = K.lib.lk_cat_vjp_nhwc_f32(n, *(ctypes.addressof(a) for a in arrays), c["R"], c["Ct"], c["c0"], c["Cs"], dst.ptr(),
                                   None if amax is None else ctypes.c_void_p(amax.data_ptr()), K._stream(dst.buf.device))
    assert rc == 0, K.lib.lk_last_error()


def _forward(R, Cs, src, dst, Ct, c0):
    """one source into its slice of ``dst`` (``src``: a _Banded ``[R, Cs]``)"""
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    if DEV == "cpu":
        dst.t[:, c0:c0 + Cs] = src.t
        return
    rc = K.lib.lk_cat_fwd_nhwc_f32(src.ptr(), R, Cs, dst.ptr(), Ct, c0, K._stream(dst.buf.device))
    assert rc == 0, K.lib.lk_last_error()


@pytest.mark.parametrize("c", [c for c in cf.CASES if not c["huge"]], ids=cf.case_id)
def test_kernels_bit_for_bit(c):
    gen = torch.Generator().manual_seed(5 + cf.CASES.index(c))
    R, Ct, c0, Cs, off = c["R"], c["Ct"], c["c0"], c["Cs"], c["off"]
    # forward: the map in three sources - what lies before the slice, the slice, what lies behind it - against torch.cat
    widths = [w for w in (c0, Cs, Ct - c0 - Cs) if w]
    srcs = [torch.randn(R, w, generator=gen) * 1.3 + 0.01 for w in widths]
    y, at = _Banded((R, Ct), off), 0
    for s in srcs:
        _forward(R, s.shape[1], _Banded(s.shape, off, init=s), y, Ct, at)
        at += s.shape[1]
    assert y.bands_intact(), "y: written outside its extent"
    assert torch.equal(y.t.cpu(), torch.cat(srcs, 1)), "y is not torch.cat of the sources"

    parts = cf.make_parts(c, gen)
    want = cf.vjp_reference(c, parts)
    dparts = _device_parts(c, parts)
    dst, amax = _Banded((R, Cs), off), torch.zeros(1, device=DEV)
    _vjp(c, dparts, dst, amax)
    assert dst.bands_intact(), "dst: written outside its extent"
    assert torch.equal(dst.t.cpu(), want), "dst is not the slice of the sum of the parts in the listed order"
    assert bool(torch.isfinite(dst.t).all())
    want_max = want.abs().max().reshape(1) if R else torch.zeros(1)
    assert torch.equal(amax.cpu().view(torch.int32), want_max.view(torch.int32)), "amax is not max|dst|"
    dst2 = _Banded((R, Cs), off)
    _vjp(c, dparts, dst2, None)  # (no amax word)
    assert torch.equal(dst.buf, dst2.buf), "a run without an amax word gives another dst"


def test_offsets_past_2_to_the_31():
    """a part of more than 2^31 elements: the forward writes its last four channels, the VJP reads them back"""
    c = next(c for c in cf.CASES if c["huge"])
    if DEV == "cpu":
        return  # (8 GiB of host memory for a rehearsal of host logic that the small cases already rehearse)
    R, Ct, c0, Cs = c["R"], c["Ct"], c["c0"], c["Cs"]
    assert R * Ct > 1 << 31 and c["kinds"] == ("f32",)
    vals = torch.randn(R, Cs, generator=torch.Generator().manual_seed(3)) + 0.01
    src = _Banded((R, Cs), 0, init=vals)
    big = _Banded((R, Ct), 0)  # (only its guard bands and the slice are looked at)
    _forward(R, Cs, src, big, Ct, c0)
    assert bool((big.buf[:big.lo] == big.fill).all()) and bool((big.buf[big.hi:] == big.fill).all())
    assert torch.equal(big.t[:, c0:].cpu(), vals) and bool((big.t[-1, :c0] == big.fill).all()) and bool((big.t[0, :c0] == big.fill).all())
    dst, amax = _Banded((R, Cs), 0), torch.zeros(1, device=DEV)
    _vjp(c, [big], dst, amax)
    assert dst.bands_intact() and torch.equal(dst.t.cpu(), vals)
    assert torch.equal(amax.cpu().view(torch.int32), vals.abs().max().reshape(1).view(torch.int32))


def test_the_bindings():
    """the Python bindings allocate what the C ABI takes, work without an ``amax`` word and refuse what does not belong together"""
    from laplace_amd._lib import LaplaceHipError, SplitTensor, get_kernels

    K = get_kernels()
    gen = torch.Generator().manual_seed(4)
    srcs = [torch.randn(2, 3, 5, w, generator=gen).to(DEV) for w in (8, 4, 36)]
    y = K.cat_forward(srcs)
    assert tuple(y.shape) == (2, 3, 5, 48) and torch.equal(y, torch.cat(srcs, 3))
    c = dict(R=30, Ct=48, c0=8, Cs=4, kinds=("split", "f32", "split"), sexp=(2, -1), off=0, huge=False)
    parts = cf.make_parts(c, gen)
    ops = [p.reshape(2, 3, 5, 48).to(DEV) if torch.is_tensor(p) else
           SplitTensor(torch.stack([p[0], p[1]]).reshape(2, 2, 3, 5, 48).to(DEV), torch.tensor([p[2]], dtype=torch.int32, device=DEV))
           for p in parts]
    dx = K.cat_vjp(ops, 8, 4)
    assert tuple(dx.shape) == (2, 3, 5, 4) and torch.equal(dx.reshape(30, 4).cpu(), cf.vjp_reference(c, parts))
    word = torch.zeros(1, device=DEV)
    assert torch.equal(K.cat_vjp(ops, 8, 4, amax=word), dx) and torch.equal(word, dx.abs().max().reshape(1))
    if DEV != "cpu":
        with pytest.raises(LaplaceHipError):
            K.cat_vjp(ops, 46, 4)  # (no slice of 48 channels)
        with pytest.raises(LaplaceHipError):
            K.cat_vjp(ops + ops[:2], 8, 4)  # (five parts)
        with pytest.raises(LaplaceHipError):
            K.cat_vjp([ops[1], ops[1][:, :, :, :40].contiguous()], 8, 4)
        with pytest.raises(LaplaceHipError):
            K.cat_vjp([SplitTensor(ops[0].planes, torch.zeros(2, dtype=torch.int32, device=DEV))], 8, 4)  # (one scale per image)
        with pytest.raises(LaplaceHipError, match="chunk-major split tensor is no NHWC map"):
            K.cat_vjp([SplitTensor(ops[0].planes, ops[0].sexp, chunked=True)], 8, 4)
        with pytest.raises(LaplaceHipError):
            K.cat_forward([srcs[0], srcs[1][:, :2].contiguous()])
        with pytest.raises(LaplaceHipError):
            K.cat_vjp([ops[1]], 8, 4, amax=torch.zeros(2, device=DEV))
        with pytest.raises(LaplaceHipError, match="dst overlaps|null pointer|out of range"):
            K._rc(K.lib.lk_cat_fwd_nhwc_f32(srcs[0].data_ptr(), 30, 8, srcs[0].data_ptr(), 8, 0, None), "lk_cat_fwd_nhwc_f32")


# ---- 2. the small DenseNets ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["relu", "tanh"])
def e2e(request):
    """(fp64 CPU model, X, y, seeds, fp64 per-tap inputs and cotangents, oracle Jacobians, factors and predictive variance) -
    computed once per fixture and left unchanged"""
    from tests.norm_sweep_fixtures import autograd_reference

    kind = request.param
    m64, X, y = cf.e2e_fixture(kind)
    seeds = torch.randn(4, X.shape[0], cf.E2E_CLASSES, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    taps = cf.e2e_taps(m64)
    f, ins, grads = autograd_reference(m64, taps, X, seeds)
    Js, _ = co.jacobians(m64, X)
    loss, kf = co.kfac_ggn(m64, X, y, X.shape[0], "classification")
    Qs, ls = co.kron_decompose(kf)
    f_var = cf.functional_variance_kron(Js, Qs, ls, 0.5)
    return dict(kind=kind, m64=m64, X=X, y=y, seeds=seeds, f=f.detach(), ins=ins, grads=grads, Js=Js, loss=loss, kf=kf, f_var=f_var)


def test_e2e_taps_of_the_split_sweep_against_float64_autograd(e2e):
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep_nhwc import SplitSweep

    model = copy.deepcopy(e2e["m64"]).float().to(DEV)
    taps = cf.e2e_taps(model)
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
    tape = b._tape()
    assert not getattr(tape, "sweep_reason", None), tape.sweep_reason
    assert isinstance(tape.sweep, SplitSweep) and tape.sweep.split_ok, getattr(tape.sweep, "split_reason", None)
    check(loss, e2e["loss"], what="loss")
    _factors(kron, e2e["kf"], "kron")
    la = HipLaplace(model, "classification", "all", "kron", prior_precision=0.5)
    la.fit(DataLoader(TensorDataset(Xd, yd), batch_size=X.shape[0]))
    _, f_var = la._glm_predictive_distribution(Xd)
    check(f_var, e2e["f_var"], what="Kron GLM predictive variance")


def test_the_switch_gives_the_same_results_on_the_nchw_sweep(e2e, monkeypatch):
    """``SplitSweep.nhwc_cat = False`` (the NCHW sweep with its own CAT rule) against the same oracle at the same tolerance"""
    from laplace_amd import HipGGN
    from laplace_amd.laplace import HipLaplace
    from laplace_amd.sweep_nhwc import SplitSweep

    monkeypatch.setattr(SplitSweep, "nhwc_cat", False)
    m64, X, y = e2e["m64"], e2e["X"], e2e["y"]
    model = copy.deepcopy(m64).float().to(DEV)
    Xd, yd = X.float().to(DEV), y.to(DEV)
    b = HipGGN(model, "classification")
    Js, f = b.jacobians(Xd)
    loss, kron = b.kron(Xd, yd, N=X.shape[0])
    tape = b._tape()
    assert not getattr(tape, "sweep_reason", None), tape.sweep_reason
    assert not getattr(tape.sweep, "split_ok", False) and tape.sweep.split_reason == "cat: cat has no NHWC rule"
    check(f, e2e["f"], what="f")
    check(Js, e2e["Js"], what="jacobians")
    check(loss, e2e["loss"], what="loss")
    _factors(kron, e2e["kf"], "kron (nhwc_cat = False)")
    la = HipLaplace(model, "classification", "all", "kron", prior_precision=0.5)
    la.fit(DataLoader(TensorDataset(Xd, yd), batch_size=X.shape[0]))
    _, f_var = la._glm_predictive_distribution(Xd)
    check(f_var, e2e["f_var"], what="Kron GLM predictive variance (nhwc_cat = False)")
