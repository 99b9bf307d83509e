"""Static slicing of both reverse sweeps on the device (-m gpu): the kernels alone (csrc/lk_slice.hip through the C ABI) bit for bit
against the emulation's rule evaluated on the CPU from the same inputs, and a small CSPNetSmall and ViTClassToken through
``SplitSweep`` / ``SeedBatchedSweep``, ``HipGGN`` and the Kron GLM predictive against float64 autograd and the oracle.

Kernel level.  The shape table is tests/slice_fixtures.CASES (tests/test_slice_fixtures.py proves on the CPU that it reaches every
launch path and that the reference tells a kernel that drops the zero fill, ignores ``c0`` or sums in another order).  Forward:
``torch.equal`` with the column range.  VJP: ``torch.equal`` with tests/slice_fixtures.vjp_reference - the order of the fp32 sums is
fixed and the scale of a split piece is a power of two, so no tolerance is involved.  ``dst`` starts as NaN (the kernel owes every
element, the zeros included) inside guard bands of ``-0.0`` / NaN that keep their fill; ``amax`` is ``max|dst|`` bit for bit; a call
without an ``amax`` word and a second equal call give the same bits.

End to end: tests/slice_fixtures.csp_fixture (widths 64 / 64, 8 x 8 inputs, B = 4, tanh) and vit_fixture (dim 32, T = 5, B = 3) at
the project's 1e-4 relative per block, as tests/test_gpu_cat.py.  ``LK_TEST_DEVICE=cpu`` rehearses this file's host logic on the
kernel emulation.
"""
import copy
import ctypes
import os

import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from oracle import curvature_oracle as co
from tests import slice_fixtures as sf
from tests.cat_fixtures import functional_variance_kron

pytestmark = pytest.mark.gpu
DEV = os.environ.get("LK_TEST_DEVICE", "cuda")
PAD = 64


@pytest.fixture(autouse=True, scope="module")
def _kernels():
    if DEV != "cpu":
        yield
        return
    from laplace_amd import _lib
    from tests.emulated_slice_kernels import EmulatedSliceKernels

    prev = _lib.set_kernels_for_testing(EmulatedSliceKernels())
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
    """``numel`` elements inside guard bands of ``PAD`` elements filled with ``fill`` (NaN or -0.0: compared by bit pattern);
    ``off``: the interior starts one element past an aligned address (4 bytes past 16 for fp32, 2 bytes past 8 for the planes);
    the interior starts as NaN unless ``init`` is given"""

    def __init__(self, shape, off, dtype=torch.float32, init=None, fill=float("nan")):
        n = 1
        for d in shape:
            n *= d
        self.buf = torch.full((2 * PAD + n + 8,), fill, dtype=dtype, device=DEV)
        self.lo, self.hi = PAD + off, PAD + off + n
        self.t = self.buf[self.lo:self.hi].view(*shape)
        if n:
            self.t.fill_(float("nan"))
        self.bands = self._bits(torch.cat([self.buf[:self.lo], self.buf[self.hi:]])).clone()
        if init is not None and n:
            self.t.copy_(init)

    @staticmethod
    def _bits(t):
        return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)

    def ptr(self):
        """address of the interior (of the allocation plus the offset: an empty view reports a null data_ptr)"""
        return ctypes.c_void_p(self.buf.data_ptr() + self.lo * self.buf.element_size())

    def bands_intact(self):
        return torch.equal(self._bits(torch.cat([self.buf[:self.lo], self.buf[self.hi:]])), self.bands)


def _device_pieces(c, pieces):
    """the pieces of a case in banded device buffers: per piece ``(_Banded | (hi, lo, sexp tensor), c0, cs)``"""
    out = []
    for p, c0, cs in pieces:
        if torch.is_tensor(p):
            out.append((_Banded(p.shape, c["off"], init=p, fill=-0.0), c0, cs))
        else:
            out.append(((_Banded(p[0].shape, c["off"], torch.float16, init=p[0]),
                         _Banded(p[1].shape, c["off"], torch.float16, init=p[1], fill=-0.0),
                         torch.tensor([p[2]], dtype=torch.int32, device=DEV)), c0, cs))
    return out


def _vjp(c, dpieces, dst, amax):
    from laplace_amd._lib import SplitTensor, get_kernels

    K, n, R, Ct = get_kernels(), len(dpieces), c["R"], c["Ct"]
    if DEV == "cpu":
        ops = [(p.t if isinstance(p, _Banded) else SplitTensor(torch.stack([p[0].t, p[1].t]), p[2]), c0, cs) for p, c0, cs in dpieces]
        if R:
            dst.t.copy_(K.slice_vjp(ops, R, Ct, amax=amax))
        return
    arrays = [(ctypes.c_void_p * n)() for _ in range(4)]
    c0s, css = (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)()
    for j, (p, c0, cs) in enumerate(dpieces):
        c0s[j], css[j] = c0, cs
        if isinstance(p, _Banded):
            arrays[0][j] = p.ptr()
        else:
            arrays[1][j], arrays[2][j], arrays[3][j] = p[0].ptr(), p[1].ptr(), p[2].data_ptr()
    rc = K.lib.lk_slice_vjp_f32(n, *(ctypes.addressof(a) for a in arrays), ctypes.addressof(c0s), ctypes.addressof(css), R, Ct,
                                dst.ptr(), None if amax is None else ctypes.c_void_p(amax.data_ptr()), K._stream(dst.buf.device))
    assert rc == 0, K.lib.lk_last_error()


def _forward(src, R, Ct, c0, cs, dst):
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    if DEV == "cpu":
        if R:
            dst.t.copy_(K.slice_forward(src.t.contiguous(), R, Ct, c0, cs))
        return
    rc = K.lib.lk_slice_fwd_f32(src.ptr(), R, Ct, c0, cs, dst.ptr(), K._stream(dst.buf.device))
    assert rc == 0, K.lib.lk_last_error()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("c", [c for c in sf.CASES if not c["wide"]], ids=sf.case_id)
def test_kernels_bit_for_bit(c):
    gen = torch.Generator().manual_seed(5 + sf.CASES.index(c))
    R, Ct, off = c["R"], c["Ct"], c["off"]
    # forward: every column range of the case out of one [R, Ct] matrix
    x = torch.randn(R, Ct, generator=gen) * 1.3 + 0.01
    src = _Banded((R, Ct), off, init=x)
    for c0, cs in sorted({(c0, cs) for c0, cs, _ in c["pieces"]}):
        y = _Banded((R, cs), off, fill=-0.0)
        _forward(src, R, Ct, c0, cs, y)
        assert y.bands_intact(), "y: written outside its extent"
        assert torch.equal(_bits(y.t.cpu()), _bits(sf.forward_reference(x, c0, cs))), "y is not the column range of the source"

    pieces = sf.make_pieces(c, gen)
    want = sf.vjp_reference(pieces, R, Ct)
    dpieces = _device_pieces(c, pieces)
    dst, amax = _Banded((R, Ct), off), torch.zeros(1, device=DEV)
    _vjp(c, dpieces, dst, amax)
    assert dst.bands_intact(), "dst: written outside its extent"
    assert bool(torch.isfinite(dst.t).all()), "dst: an element was not written"
    assert torch.equal(_bits(dst.t.cpu()), _bits(want)), "dst is not the sum of the covering pieces in the listed order"
    want_max = want.abs().max().reshape(1) if R else torch.zeros(1)
    assert torch.equal(amax.cpu().view(torch.int32), want_max.view(torch.int32)), "amax is not max|dst|"
    dst2 = _Banded((R, Ct), off)
    _vjp(c, dpieces, dst2, None)  # (no amax word)
    assert torch.equal(_bits(dst.buf), _bits(dst2.buf)), "a run without an amax word gives another dst"
    dst3, amax3 = _Banded((R, Ct), off), torch.zeros(1, device=DEV)
    _vjp(c, dpieces, dst3, amax3)
    assert torch.equal(_bits(dst.buf), _bits(dst3.buf)) and torch.equal(amax, amax3), "two equal calls differ"
    assert all((p if isinstance(p, _Banded) else p[0]).bands_intact() for p, _, _ in dpieces)


def test_the_bindings():
    """the Python bindings allocate what the C ABI takes, work without an ``amax`` word and refuse what does not belong together"""
    from laplace_amd._lib import LaplaceHipError, SplitTensor, get_kernels

    K = get_kernels()
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, 5, 48, generator=gen)
    y = K.slice_forward(x.to(DEV), 30, 48, 8, 36)
    assert tuple(y.shape) == (30, 36) and torch.equal(y.cpu(), x.reshape(30, 48)[:, 8:44])
    c = dict(R=30, Ct=48, pieces=((8, 4, "split"), (0, 48, "f32"), (8, 40, "split")), sexp=(2, -1), off=0, cancel=False, wide=False)
    pieces = sf.make_pieces(c, gen)
    ops = [(p.to(DEV) if torch.is_tensor(p) else
            SplitTensor(torch.stack([p[0], p[1]]).to(DEV), torch.tensor([p[2]], dtype=torch.int32, device=DEV)), c0, cs)
           for p, c0, cs in pieces]
    want = sf.vjp_reference(pieces, 30, 48)
    dx = K.slice_vjp(ops, 30, 48)
    assert tuple(dx.shape) == (30, 48) and torch.equal(dx.cpu(), want)
    word = torch.zeros(1, device=DEV)
    assert torch.equal(K.slice_vjp(ops, 30, 48, amax=word), dx) and torch.equal(word, dx.abs().max().reshape(1))
    # more than eight pieces: the result so far is the first piece of a further launch
    from laplace_amd.sweep import SeedBatchedSweep

    many = [ops[1]] + [ops[0]] * 9
    got = SeedBatchedSweep.slice_vjp_launches(K, many, 30, 48)
    ref = sf.vjp_reference([pieces[1]] + [pieces[0]] * 9, 30, 48)
    assert torch.equal(got.cpu(), ref)
    if DEV != "cpu":
        with pytest.raises(LaplaceHipError):
            K.slice_vjp(ops[:1], 30, 10)  # (columns [8, 12) are no slice of 10)
        with pytest.raises(LaplaceHipError):
            K.slice_vjp(many[:9], 30, 48)  # (nine pieces)
        with pytest.raises(LaplaceHipError):
            K.slice_vjp([(ops[1][0], 0, 40)], 30, 48)  # (the tensor holds 48 columns, not 40)
        with pytest.raises(LaplaceHipError):
            K.slice_vjp([(SplitTensor(ops[0][0].planes, torch.zeros(2, dtype=torch.int32, device=DEV)), 8, 4)], 30, 48)
        with pytest.raises(LaplaceHipError, match="chunk-major split tensor is no row matrix"):
            K.slice_vjp([(SplitTensor(ops[0][0].planes, ops[0][0].sexp, chunked=True), 8, 4)], 30, 48)
        with pytest.raises(LaplaceHipError):
            K.slice_forward(x.to(DEV), 30, 48, 40, 9)
        with pytest.raises(LaplaceHipError):
            K.slice_vjp(ops[:1], 30, 48, amax=torch.zeros(2, device=DEV))
        with pytest.raises(LaplaceHipError, match="dst overlaps"):
            xd = x.to(DEV)
            K._rc(K.lib.lk_slice_fwd_f32(xd.data_ptr(), 30, 48, 0, 8, xd.data_ptr(), None), "lk_slice_fwd_f32")


# ---- 2. the small networks -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["csp", "vit"])
def e2e(request):
    """(fp64 CPU model, X, y, seeds, fp64 per-tap inputs and cotangents, oracle Jacobians, factors and predictive variance) -
    computed once per fixture and left unchanged"""
    from tests.norm_sweep_fixtures import autograd_reference

    kind = request.param
    m64, X, y = sf.csp_fixture() if kind == "csp" else sf.vit_fixture()
    seeds = torch.randn(4, X.shape[0], sf.E2E_CLASSES, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    taps = sf.taps(m64)
    f, ins, grads = autograd_reference(m64, taps, X, seeds)
    Js, _ = co.jacobians(m64, X)
    loss, kf = co.kfac_ggn(m64, X, y, X.shape[0], "classification")
    Qs, ls = co.kron_decompose(kf)
    f_var = functional_variance_kron(Js, Qs, ls, 0.5)
    return dict(kind=kind, m64=m64, X=X, y=y, seeds=seeds, f=f.detach(), ins=ins, grads=grads, Js=Js, loss=loss, kf=kf, f_var=f_var)


def test_e2e_taps_of_both_sweeps_against_float64_autograd(e2e):
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep import SeedBatchedSweep
    from laplace_amd.sweep_nhwc import SplitSweep

    for cls in (SplitSweep, SeedBatchedSweep):
        model = copy.deepcopy(e2e["m64"]).float().to(DEV)
        taps = sf.taps(model)
        sw = cls(model, taps, kernels=get_kernels)
        if cls is SplitSweep:  # (the CSP network runs the NHWC walk; the attention node keeps the transformer on the NCHW walk)
            assert sw.split_ok == (e2e["kind"] == "csp"), sw.split_reason
        f = sw.forward(e2e["X"].float().to(DEV))
        grads = sw.backward(e2e["seeds"].float().to(DEV))
        check(f, e2e["f"], what=f"{cls.__name__}: f")
        for n in taps:
            check(sw.taps[n]["a"], e2e["ins"][n], what=f"{cls.__name__}: {n}: a")
            assert tuple(grads[n].shape) == tuple(e2e["grads"][n].shape), n
            check(grads[n], e2e["grads"][n], what=f"{cls.__name__}: {n}: cotangent")


def _factors(kron, kf_ref, what):
    for i, (F_, G_) in enumerate(zip(kron.kfacs, kf_ref)):
        for j, (a, ref) in enumerate(zip(F_, G_)):
            check(a, ref, what=f"{what}: block {i} factor {j}")


def _backend_checks(e2e, what, want_split):
    from laplace_amd import HipGGN
    from laplace_amd.laplace import HipLaplace
    from laplace_amd.sweep_nhwc import SplitSweep

    m64, X, y = e2e["m64"], e2e["X"], e2e["y"]
    model = copy.deepcopy(m64).float().to(DEV)
    Xd, yd = X.float().to(DEV), y.to(DEV)
    b = HipGGN(model, "classification")
    Js, f = b.jacobians(Xd)
    check(f, e2e["f"], what=f"{what}: f")
    check(Js, e2e["Js"], what=f"{what}: jacobians")
    loss, kron = b.kron(Xd, yd, N=X.shape[0])
    tape = b._tape()
    assert not getattr(tape, "sweep_reason", None), tape.sweep_reason
    assert isinstance(tape.sweep, SplitSweep) and tape.sweep.split_ok == want_split, getattr(tape.sweep, "split_reason", None)
    check(loss, e2e["loss"], what=f"{what}: loss")
    _factors(kron, e2e["kf"], f"{what}: kron")
    la = HipLaplace(model, "classification", "all", "kron", prior_precision=0.5)
    la.fit(DataLoader(TensorDataset(Xd, yd), batch_size=X.shape[0]))
    _, f_var = la._glm_predictive_distribution(Xd)
    check(f_var, e2e["f_var"], what=f"{what}: Kron GLM predictive variance")
    return tape.sweep


def test_e2e_jacobians_kron_and_predictive_against_the_oracle(e2e):
    _backend_checks(e2e, e2e["kind"], want_split=e2e["kind"] == "csp")


def test_the_switches_give_the_same_results(e2e, monkeypatch):
    """``SplitSweep.nhwc_slice = False`` (the NCHW sweep with its own SLICE rule on the kernels) and then also
    ``use_slice_kernels = False`` (the torch sequence) against the same oracle at the same tolerance"""
    from laplace_amd.sweep import SeedBatchedSweep
    from laplace_amd.sweep_nhwc import SplitSweep

    monkeypatch.setattr(SplitSweep, "nhwc_slice", False)
    sweep = _backend_checks(e2e, f"{e2e['kind']} (nhwc_slice = False)", want_split=False)
    if e2e["kind"] == "csp":
        assert sweep.split_reason.endswith("has no NHWC rule") and "chunk" in sweep.split_reason
    monkeypatch.setattr(SeedBatchedSweep, "use_slice_kernels", False)
    _backend_checks(e2e, f"{e2e['kind']} (nhwc_slice = False, use_slice_kernels = False)", want_split=False)
