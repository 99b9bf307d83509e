"""The product rule of the seed-batched reverse sweep on the device (-m gpu): the kernel alone (csrc/lk_mul.hip through the C ABI)
against the fp64 reference computed on the CPU from the same inputs, and a small SEResNetSmall and ViTSwiGLU through
``SeedBatchedSweep``, ``HipGGN`` and the Kron GLM predictive against float64 autograd and the oracle.

Kernel level.  The shape table is tests/mul_fixtures.CASES (tests/test_mul_fixtures.py proves on the CPU that it reaches every launch
path and that the criteria tell four wrong kernels from the right one).  ``da``, and ``db`` of the full form, are ``torch.equal`` to
the fp32 product - one rounding, no tolerance; ``db`` of a row gate lies within ``(L + 1) 2^-24 sum_l |g a|`` of the exact sum (fp64),
the bound of a sum of L products in any order, fused or not (gamma_L <= (L + 1) u for L <= 4096, which every case respects).  The
outputs start as NaN (the kernel owes every element) inside guard bands of NaN / ``-0.0`` that keep their bits; a second equal call
gives the same bits; with one output null the other keeps its bits.

End to end: tests/mul_fixtures.se_fixture (widths 8 / 16, 8 x 8 inputs, B = 4, tanh) and swiglu_fixture (dim 32, T = 5, B = 3) at the
project's 1e-4 relative per block, as tests/test_gpu_cat.py and tests/test_gpu_slice.py.  ``LK_TEST_DEVICE=cpu`` rehearses this
file's host logic on the kernel emulation.
"""
import copy
import ctypes
import os

import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from oracle import curvature_oracle as co
from tests import mul_fixtures as mf
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
    from tests.emulated_mul_kernels import EmulatedMulKernels

    prev = _lib.set_kernels_for_testing(EmulatedMulKernels())
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


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------
class _Banded:
    """``numel`` fp32 elements inside guard bands of ``PAD`` elements filled with ``fill`` (NaN or -0.0: compared by bit pattern);
    ``off``: the interior starts one element (4 bytes) past a 16-byte aligned address; the interior starts as NaN unless ``init`` is
    given"""

    def __init__(self, shape, off, init=None, fill=float("nan")):
        n = 1
        for d in shape:
            n *= d
        self.buf = torch.full((2 * PAD + n + 8,), fill, dtype=torch.float32, device=DEV)
        self.lo, self.hi = PAD + off, PAD + off + n
        self.t = self.buf[self.lo:self.hi].view(*shape)
        if n:
            self.t.fill_(float("nan"))
        self.bands = torch.cat([self.buf[:self.lo], self.buf[self.hi:]]).view(torch.int32).clone()
        if init is not None and n:
            self.t.copy_(init)

    def ptr(self):
        """address of the interior (of the allocation plus the offset: an empty view reports a null data_ptr)"""
        return ctypes.c_void_p(self.buf.data_ptr() + self.lo * 4)

    def bands_intact(self):
        return torch.equal(torch.cat([self.buf[:self.lo], self.buf[self.hi:]]).view(torch.int32), self.bands)


def _call(c, g, a, b, da, db):
    """one call of lk_mul_vjp_f32 on banded buffers (``da`` / ``db``: a ``_Banded`` or ``None``)"""
    from laplace_amd._lib import get_kernels

    K, S, R, L = get_kernels(), c["S"], c["R"], c["L"]
    if DEV == "cpu":
        if R:
            got = K.mul_vjp(g.t.reshape(S * R, L).contiguous(), a.t.contiguous(), b.t.contiguous(), S, c["row"],
                            (da is not None, db is not None))
            for dst, val in zip((da, db), got):
                if dst is not None:
                    dst.t.copy_(val.reshape(dst.t.shape))
        return
    rc = K.lib.lk_mul_vjp_f32(g.ptr(), a.ptr(), b.ptr(), S, R, L, int(c["row"]), None if da is None else da.ptr(),
                              None if db is None else db.ptr(), K._stream(g.buf.device))
    assert rc == 0, K.lib.lk_last_error()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("c", [c for c in mf.CASES if not c["wide"]], ids=mf.case_id)
def test_kernel_against_the_float64_reference(c):
    gen = torch.Generator().manual_seed(7 + mf.CASES.index(c))
    S, R, L, off, row = c["S"], c["R"], c["L"], c["off"], c["row"]
    g, a, b = mf.make_inputs(c, gen)
    ref = mf.vjp_reference(g, a, b, row)
    want_da, want_db = mf.wants(c)
    dg, da_in, db_in = _Banded((S, R, L), off, init=g, fill=-0.0), _Banded((R, L), off, init=a), _Banded(b.shape, off, init=b, fill=-0.0)
    db_shape = (S, R) if row else (S, R, L)

    def run(with_da, with_db):
        da = _Banded((S, R, L), off) if with_da else None
        db = _Banded(db_shape, off, fill=-0.0) if with_db else None
        _call(c, dg, da_in, db_in, da, db)
        for name, o in (("da", da), ("db", db)):
            if o is not None:
                assert o.bands_intact(), f"{name}: written outside its extent"
                assert bool(torch.isfinite(o.t).all()), f"{name}: an element was not written"
        return da, db

    da, db = run(want_da, want_db)
    bad = mf.violations(c, None if da is None else da.t, None if db is None else db.t, ref)
    assert not bad, bad
    da2, db2 = run(want_da, want_db)
    for name, x, y in (("da", da, da2), ("db", db, db2)):
        assert x is None or torch.equal(_bits(x.buf), _bits(y.buf)), f"{name}: two equal calls differ"
    if want_da and want_db:  # with one output null the other keeps its bits
        da3, none = run(True, False)
        none, db3 = run(False, True)
        assert torch.equal(_bits(da.buf), _bits(da3.buf)), "da changes when db is null"
        assert torch.equal(_bits(db.buf), _bits(db3.buf)), "db changes when da is null"
    assert dg.bands_intact() and da_in.bands_intact() and db_in.bands_intact()
    assert torch.equal(_bits(dg.t.cpu()), _bits(g)) and torch.equal(_bits(da_in.t.cpu()), _bits(a))  # (the inputs are as they were)


def test_the_bindings():
    """the Python bindings allocate what the C ABI takes, shape the outputs as the sweep wants them and refuse what does not belong
    together"""
    from laplace_amd._lib import LaplaceHipError, get_kernels

    K = get_kernels()
    gen = torch.Generator().manual_seed(4)
    S, B = 3, 2
    a, gate = mf.full_mantissa((B, 6, 5, 5), gen), mf.full_mantissa((B, 6, 1, 1), gen)
    g = mf.full_mantissa((S * B, 6, 5, 5), gen)
    c = dict(row=True, S=S, R=B * 6, L=25, want="both")
    ref = mf.vjp_reference(g.reshape(S, B * 6, 25), a.reshape(B * 6, 25), gate.reshape(B * 6), True)
    da, db = K.mul_vjp(g.to(DEV), a.to(DEV), gate.to(DEV), S, True)
    assert tuple(da.shape) == (S * B, 6, 5, 5) and tuple(db.shape) == (S * B, 6, 1, 1)
    assert mf.violations(c, da, db, ref) == []
    only, none = K.mul_vjp(g.to(DEV), a.to(DEV), gate.to(DEV), S, True, want=(True, False))
    assert none is None and torch.equal(only, da)
    b = mf.full_mantissa((B, 6, 5, 5), gen)
    c = dict(row=False, S=S, R=B, L=150, want="both")
    ref = mf.vjp_reference(g.reshape(S, B, 150), a.reshape(B, 150), b.reshape(B, 150), False)
    da, db = K.mul_vjp(g.to(DEV), a.to(DEV), b.to(DEV), S, False)
    assert tuple(da.shape) == tuple(db.shape) == (S * B, 6, 5, 5) and mf.violations(c, da, db, ref) == []
    if DEV != "cpu":
        gd, ad, bd = g.to(DEV), a.to(DEV), b.to(DEV)
        with pytest.raises(LaplaceHipError, match="do not belong together"):
            K.mul_vjp(gd, ad, bd, S + 1, False)
        with pytest.raises(LaplaceHipError, match="do not belong together"):
            K.mul_vjp(gd, ad, bd[:, :3].contiguous(), S, False)
        with pytest.raises(LaplaceHipError, match="do not belong together"):
            K.mul_vjp(gd, ad, bd, S, False, want=(False, False))
        with pytest.raises(LaplaceHipError, match="contiguous"):
            K.mul_vjp(gd, ad.transpose(2, 3), bd, S, False)
        with pytest.raises(LaplaceHipError, match="an output overlaps an input"):
            K._rc(K.lib.lk_mul_vjp_f32(gd.data_ptr(), ad.data_ptr(), bd.data_ptr(), S, B, 150, 0, gd.data_ptr(), None, None), "lk_mul_vjp_f32")


# ---- 2. the small networks -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["se", "swiglu"])
def e2e(request):
    """(fp64 CPU model, X, y, seeds, fp64 per-tap inputs and cotangents, oracle Jacobians, factors and predictive variance) -
    computed once per fixture and left unchanged"""
    from tests.norm_sweep_fixtures import autograd_reference

    kind = request.param
    m64, X, y = mf.se_fixture() if kind == "se" else mf.swiglu_fixture()
    seeds = torch.randn(4, X.shape[0], mf.E2E_CLASSES, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    taps = mf.taps(m64)
    f, ins, grads = autograd_reference(m64, taps, X, seeds)
    Js, _ = co.jacobians(m64, X)
    Hl = co.functional_hessian(f.detach(), "classification")
    loss, kf = co.kfac_ggn(m64, X, y, X.shape[0], "classification")
    Qs, ls = co.kron_decompose(kf)
    f_var = functional_variance_kron(Js, Qs, ls, 0.5)
    return dict(kind=kind, m64=m64, X=X, y=y, seeds=seeds, f=f.detach(), ins=ins, grads=grads, Js=Js, diag=co.ggn_diag(Js, Hl), loss=loss,
                kf=kf, f_var=f_var)


def test_e2e_taps_of_the_sweep_against_float64_autograd(e2e):
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep import SeedBatchedSweep
    from laplace_amd.sweep_nhwc import SplitSweep

    for cls in (SplitSweep, SeedBatchedSweep):  # (the split sweep names the product / the attention node and runs the NCHW walk)
        model = copy.deepcopy(e2e["m64"]).float().to(DEV)
        taps = mf.taps(model)
        sw = cls(model, taps, kernels=get_kernels)
        if cls is SplitSweep:
            assert not sw.split_ok and sw.split_reason.endswith("has no NHWC rule"), sw.split_reason
            assert e2e["kind"] != "se" or sw.split_reason == "mul has no NHWC rule"
        f = sw.forward(e2e["X"].float().to(DEV))
        grads = sw.backward(e2e["seeds"].float().to(DEV))
        check(f, e2e["f"], what=f"{cls.__name__}: f")
        for n in taps:
            check(sw.taps[n]["a"], e2e["ins"][n], what=f"{cls.__name__}: {n}: a")
            assert tuple(grads[n].shape) == tuple(e2e["grads"][n].shape), n
            check(grads[n], e2e["grads"][n], what=f"{cls.__name__}: {n}: cotangent")


def _backend_checks(e2e, what):
    from laplace_amd import HipGGN
    from laplace_amd.laplace import HipLaplace
    from laplace_amd.sweep import SeedBatchedSweep

    m64, X, y = e2e["m64"], e2e["X"], e2e["y"]
    model = copy.deepcopy(m64).float().to(DEV)
    Xd, yd = X.float().to(DEV), y.to(DEV)
    b = HipGGN(model, "classification")
    Js, f = b.jacobians(Xd)
    check(f, e2e["f"], what=f"{what}: f")
    check(Js, e2e["Js"], what=f"{what}: jacobians")
    _, h = b.diag(Xd, yd)
    check(h, e2e["diag"], what=f"{what}: diag")
    loss, kron = b.kron(Xd, yd, N=X.shape[0])
    tape = b._tape()
    assert getattr(tape, "sweep_reason", None) is None, tape.sweep_reason
    assert isinstance(tape.sweep, SeedBatchedSweep) and not getattr(tape.sweep, "split_ok", False)
    check(loss, e2e["loss"], what=f"{what}: loss")
    for i, (F_, G_) in enumerate(zip(kron.kfacs, e2e["kf"])):
        for j, (got, ref) in enumerate(zip(F_, G_)):
            check(got, ref, what=f"{what}: kron: block {i} factor {j}")
    la = HipLaplace(model, "classification", "all", "kron", prior_precision=0.5)
    la.fit(DataLoader(TensorDataset(Xd, yd), batch_size=X.shape[0]))
    _, f_var = la._glm_predictive_distribution(Xd)
    check(f_var, e2e["f_var"], what=f"{what}: Kron GLM predictive variance")


def test_e2e_jacobians_diag_kron_and_predictive_against_the_oracle(e2e):
    _backend_checks(e2e, e2e["kind"])


def test_the_switch_gives_the_same_results(e2e, monkeypatch):
    """``use_mul_kernels = False`` (the torch math of the rule) against the same oracle at the same tolerance"""
    from laplace_amd.sweep import SeedBatchedSweep

    monkeypatch.setattr(SeedBatchedSweep, "use_mul_kernels", False)
    _backend_checks(e2e, f"{e2e['kind']} (use_mul_kernels = False)")
