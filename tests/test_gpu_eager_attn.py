"""Hand-written attention in the seed-batched reverse sweep on the device (-m gpu): the two kernels alone (csrc/lk_softmax.hip and
csrc/lk_matmul.hip through the C ABI) against fp64 references computed on the CPU from the same inputs, and a small ViTEager
through ``SeedBatchedSweep``, ``HipGGN`` and the Kron GLM predictive against float64 autograd and the oracle.

Kernel level.  The shape tables are tests/eager_attn_fixtures.SOFTMAX_CASES / MATMUL_CASES (tests/test_eager_attn_fixtures.py
proves on the CPU that they reach every launch path and that the criteria accept every summation order and tell five wrong kernels
from the right one).  The criteria are the order-free rounding bounds derived in that file's docstring: a matmul element within
``(depth + 1) 2^-24 sum|x||y|`` of the exact dot product and bit-equal on small integers; a softmax element within
``2^-24 |y| ((L + 4) sum|g y| + 3 |g|)`` (exactly zero where the probability is zero), a log-softmax element within
``2^-24 (exp(y) sum|g| (L + C_EXP + 4) + 2 |g|)`` with the device ``expf`` term ``C_EXP = 2.06`` (twice the CPU's measured fp32
``exp`` error).  The outputs start as NaN (the kernel owes every element) inside guard bands of NaN / ``-0.0`` that keep their bits; a
second equal call gives the same bits; with one output null the other keeps its bits; ``off`` cases start 4 bytes past alignment.

End to end: tests/eager_attn_fixtures.vit_eager_fixture (dim 32, 2 heads, T = 5 and T = 17, B = 3, with and without the
relative-position bias, GELU) at the project's 1e-4 relative per block, with the kernels on and with both switches off.
``LK_TEST_DEVICE=cpu`` rehearses this file's host logic on the kernel emulations.
"""
import copy
import ctypes
import os

import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from oracle import curvature_oracle as co
from tests import eager_attn_fixtures as ef
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
    from tests.emulated_matmul_kernels import EmulatedEagerAttnKernels

    prev = _lib.set_kernels_for_testing(EmulatedEagerAttnKernels())
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


# ---- 1. the kernels alone ----------------------------------------------------------------------------------------------------------
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


def _bits(t):
    return t.contiguous().view(torch.int32)


def _written(name, o):
    assert o.bands_intact(), f"{name}: written outside its extent"
    assert bool(torch.isfinite(o.t).all()), f"{name}: an element was not written"


SMX = [i for i, c in enumerate(ef.SOFTMAX_CASES) if not c["wide"]]
MM = [i for i, c in enumerate(ef.MATMUL_CASES) if not c["wide"]]


@pytest.mark.parametrize("i", SMX, ids=lambda i: ef.softmax_case_id(ef.SOFTMAX_CASES[i]))
def test_softmax_kernel_against_the_float64_reference(i):
    from laplace_amd._lib import get_kernels

    K, c = get_kernels(), ef.SOFTMAX_CASES[i]
    S, R, L, off, log = c["S"], c["R"], c["L"], c["off"], c["log"]
    g, y = ef.softmax_case_inputs(i)
    ref = ef.softmax_reference(g, y, log)
    dg, dy = _Banded((S, R, L), off, init=g, fill=-0.0), _Banded((R, L), off, init=y)

    def run():
        dx = _Banded((S, R, L), off, fill=-0.0)
        if DEV == "cpu":
            if R:
                dx.t.copy_(K.softmax_vjp(dg.t.reshape(S * R, L).contiguous(), dy.t.contiguous(), S, log).reshape(S, R, L))
        else:
            rc = K.lib.lk_softmax_vjp_f32(dg.ptr(), dy.ptr(), S, R, L, int(log), dx.ptr(), K._stream(dg.buf.device))
            assert rc == 0, K.lib.lk_last_error()
        _written("dx", dx)
        return dx

    dx = run()
    bad = ef.softmax_violations(c, dx.t, ref)
    assert not bad, bad
    if c["kind"] != "random" and not log:  # a masked key: an exact zero, whatever the cotangent
        assert bool((dx.t.cpu()[:, y == 0] == 0).all())
    assert torch.equal(_bits(dx.buf), _bits(run().buf)), "dx: two equal calls differ"
    assert dg.bands_intact() and dy.bands_intact()
    assert torch.equal(_bits(dg.t.cpu()), _bits(g)) and torch.equal(_bits(dy.t.cpu()), _bits(y))  # (the inputs are as they were)


@pytest.mark.parametrize("ints", (False, True), ids=("mantissa", "integers"))
@pytest.mark.parametrize("i", MM, ids=lambda i: ef.matmul_case_id(ef.MATMUL_CASES[i]))
def test_matmul_kernel_against_the_float64_reference(i, ints):
    from laplace_amd._lib import get_kernels

    K, c = get_kernels(), ef.MATMUL_CASES[i]
    S, NB, M, Kd, N = c["S"], c["NB"], c["M"], c["K"], c["N"]
    off = i % 2  # (4-byte accesses only: every other case starts 4 bytes past a 16-byte aligned address)
    g, a, b = ef.matmul_case_inputs(i, ints)
    ref = ef.matmul_reference(g, a, b)
    want_da, want_db = ef.matmul_wants(c)
    dg, da_in, db_in = _Banded((S, NB, M, N), off, init=g, fill=-0.0), _Banded((NB, M, Kd), off, init=a), _Banded((NB, Kd, N), off, init=b, fill=-0.0)

    def run(with_da, with_db):
        da = _Banded((S, NB, M, Kd), off) if with_da else None
        db = _Banded((S, NB, Kd, N), off, fill=-0.0) if with_db else None
        if DEV == "cpu":
            if NB:
                got = K.matmul_vjp(dg.t.reshape(S * NB, M, N).contiguous(), da_in.t.contiguous(), db_in.t.contiguous(), S, (with_da, with_db))
                for dst, val in zip((da, db), got):
                    if dst is not None:
                        dst.t.copy_(val.reshape(dst.t.shape))
        else:
            rc = K.lib.lk_matmul_vjp_f32(dg.ptr(), da_in.ptr(), db_in.ptr(), S, NB, M, Kd, N, None if da is None else da.ptr(),
                                         None if db is None else db.ptr(), K._stream(dg.buf.device))
            assert rc == 0, K.lib.lk_last_error()
        for name, o in (("da", da), ("db", db)):
            if o is not None:
                _written(name, o)
        return da, db

    da, db = run(want_da, want_db)
    bad = ef.matmul_violations(c, None if da is None else da.t, None if db is None else db.t, ref, ints)
    assert not bad, bad
    da2, db2 = run(want_da, want_db)
    for name, x, y in (("da", da, da2), ("db", db, db2)):
        assert x is None or torch.equal(_bits(x.buf), _bits(y.buf)), f"{name}: two equal calls differ"
    if want_da and want_db:  # with one output null the other keeps its bits
        da3, _ = run(True, False)
        _, db3 = run(False, True)
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
    S, B, H, T, D = 3, 2, 2, 5, 4
    q, kt = ef.full_mantissa((B, H, T, D), gen), ef.full_mantissa((B, H, D, T), gen)
    g = ef.full_mantissa((S * B, H, T, T), gen)
    c = dict(S=S, NB=B * H, M=T, K=D, N=T, want="both")
    ref = ef.matmul_reference(g.reshape(S, B * H, T, T), q.reshape(B * H, T, D), kt.reshape(B * H, D, T))
    da, db = K.matmul_vjp(g.to(DEV), q.to(DEV), kt.to(DEV), S)
    assert tuple(da.shape) == (S * B, H, T, D) and tuple(db.shape) == (S * B, H, D, T)
    assert ef.matmul_violations(c, da, db, ref) == []
    only, none = K.matmul_vjp(g.to(DEV), q.to(DEV), kt.to(DEV), S, want=(True, False))
    assert none is None and torch.equal(only, da)
    y = torch.softmax(torch.randn(B, H, T, T, generator=gen, dtype=torch.float64), -1).float()
    dx = K.softmax_vjp(g.to(DEV), y.to(DEV), S)
    assert tuple(dx.shape) == tuple(g.shape)
    cs = dict(S=S, R=B * H * T, L=T, log=False)
    assert ef.softmax_violations(cs, dx, ef.softmax_reference(g.reshape(S, -1, T), y.reshape(-1, T), False)) == []
    if DEV != "cpu":
        gd, qd, kd, yd = g.to(DEV), q.to(DEV), kt.to(DEV), y.to(DEV)
        with pytest.raises(LaplaceHipError, match="do not belong together"):
            K.matmul_vjp(gd, qd, kd, S + 1)
        with pytest.raises(LaplaceHipError, match="do not belong together"):
            K.matmul_vjp(gd, qd, kd[..., :3].contiguous(), S)
        with pytest.raises(LaplaceHipError, match="do not belong together"):
            K.matmul_vjp(gd, qd, kd, S, want=(False, False))
        with pytest.raises(LaplaceHipError, match="contiguous"):
            K.matmul_vjp(gd, qd, qd.transpose(-1, -2), S)
        with pytest.raises(LaplaceHipError, match="do not belong together"):
            K.softmax_vjp(gd, yd, S + 1)
        with pytest.raises(LaplaceHipError, match="dx overlaps an input"):
            K._rc(K.lib.lk_softmax_vjp_f32(gd.data_ptr(), yd.data_ptr(), S, B * H * T, T, 0, gd.data_ptr(), None), "lk_softmax_vjp_f32")
        with pytest.raises(LaplaceHipError, match="an output overlaps an input"):
            K._rc(K.lib.lk_matmul_vjp_f32(gd.data_ptr(), qd.data_ptr(), kd.data_ptr(), S, B * H, T, D, T, gd.data_ptr(), None, None),
                  "lk_matmul_vjp_f32")


# ---- 2. the small transformer ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(5, True), (5, False), (17, True), (17, False)], ids=lambda p: f"T{p[0]}-{'bias' if p[1] else 'plain'}")
def e2e(request):
    """(fp64 CPU model, X, y, seeds, fp64 per-tap inputs and cotangents, oracle Jacobians, factors and predictive variance) -
    computed once per fixture and left unchanged"""
    from tests.norm_sweep_fixtures import autograd_reference

    T, bias = request.param
    m64, X, y = ef.vit_eager_fixture(T=T, rel_bias=bias, softmax_module=bias)  # (both spellings of the softmax)
    seeds = torch.randn(4, X.shape[0], ef.E2E_CLASSES, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    taps = ef.taps(m64)
    f, ins, grads = autograd_reference(m64, taps, X, seeds)
    Js, _ = co.jacobians(m64, X)
    Hl = co.functional_hessian(f.detach(), "classification")
    loss, kf = co.kfac_ggn(m64, X, y, X.shape[0], "classification")
    Qs, ls = co.kron_decompose(kf)
    f_var = functional_variance_kron(Js, Qs, ls, 0.5)
    return dict(kind=f"T{T}-{'bias' if bias else 'plain'}", m64=m64, X=X, y=y, seeds=seeds, f=f.detach(), ins=ins, grads=grads, Js=Js,
                diag=co.ggn_diag(Js, Hl), loss=loss, kf=kf, f_var=f_var)


def _switches(monkeypatch, on):
    from laplace_amd.sweep import SeedBatchedSweep

    monkeypatch.setattr(SeedBatchedSweep, "use_matmul_kernels", on)
    monkeypatch.setattr(SeedBatchedSweep, "use_softmax_kernels", on)


@pytest.mark.parametrize("on", (True, False), ids=("kernels", "torch-math"))
def test_e2e_taps_of_the_sweep_against_float64_autograd(e2e, on, monkeypatch):
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep import SeedBatchedSweep
    from laplace_amd.sweep_nhwc import SplitSweep

    _switches(monkeypatch, on)
    for cls in (SplitSweep, SeedBatchedSweep):  # (the split sweep names the matrix product and runs the NCHW walk)
        model = copy.deepcopy(e2e["m64"]).float().to(DEV)
        taps = ef.taps(model)
        sw = cls(model, taps, kernels=get_kernels)
        if cls is SplitSweep:
            assert not sw.split_ok and sw.split_reason == "matmul has no NHWC rule", sw.split_reason
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
    assert getattr(tape, "sweep_reason", None) is None, tape.sweep_reason  # (a sweep, not the tape, produced the result)
    assert isinstance(tape.sweep, SeedBatchedSweep) and not getattr(tape.sweep, "split_ok", False)
    check(loss, e2e["loss"], what=f"{what}: loss")
    for i, (F_, G_) in enumerate(zip(kron.kfacs, e2e["kf"])):
        for j, (got, ref) in enumerate(zip(F_, G_)):
            check(got, ref, what=f"{what}: kron: block {i} factor {j}")
    la = HipLaplace(model, "classification", "all", "kron", prior_precision=0.5)
    la.fit(DataLoader(TensorDataset(Xd, yd), batch_size=X.shape[0]))
    _, f_var = la._glm_predictive_distribution(Xd)
    check(f_var, e2e["f_var"], what=f"{what}: Kron GLM predictive variance")


@pytest.mark.parametrize("on", (True, False), ids=("kernels", "torch-math"))
def test_e2e_jacobians_diag_kron_and_predictive_against_the_oracle(e2e, on, monkeypatch):
    _switches(monkeypatch, on)
    _backend_checks(e2e, f"{e2e['kind']} ({'kernels' if on else 'both switches off'})")
