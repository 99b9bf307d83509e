"""lk_syevj_f32 / lk_syevj_batched_f32 on the spectra, sizes and scales KFAC factors have (tests/eig_fixtures.py), on the
MI355X (-m gpu): against the fp64 ``eigvalsh``, each of the eigenvalue error, max|Q^T Q - I| and the reconstruction error
below 5e-6 of lambda_max -- the bound of ``_eig_checks`` in tests/test_gpu_kernels.py, which fp32 LAPACK meets on every one
of these matrices (tests/test_eig_fixtures.py).  Besides the accuracy: ties in the sort, the zero matrix, ``clamp=False``,
the pad-to-64 and 32-wide index-block seams, inputs scaled by 2^-100 ... 2^100, the NaN / inf guard of the load, the status
word of a solve that runs out of sweeps, and the ``M + I`` re-solve of ``HipKronDecomposed`` with the real solver failing.

LK_TEST_DEVICE=cpu runs the bodies against the CPU restatement of the kernels (a self-check of this file on a GPU-less
box); the real run uses the HIP library on cuda:0."""
import os

import pytest
import torch

from tests.eig_fixtures import BOUND, CLAMPED, FAMILIES, SIZES, eig_errors, scaled, spectrum, wishart
from tests.emulated_kernels import EmulatedKernels
from tests.parity_log import record_error

pytestmark = pytest.mark.gpu

DEV = os.environ.get("LK_TEST_DEVICE", "cuda")


@pytest.fixture(scope="module")
def K():
    if DEV == "cpu":
        return EmulatedKernels()
    from laplace_amd._lib import HipKernels

    return HipKernels()


def _sync():
    if DEV != "cpu":
        torch.cuda.synchronize()


def _dev(A64):
    return A64.float().to(DEV).contiguous()


def _solve(K, A64, clamp=True, max_sweeps=0):
    w, Q, info = K.syevj(_dev(A64), clamp=clamp, max_sweeps=max_sweeps)
    _sync()
    return w, Q, info


def _measure(what, A64, w, Q, clamp):
    """the three figures, logged (tests/parity_log.py) and printed before anything is asserted on them"""
    val, orth, rec = (record_error(e) for e in eig_errors(A64, w, Q, clamp=clamp))
    print(f"{what}: val {val:.2e} orth {orth:.2e} rec {rec:.2e}")
    return val, orth, rec


def _assert_solved(what, A64, w, Q, info, clamp):
    val, orth, rec = _measure(what, A64, w, Q, clamp)
    assert int(info[0].item()) == 0, f"{what}: eigensolver did not converge"
    w64 = w.double().cpu()
    assert torch.all(w64[1:] >= w64[:-1]), f"{what}: eigenvalues not ascending"
    assert val < BOUND, f"{what}: eigenvalues off by {val:.2e}"
    assert orth < BOUND, f"{what}: orthogonality {orth:.2e}"
    assert rec < BOUND, f"{what}: reconstruction {rec:.2e}"


# ---- a. families x sizes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family", FAMILIES)
def test_family(K, family, n):
    A64 = spectrum(family, n)
    clamp = CLAMPED[family]
    w, Q, info = _solve(K, A64, clamp=clamp)
    _assert_solved(f"{family} n={n}", A64, w, Q, info, clamp)
    if family == "identity":
        Qc = Q.cpu()
        assert torch.equal(w.cpu(), torch.ones(n)), "identity: every eigenvalue is exactly 1"
        assert torch.all((Qc == 0) | (Qc == 1)) and torch.all(Qc.sum(0) == 1) and torch.all(Qc.sum(1) == 1), \
            "identity: Q is a permutation of I, exactly"
    if family == "zero":
        assert torch.equal(w.cpu(), torch.zeros(n)), "zero: every eigenvalue is exactly 0"
    if family == "indefinite":
        wc, Qc, infoc = _solve(K, A64, clamp=True)
        assert int(infoc[0].item()) == 0
        neg = w < 0
        assert bool(neg.any()) and bool((~neg).any())
        assert torch.all(wc[neg] == 0), "clamp: negative eigenvalues come out as exactly 0"
        assert torch.equal(wc[~neg], w[~neg]) and torch.equal(Qc, Q), "clamp changes nothing else, bit for bit"


# ---- b. scales -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [-100, -60, -30, 30, 60])
@pytest.mark.parametrize("n", [65, 193])
@pytest.mark.parametrize("family", ["spiked", "graded", "dscaled"])
def test_scaled(K, family, n, k):
    """a power-of-two factor is exact in fp32: the same three bounds, normalised by the scaled lambda_max"""
    A64 = scaled(spectrum(family, n), k)
    w, Q, info = _solve(K, A64)
    _assert_solved(f"{family} n={n} x 2^{k}", A64, w, Q, info, True)


# ---- c. the fp32 product a_pp * a_qq overflows ---------------------------------------------------------------------------
def _solved_or_reported(K, what, A64):
    """the contract of the entry point: the three bounds hold, or the call reports that it cannot serve this matrix (a
    negative return code, raised by the binding, or info[0] != 0) -- never info[0] == 0 with a wrong spectrum"""
    from laplace_amd._lib import LaplaceHipError

    assert bool(torch.isfinite(A64.float()).all())
    try:
        w, Q, info = _solve(K, A64)
    except LaplaceHipError as e:
        print(f"{what}: reported by the return code: {e}")
        return "reported"
    val, orth, rec = _measure(what, A64, w, Q, True)
    if int(info[0].item()) != 0:
        print(f"{what}: reported by info[0] = {int(info[0].item())}")
        assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(Q).all())
        return "reported"
    assert val < BOUND, f"{what}: info[0] == 0 with eigenvalues off by {val:.2e}"
    assert orth < BOUND, f"{what}: info[0] == 0 with orthogonality {orth:.2e}"
    assert rec < BOUND, f"{what}: info[0] == 0 with reconstruction {rec:.2e}"
    return "solved"


@pytest.mark.parametrize("k", [70, 100])
def test_entries_whose_products_overflow(K, k):
    """finite fp32 entries of ~2^(k+3): a_pp * a_qq is inf in fp32 (the rotation test of the pivot solve forms it for an
    unscaled matrix), lambda_max ~ 2^(k+9) is an ordinary float"""
    _solved_or_reported(K, f"spiked n=65 x 2^{k}", scaled(spectrum("spiked", 65), k))


@pytest.mark.parametrize("k", [120, -140])
def test_outside_the_supported_range_is_reported(K, k):
    """the edges stated in include/laplace_hip.h: at 2^120 the entries are finite floats but lambda_max ~ 2^129 is not, at
    2^-140 every entry is a denormal of a few bits -- neither spectrum can be written in fp32, and the call says so"""
    assert _solved_or_reported(K, f"spiked n=65 x 2^{k}", scaled(spectrum("spiked", 65), k)) == "reported"


# ---- d. non-finite entries ----------------------------------------------------------------------------------------------
def test_nan_and_inf_are_read_as_zero(K):
    n = 70
    A = wishart(n).float()
    bad = A.clone()
    bad[3, 40] = float("nan")
    bad[10, 55] = float("inf")
    zeroed = A.clone()
    zeroed[3, 40] = 0.0
    zeroed[10, 55] = 0.0
    w, Q, info = K.syevj(bad.to(DEV).contiguous())
    w0, Q0, info0 = K.syevj(zeroed.to(DEV).contiguous())
    _sync()
    assert int(info[0].item()) == 0 and int(info0[0].item()) == 0
    assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(Q).all())
    assert torch.equal(w, w0) and torch.equal(Q, Q0), "the guard of the load: a NaN / inf entry is a 0 entry"
    sym = torch.triu(zeroed) + torch.triu(zeroed, 1).T  # (the lower triangle is never read)
    _assert_solved("wishart n=70 with two entries zeroed", sym.double(), w, Q, info, True)


# ---- e. the status word, from the real solver ------------------------------------------------------------------------------
def test_status_word_of_a_solve_that_runs_out_of_sweeps(K):
    A64 = wishart(130)
    w, Q, info = _solve(K, A64, max_sweeps=1)
    assert int(info[0].item()) == 1 and int(info[1].item()) == 1, "one sweep of a dense matrix: ran out, after 1 sweep"
    assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(Q).all())
    w, Q, info = _solve(K, A64)
    assert int(info[0].item()) == 0 and 1 <= int(info[1].item()) <= 24
    _assert_solved("wishart n=130", A64, w, Q, info, True)


# ---- f. the retry of HipKronDecomposed, with the real solver failing ---------------------------------------------------------
@pytest.mark.skipif(DEV == "cpu", reason="the retry on the emulation is tests/test_eig_convergence.py; this one is about the device")
def test_failed_factor_is_resolved_with_jitter_on_the_device():
    from laplace_amd import _lib
    from laplace_amd.kron import HipKron

    class OneSweepOnce(_lib.HipKernels):
        """the real kernels; the first call that holds a matrix of size `n_bad` gets a single sweep"""

        def __init__(self, n_bad):
            super().__init__()
            self.n_bad, self.tripped, self.calls = n_bad, False, []

        def syevj_batched(self, mats, clamp=True, max_sweeps=0, streams=None):
            if not self.tripped and any(M.shape[0] == self.n_bad for M in mats):
                self.tripped, max_sweeps = True, 1
            self.calls.append(dict(sizes=[M.shape[0] for M in mats], clamp=clamp, max_sweeps=max_sweeps,
                                   cuda=all(M.is_cuda for M in mats)))
            return super().syevj_batched(mats, clamp=clamp, max_sweeps=max_sweeps, streams=streams)

    A64, B64 = wishart(130), wishart(40)
    flaky = OneSweepOnce(130)
    prev = _lib.set_kernels_for_testing(flaky)
    try:
        H = HipKron([[_dev(A64), _dev(B64)], [_dev(A64)]])
        dec = H.decompose()  # never raises: the status words are still on the device
        assert len(flaky.calls) == 1 and flaky.calls[0]["max_sweeps"] == 1, "the status is not read before the first use"
        assert all(int(i[0].item()) == 1 for i in dec._eig_info), "one sweep: every factor of the call ran out"
        post = dec * 2.0 + torch.tensor(0.5, device=DEV)
        got = float(post.logdet())
        retries = flaky.calls[1:]
        assert sorted(c["sizes"][0] for c in retries) == [40, 130, 130] and all(len(c["sizes"]) == 1 for c in retries)
        assert all(c["clamp"] is False and c["max_sweeps"] == 0 and c["cuda"] for c in retries), \
            "the M + I re-solve runs unclamped, with the default sweeps, on the device"
        lA, lB = torch.linalg.eigvalsh(A64), torch.linalg.eigvalsh(B64)
        for name, l, ref in (("A", dec.eigenvalues[0][0], lA), ("B", dec.eigenvalues[0][1], lB), ("A alone", dec.eigenvalues[1][0], lA)):
            err = record_error((torch.sort(l.double().cpu())[0] - ref).abs().max().item() / ref.max().item())
            print(f"re-solved factor {name}: eigenvalues off by {err:.2e}")
            assert err < BOUND, f"re-solved factor {name}: eigenvalues off by {err:.2e}"
        want = float(torch.log(2.0 * torch.outer(lA, lB) + 0.5).sum() + torch.log(2.0 * lA + 0.5).sum())
        err = record_error(abs(got - want) / abs(want))
        print(f"logdet {got:.6f} (fp64 {want:.6f}): rel {err:.2e}")
        assert err < 1e-5
        assert len(flaky.calls) == 4, "re-solved once, at the first use"
    finally:
        _lib.set_kernels_for_testing(prev)


# ---- g. a mixed batch ---------------------------------------------------------------------------------------------------
def test_mixed_batch(K):
    """one scheduled call on two streams over matrices that converge after different numbers of sweeps, at scales 2^80
    apart: each within the bounds, and bit for bit what its own single solve returns"""
    mats64 = [("spiked n=193 x 2^-40", scaled(spectrum("spiked", 193), -40)), ("graded n=129 x 2^40", scaled(spectrum("graded", 129), 40)),
              ("zero n=33", spectrum("zero", 33)), ("identity n=63", spectrum("identity", 63)), ("pairs n=65", spectrum("pairs", 65)),
              ("wishart n=257", wishart(257))]
    mats = [_dev(A64) for _, A64 in mats64]
    streams = [torch.cuda.Stream() for _ in range(2)] if DEV != "cpu" else None
    outs = K.syevj_batched(mats, clamp=True, streams=streams)
    if streams:
        for st in streams:
            torch.cuda.current_stream().wait_stream(st)
    _sync()
    assert len(outs) == len(mats)
    for (what, A64), M, (w, Q, info) in zip(mats64, mats, outs):
        _assert_solved(f"batched {what}", A64, w, Q, info, True)
        w1, Q1, _ = K.syevj(M)
        _sync()
        assert torch.equal(w1, w) and torch.equal(Q1, Q), f"{what}: the batched solve differs from the single one"
