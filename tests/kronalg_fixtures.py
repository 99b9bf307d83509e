"""The eigenvalue algebra of the Kron posterior on the spectra KFAC factors really have: cases, fp64 references, metrics and
the checks themselves for ``kron_pow``, ``kron_logdet``, ``kron_logdet_blocks``, ``kron_sandwich`` and the quadratic forms of
the GLM predictive (csrc/lk_kron.hip, lk_gemm.hip, lk_grid.hip, and the weight-sharing forms).

TEST INFRASTRUCTURE, in the style of tests/eig_fixtures.py.  Each ``check_*`` takes a kernels object and a ``dev`` function
that places an fp64 tensor where those kernels read it, runs every case and returns the worst figure per metric:
tests/test_kronalg_fixtures.py passes :class:`Fp32Kernels` (a plain torch-float32 evaluation of the same formulas, on the
CPU) and pins that every case meets its bound there; tests/test_gpu_kron_spectra.py passes the HIP library and asks the
same.  Every input is an fp64 number that fp32 holds exactly, so both read what the fp64 reference reads.

Eigenvalues come from tests/eig_fixtures.py: ``eigvalsh(spectrum(family, n)).clamp(min=0) * 2^k`` -- graded over many
decades, one eigenvalue n times the bulk, rank 1 and rank 0 (exact zeros, as ``Kron.decompose`` hands them over), a common
factor of 2^-20 or 2^16 -- and ``delta`` spans the prior search's 1e-4 ... 1e4.
"""
from __future__ import annotations

from functools import lru_cache

import torch

from tests.eig_fixtures import orthogonal, scaled, spectrum
from tests.emulated_kernels import EmulatedKernels
from tests.lik_fixtures import sample_err
from tests.test_prior_grid import GridKernels

FAMILIES = ("spiked", "graded", "dscaled", "pairs", "identity", "ones", "zero")
SCALES = (-20, 0, 16)
SIZES = ((1, 0), (33, 0), (2, 65), (64, 193), (129, 257))
DELTAS = (1e-4, 1.0, 1e4)
EXPONENTS = (-1.0, -0.5, 1.0, 0.5)

#: existing ``test_kron_logdet*`` of tests/test_gpu_kernels.py
BOUND_POW = BOUND_LOGDET = 1e-5
#: "within 1e-4 rel fp32" of BASELINE.json, as ``test_quadforms`` and ``test_quadform_shared`` use it -- here per sample
BOUND_QUAD = 1e-4
#: tests/test_gpu_prior_grid.py, element-wise
BOUND_GRID = 1e-5
#: ``_bmm``'s bound in tests/test_gpu_kron_algebra.py -- here per row of W
BOUND_SANDWICH = 1e-4

REF = EmulatedKernels()  # on fp64 tensors: the reference
GREF = GridKernels()


def f32(t):
    """round to what fp32 holds, keep fp64"""
    return t.float().double()


@lru_cache(maxsize=None)
def eigs(family: str, n: int, k: int = 0) -> torch.Tensor:
    lam = torch.linalg.eigvalsh(spectrum(family, n)).clamp(min=0)
    # (the fp64 solve leaves ~1e-16 lambda_max where a rank-deficient factor has exact zeros; scaled by 2^-20 some of it would
    #  be an fp32 denormal.  An exact zero is what the clamped device solve hands over.)
    lam = torch.where(lam < 1e-13 * lam.max(), torch.zeros_like(lam), lam)
    return f32(scaled(lam, k))


def delta_t(d: float) -> torch.Tensor:
    return f32(torch.tensor([d], dtype=torch.float64))


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def partner(family: str) -> str:
    """the family of the second factor: the next one, so that a rank-0 or rank-1 factor meets a full-rank one as well"""
    return FAMILIES[(FAMILIES.index(family) + 3) % len(FAMILIES)]


def factors(family: str, n1: int, n2: int, k: int, mixed: bool = False):
    l1 = eigs(family, n1, k)
    l2 = eigs(partner(family) if mixed else family, n2, k) if n2 else None
    return l1, l2


# ---- metrics -------------------------------------------------------------------------------------------------------------
def elem_err(got, want) -> float:
    """element-wise relative error of entries that are sums of positive terms; an expected exact zero must come back as an
    exact zero (inf otherwise); NaN in ``got`` is NaN"""
    got, want = got.detach().double().cpu().reshape(-1), want.detach().double().cpu().reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    if bool(torch.isnan(got).any()):
        return float("nan")
    if got.numel() == 0:
        return 0.0
    nz = want != 0
    rel = torch.where(nz, (got - want).abs() / torch.where(nz, want.abs(), torch.ones_like(want)),
                      torch.where(got != 0, torch.full_like(want, float("inf")), torch.zeros_like(want)))
    return rel.max().item()


#: Rounding v = l1 l2 + delta to fp32 moves log v by up to 2^-24 in ABSOLUTE terms whatever the kernel does, so a table whose
#: logs are all ~0 (delta = 1 on top of eigenvalues of 2^-20, say: v = 1 + 1e-5) cannot be summed to 1e-5 of sum |log v| in
#: fp32.  The value is measured where the mean |log v| is at least this (the rounding is then below 2e-6 of the sum); a table
#: whose logs are all exactly 0 must give exactly 0; the rest only have their derivatives checked.
MIN_MEAN_ABS_LOG = 0.05


def logdet_err(got, want: float, abs_logs: float, count: int):
    """|got - want| / sum |log v|: the logs have both signs at delta = 1e-4 and their sum can cancel.  None where fp32
    cannot resolve the sum (see ``MIN_MEAN_ABS_LOG``)."""
    if abs_logs == 0.0:
        return 0.0 if float(got) == 0.0 else float("inf")
    if abs_logs < MIN_MEAN_ABS_LOG * count:
        return None
    return abs(float(got) - want) / abs_logs


class Worst(dict):
    """worst figure per metric name"""

    def see(self, name: str, value):
        if value is None:  # not measurable in fp32 (logdet_err)
            return None
        prev = self.get(name, 0.0)
        self[name] = prev if prev != prev else (value if value != value else max(prev, value))
        return value


# ---- a plain fp32 evaluation ----------------------------------------------------------------------------------------------
class Fp32Kernels(GridKernels):
    """the emulation's formulas on float32 tensors; the two logdets sum each row of the eigenvalue outer product in fp32
    and reduce the rows in fp64, as the kernels do"""

    def kron_logdet(self, l1, l2, delta, damping=False, want_grads=False):
        d = delta.reshape(())
        if l2 is None:
            M = (l1 + d).reshape(-1, 1)
        elif damping:
            sd = d.sqrt()
            M = torch.outer(l1 + sd, l2 + sd)
        else:
            M = torch.outer(l1, l2) + d
        out = torch.log(M).sum(1).double().sum().float().reshape(1)
        if not want_grads:
            return out, None, None, None
        inv = 1.0 / M
        dd = inv.sum(1).double().sum().float().reshape(1)
        if l2 is None:
            return out, inv.reshape(-1), None, dd
        return out, (inv * l2.view(1, -1)).sum(1), (inv * l1.view(-1, 1)).sum(0), dd

    def kron_logdet_blocks(self, blocks, deltas, scale=None, want_grads=False):
        s = torch.ones(()) if scale is None else scale.reshape(())
        out = torch.zeros((), dtype=torch.float64)
        dd, ds = [], torch.zeros((), dtype=torch.float64)
        for ls, d in zip(blocks, deltas):
            lam = ls[0].reshape(-1, 1) if len(ls) == 1 else torch.outer(ls[0], ls[1])
            M = s * lam + d
            inv = 1.0 / M
            out = out + torch.log(M).sum(1).double().sum()
            dd.append(inv.sum(1).double().sum().float())
            ds = ds + (lam * inv).sum(1).double().sum()
        return (out.float().reshape(1), torch.stack(dd) if want_grads else None,
                ds.float().reshape(1) if want_grads and scale is not None else None)


def cpu_f32(t64):
    return t64.float()


# ---- kron_pow ---------------------------------------------------------------------------------------------------------------
def check_pow(K, dev, family: str, n1: int, n2: int) -> Worst:
    w = Worst()
    for k in SCALES:
        for mixed in ((False, True) if n2 else (False,)):
            l1, l2 = factors(family, n1, n2, k, mixed)
            for d in DELTAS:
                dt = delta_t(d)
                for e in EXPONENTS:
                    for damping in ((False, True) if n2 else (False,)):
                        want = REF.kron_pow(l1, l2, dt, e, damping)
                        assert bool((want > 0).all()) and bool(torch.isfinite(want).all())
                        got = K.kron_pow(dev(l1), None if l2 is None else dev(l2), dev(dt), e, damping)
                        assert tuple(got.shape) == tuple(want.shape)
                        w.see("kron_pow", elem_err(got, want))
    return w


# ---- kron_logdet ------------------------------------------------------------------------------------------------------------
def _abs_logs(l1, l2, dt, damping=False):
    """(sum |log v|, number of entries)"""
    v = REF.kron_pow(l1, l2, dt, 1.0, damping)
    return v.log().abs().sum().item(), v.numel()


def check_logdet(K, dev, family: str, n1: int, n2: int) -> Worst:
    w = Worst()
    for k in SCALES:
        for mixed in ((False, True) if n2 else (False,)):
            l1, l2 = factors(family, n1, n2, k, mixed)
            for d in DELTAS:
                dt = delta_t(d)
                want = REF.kron_logdet(l1, l2, dt, False, True)
                got = K.kron_logdet(dev(l1), None if l2 is None else dev(l2), dev(dt), False, True)
                w.see("kron_logdet value", logdet_err(got[0].item(), want[0].item(), *_abs_logs(l1, l2, dt)))
                for g_, w_, nm in zip(got[1:], want[1:], ("d_l1", "d_l2", "d_delta")):
                    assert (g_ is None) == (w_ is None), nm
                    if w_ is not None:
                        w.see(f"kron_logdet {nm}", elem_err(g_, w_))
                if n2:
                    wd = REF.kron_logdet(l1, l2, dt, True)[0].item()
                    gd = K.kron_logdet(dev(l1), dev(l2), dev(dt), True)[0].item()
                    w.see("kron_logdet damped value", logdet_err(gd, wd, *_abs_logs(l1, l2, dt, True)))
    return w


def logdet_blocks_case():
    """42 blocks (more than the 32 one launch carries): every family at every scale, sizes and deltas cycling, every other
    two-factor block with a second factor of another family"""
    blocks, deltas = [], []
    i = 0
    for rep in range(2):
        for fam in FAMILIES:
            for k in SCALES:
                n1, n2 = SIZES[(i + rep) % len(SIZES)]
                l1, l2 = factors(fam, n1, n2, k, mixed=bool(i % 2))
                blocks.append((l1,) if l2 is None else (l1, l2))
                deltas.append(DELTAS[(i + 2 * rep) % len(DELTAS)])
                i += 1
    return blocks, f32(torch.tensor(deltas, dtype=torch.float64))


def check_logdet_blocks(K, dev, scale) -> Worst:
    w = Worst()
    blocks, deltas = logdet_blocks_case()
    sc = None if scale is None else f32(torch.tensor([scale], dtype=torch.float64))
    want = REF.kron_logdet_blocks(blocks, deltas, sc, True)  # (fp64 inside, fp32 out: recompute the value in fp64 below)
    s = 1.0 if sc is None else sc.item()
    val, abs_logs, count, dd, ds = 0.0, 0.0, 0, [], 0.0
    for ls, d in zip(blocks, deltas):
        lam = ls[0] if len(ls) == 1 else torch.outer(ls[0], ls[1])
        M = s * lam + d
        val += torch.log(M).sum().item()
        abs_logs += torch.log(M).abs().sum().item()
        count += M.numel()
        dd.append((1.0 / M).sum())
        ds += (lam / M).sum().item()
    args = ([tuple(dev(l) for l in ls) for ls in blocks], dev(deltas), None if sc is None else dev(sc), True)
    got = K.kron_logdet_blocks(*args)
    assert (got[2] is None) == (sc is None) and want[1].shape == got[1].shape
    w.see("kron_logdet_blocks value", logdet_err(got[0].item(), val, abs_logs, count))
    w.see("kron_logdet_blocks d_delta", elem_err(got[1], torch.stack(dd)))
    if sc is not None:
        w.see("kron_logdet_blocks d_scale", elem_err(got[2], torch.tensor([ds], dtype=torch.float64)))
    again = K.kron_logdet_blocks(*args)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1]), "fixed-order reduction: bit for bit"
    assert sc is None or torch.equal(again[2], got[2])
    return w


# ---- kron_sandwich ----------------------------------------------------------------------------------------------------------
SANDWICH_SIZES = ((1, 0), (33, 0), (2, 65), (64, 193), (129, 257))
SANDWICH_ROWS = 9


def check_sandwich(K, dev, family: str, pi: int, po: int) -> Worst:
    """rows of W scaled over 2^-20 ... 2^20 within one call, the block at a non-zero ``col0`` inside a wider ``P``; the
    error of each row against its own largest entry, and the columns outside the block untouched"""
    w = Worst()
    R, col0 = SANDWICH_ROWS, 7
    p = pi * po if po else pi
    P = col0 + p + 5
    Q1 = f32(orthogonal(pi, 50 + pi))
    Q2 = f32(orthogonal(po, 70 + po)) if po else None
    W = _randn(R, P, seed=pi * 1000 + po)
    W = f32(W * torch.exp2(torch.linspace(-20, 20, R).round()).view(R, 1))
    for k in SCALES:
        l1, l2 = factors(family, pi, po, k, mixed=True)
        for d, e in ((1e-4, -1.0), (1.0, -0.5), (1e4, -1.0)):
            lam = f32(REF.kron_pow(l1, l2, delta_t(d), e))
            fill = _randn(R, P, seed=3)
            want = REF.kron_sandwich(W, col0, P, R, Q1, Q2, lam, fill.clone())
            out = dev(fill)
            K.kron_sandwich(dev(W), col0, P, R, dev(Q1), None if Q2 is None else dev(Q2), dev(lam), out)
            got = out.detach().double().cpu()
            w.see("kron_sandwich per row", sample_err(got[:, col0:col0 + p], want[:, col0:col0 + p]))
            keep = torch.ones(P, dtype=torch.bool)
            keep[col0:col0 + p] = False
            assert torch.equal(got[:, keep], f32(fill)[:, keep]) or torch.equal(got[:, keep], fill[:, keep]), \
                "columns outside the block are not touched"
    return w


# ---- quadratic forms ----------------------------------------------------------------------------------------------------------
LINEAR_SHAPES = ((1, 1, 1, 1), (5, 3, 5, 67), (9, 10, 33, 257))            # B, C, Do, Di
SHARED_SHAPES = ((1, 1, 1, 1, 1), (5, 3, 5, 67, 9), (9, 10, 33, 257, 17))  # B, C, Do, Dk, L: B = 9 is more samples than fit
#                                                                            one workgroup of the shared kernel


def sample_scales(B: int, zero: bool):
    """2^{k_n}, k_n spread over -20 ... 20, and the index of the all-zero sample (None without one)"""
    k = torch.linspace(-20, 20, B).round() if B > 1 else torch.tensor([-20.0])
    s = torch.exp2(k.double())
    z = (B // 2 if B > 1 else 0) if zero else None
    if z is not None:
        s[z] = 0.0
    return s, z


def _zero_variants(B):
    return (True,) if B > 1 else (True, False)  # a batch of one: once as the zero sample, once as an ordinary one


def _base_for(res, z, seed):
    """what the accumulating kernels are handed: per sample a symmetric block of the size of that sample's result (so the
    sum still shows the result), O(1) for the zero sample"""
    B, C = res.shape[0], res.shape[1]
    b = _randn(B, C, C, seed=seed)
    b = b + b.transpose(1, 2)
    mag = res.abs().reshape(B, -1).amax(1)
    if z is not None:
        mag[z] = 1.0
    return f32(b * mag.view(B, 1, 1))


def _check_accumulating(w, name, call, ref, shape, z, seed, dev):
    """``call(base)`` / ``ref(base)`` accumulate into ``base [B, C, C]``"""
    res = ref(torch.zeros(shape, dtype=torch.float64))
    base = _base_for(res, z, seed)
    want = ref(base.clone())
    got = call(dev(base)).detach().double().cpu()
    w.see(name, sample_err(got, want))
    if z is not None:
        assert torch.equal(got[z], base[z]), f"{name}: the all-zero sample's block must come back as it was passed in"


def check_quad_linear(K, dev, family: str, shape) -> Worst:
    w = Worst()
    B, C, Do, Di = shape
    for zero in _zero_variants(B):
        s, z = sample_scales(B, zero)
        u = f32(_randn(C, B, Do, seed=11) * s.view(1, B, 1))
        ub = f32(_randn(C, B, Do, seed=12) * s.view(1, B, 1))
        v = f32(_randn(B, Di, seed=13) * (s != 0).double().view(B, 1))
        Js = f32(_randn(B, C, Do * Di, seed=14) * s.view(B, 1, 1))
        for k in SCALES:
            l1, l2 = eigs(family, Do, k), eigs(partner(family), Di, k)
            lb = eigs(family, Do, k)
            for d in DELTAS:
                dt = delta_t(d)
                for bias in (False, True):
                    extra = (ub, lb, dt) if bias else ()
                    _check_accumulating(
                        w, "kron_quadform_linear" + (" + bias" if bias else ""),
                        lambda b: K.kron_quadform_linear(dev(u), dev(v), dev(l1), dev(l2), dev(dt), b, *map(dev, extra)),
                        lambda b: REF.kron_quadform_linear(u, v, l1, l2, dt, b, *extra), (B, C, C), z, 21, dev)
                vw = f32(REF.kron_pow(l1, l2, dt, -1.0)).reshape(-1)
                vb = f32(REF.kron_pow(lb, None, dt, -1.0))
                for bias in (False, True):
                    _check_accumulating(
                        w, "diag_quadform_linear" + (" + bias" if bias else ""),
                        lambda b: K.diag_quadform_linear(dev(v), dev(u), dev(vw), dev(vb) if bias else None, b),
                        lambda b: REF.diag_quadform_linear(v, u, vw, vb if bias else None, b), (B, C, C), z, 22, dev)
                got = K.diag_quadform_js(dev(Js), dev(vw)).detach().double().cpu()
                w.see("diag_quadform_js", sample_err(got, REF.diag_quadform_js(Js, vw)))
                if z is not None:
                    assert bool((got[z] == 0).all()), "diag_quadform_js: the all-zero sample's block is exactly zero"
    return w


def _grid_weights(mode, l1, l2, Do, Di):
    """(w0, w1) of the grid kernels: the eigenvalues (Kron, damped Kron) or a diagonal Hessian h [Do, Di]"""
    if mode == 2:
        return torch.outer(l1, l2).reshape(-1), None
    return l1, l2


def _check_grid(w, name, call, ref, G, B, C, z, dev):
    base = torch.zeros(G, B, C, dtype=torch.float64)
    if z is not None:
        base[:, z] = 0.375
    want = ref(base.clone())
    got = call(dev(base)).detach().double().cpu()
    w.see(name, elem_err(got, want))
    if z is not None:
        assert torch.equal(got[:, z], base[:, z]), f"{name}: the all-zero sample's row must come back as it was passed in"


def check_grid_linear(K, dev, family: str, shape) -> Worst:
    w = Worst()
    B, C, Do, Di = shape
    deltas = f32(torch.tensor(DELTAS, dtype=torch.float64))
    for zero in _zero_variants(B):
        s, z = sample_scales(B, zero)
        u = f32(_randn(C, B, Do, seed=11) * s.view(1, B, 1))
        ub = f32(_randn(C, B, Do, seed=12) * s.view(1, B, 1))
        v = f32(_randn(B, Di, seed=13) * (s != 0).double().view(B, 1))
        for k in SCALES:
            l1, l2, wb = eigs(family, Do, k), eigs(partner(family), Di, k), eigs(family, Do, k)
            for mode in (0, 1, 2):
                w0, w1 = _grid_weights(mode, l1, l2, Do, Di)
                for bias in (False, True):
                    extra = (ub, wb) if bias else ()
                    _check_grid(
                        w, f"quadform_linear_grid mode {mode}",
                        lambda b: K.quadform_linear_grid(dev(u), dev(v), dev(w0), None if w1 is None else dev(w1), dev(deltas),
                                                         mode, b, *map(dev, extra)),
                        lambda b: GREF.quadform_linear_grid(u, v, w0, w1, deltas, mode, b, *extra), len(DELTAS), B, C, z, dev)
    return w


def check_quad_shared(K, dev, family: str, shape) -> Worst:
    w = Worst()
    B, C, Do, Dk, L = shape
    deltas = f32(torch.tensor(DELTAS, dtype=torch.float64))
    for zero in _zero_variants(B):
        s, z = sample_scales(B, zero)
        u = f32(_randn(B, C, Do, L, seed=31) * s.view(B, 1, 1, 1))
        us = u.permute(1, 0, 2, 3).contiguous()
        v = f32(_randn(B, Dk, L, seed=32) * (s != 0).double().view(B, 1, 1))
        for k in SCALES:
            l1, l2 = eigs(family, Do, k), eigs(partner(family), Dk, k)
            for d in DELTAS:
                dt = delta_t(d)
                for seed_major in (False, True):
                    uu = us if seed_major else u
                    _check_accumulating(
                        w, "kron_quadform_shared" + (" seed-major" if seed_major else ""),
                        lambda b: K.kron_quadform_shared(dev(uu), dev(v), dev(l1), dev(l2), dev(dt), b, seed_major=seed_major),
                        lambda b: REF.kron_quadform_shared(uu, v, l1, l2, dt, b, seed_major=seed_major), (B, C, C), z, 41, dev)
                vw = f32(REF.kron_pow(l1, l2, dt, -1.0))
                _check_accumulating(
                    w, "diag_quadform_shared", lambda b: K.diag_quadform_shared(dev(u), dev(v), dev(vw), b),
                    lambda b: REF.diag_quadform_shared(u, v, vw, b), (B, C, C), z, 42, dev)
            for mode in (0, 1, 2):
                w0, w1 = _grid_weights(mode, l1, l2, Do, Dk)
                for seed_major in (False, True):
                    uu = us if seed_major else u
                    _check_grid(
                        w, f"quadform_shared_grid mode {mode}",
                        lambda b: K.quadform_shared_grid(dev(uu), dev(v), dev(w0), None if w1 is None else dev(w1), dev(deltas),
                                                         mode, b, seed_major=seed_major),
                        lambda b: GREF.quadform_shared_grid(uu, v, w0, w1, deltas, mode, b, seed_major=seed_major),
                        len(DELTAS), B, C, z, dev)
    return w


def bound_of(metric: str) -> float:
    if metric.startswith("kron_pow") or metric.startswith("kron_logdet"):
        return BOUND_POW
    if metric.startswith("kron_sandwich"):
        return BOUND_SANDWICH
    if "grid" in metric:
        return BOUND_GRID
    return BOUND_QUAD
