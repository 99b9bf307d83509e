"""Cases, fp64 references and the error bound of the spectral dense-Laplace kernels (csrc/lk_spectral.hip):

    COV   fvar[n][c][k] = sum_j R[n][c][j] R[n][k][j] / (hfac lam_j + delta)
    GRID  var[g][n][c]  = sum_j R[n][c][j]^2 / (hfac lam_j + deltas[g])

with R given (the R loader) or R[n][c][j] = sum_d phi[n][d] Q[c D + d][j] (+ Q[C D + c][j]) formed by the kernel (the LL loader).

The table takes the smallest shapes at which each path can go wrong, read off ``lk_spectral_variant``: tiles of TILE_N = 32 samples
x TILE_J = 128 eigen-columns; a workgroup walks a contiguous range of column tiles (ONE tile each unless the sample tiles alone
fill the device: the 9 600-sample rows are there for the ranges of two tiles, i.e. for the running sums carried from tile to tile);
COV holds 1, 2, 5 or 10 outputs and runs C > 10 in pairs of blocks of 5; GRID walks chunks of 64 / CT (5 for ten outputs) grid
points and 128 points per launch.

The bound (element-wise, independent of the summation order; u = 2^-24).  The kernel's R_c differs from the exact one by at most
e_c = (D + 3) u a,  a = sum_d |phi| |Q| + |bias row|  (D products accumulated in fp32 in some order plus one addition: gamma_{D+1} a,
first order, with slack; e = 0 for the R loader, which reads R).  Each term w_j R_c R_k then carries the perturbation of the two
factors, (|R_c| + e_c)(|R_k| + e_k) - |R_c R_k|, and the roundings of its own arithmetic: hfac lam (1), + delta (1), the hardware
reciprocal (1 ulp = 2 u), the two products (2); summing P such terms in ANY order adds at most (P - 1) u of the sum of their
magnitudes.  6 + P - 1 <= P + 10, and 3 more for the second-order terms dropped:

    |err| <= sum_j w_j [(|R_c| + e_c)(|R_k| + e_k) - |R_c R_k|] + (P + 10 + 3) u sum_j w_j |R_c R_k| + P 2^-126

(2^-126 per term: a product that underflows).  Nothing here is tuned to what the kernels return.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import torch

from tests.eig_fixtures import orthogonal
from tests.kronalg_fixtures import eigs

U = 2.0 ** -24
TILE_N, TILE_J, GMAX = 32, 128, 128
QUAD_LL, GRID_LL, QUAD_R, GRID_R, BIAS = 0, 1, 2, 3, 4
FAMILIES = ("spiked", "graded", "dscaled")
DELTAS = (1e-4, 1.0, 1e4)
HFACS = (0.25, 1.0, 7.0)
BIG_N = 32 * 300  # sample tiles enough that a workgroup owns TWO column tiles (ceil(512 / 300) = 2 ranges for three tiles)


def _case(loader, epi, N, C, DP, bias=0, G=1, i=0, unaligned=False, exact=False):
    return dict(loader=loader, epi=epi, N=N, C=C, DP=DP, bias=bias, G=G, family=FAMILIES[i % 3], delta=DELTAS[i % 3],
                hfac=HFACS[(i // 3 + i) % 3], unaligned=unaligned, exact=exact)


def _table():
    rows, i = [], 0

    def add(*a, **k):
        nonlocal i
        rows.append(_case(*a, i=i, **k))
        i += 1

    # R loader: P around the column tile (1, tile - 1, tile, tile + 1, two tiles + 1), every class block, N around the sample tile
    for P in (1, 127, 128, 129, 257):
        add("r", "cov", 1 if P == 1 else 33, 3, P, unaligned=P == 129)
        add("r", "grid", 31, 2, P, G=6, unaligned=P == 257)
    for C in (1, 2, 3, 10, 11, 21):
        add("r", "cov", 33, C, 129)
        add("r", "grid", 1 if C == 1 else 31, C, 129, G={1: 64, 2: 33, 3: 11, 10: 6, 11: 5, 21: 4}[C])
    # grid chunks: 64 / CT points (CT = 1: 63, 64, 65; CT = 10: 4, 5, 6), the grid of the search (100), more than one launch (130)
    for G in (1, 63, 65, 100, 130):
        add("r", "grid", 2, 1, 130, G=G)
    add("r", "grid", 33, 10, 257, G=100)
    # column ranges of two tiles (the sums carried across tiles; the last range holds one)
    add("r", "cov", BIG_N, 1, 257)
    add("r", "grid", BIG_N, 1, 257, G=2)
    # LL loader: D in {1, 31, 33} with and without a bias row, every class block
    for D in (1, 31, 33):
        for bias in (0, 1):
            add("ll", "cov", 33, 3, D, bias=bias, unaligned=D == 31)
            add("ll", "grid", 31, 2, D, bias=bias, G=33)
    add("ll", "cov", 1, 1, 1)
    add("ll", "grid", 1, 1, 1, G=1)
    for C in (1, 2, 3, 10, 11, 21):
        add("ll", "cov", 31, C, 33 if C < 21 else 31, bias=1)
        add("ll", "grid", 33, C, 31, bias=C % 2, G=5 if C >= 10 else 7)
    add("ll", "grid", 33, 10, 31, bias=1, G=100)
    # the widest heads: more than 64 KiB of staged features (the raised dynamic-LDS limit), and the largest arena the guard admits
    add("ll", "cov", 33, 1, 512, bias=1)
    add("ll", "grid", 2, 1, 896, bias=1, G=65)
    add("ll", "cov", BIG_N, 8, 33, bias=1)
    add("ll", "grid", BIG_N, 8, 33, bias=1, G=2)
    # integer operands and power-of-two weights: every product and sum is exact, the result is bit-equal in any order
    add("r", "cov", 33, 3, 129, exact=True)
    add("ll", "cov", 33, 3, 33, bias=1, exact=True)
    add("ll", "grid", 33, 2, 31, bias=1, G=3, exact=True)
    return rows


CASES = _table()


def case_id(c) -> str:
    return (f"{c['loader']}-{c['epi']}-N{c['N']}-C{c['C']}-{'D' if c['loader'] == 'll' else 'P'}{c['DP']}"
            f"{'b' if c['bias'] else ''}-G{c['G']}{'-x' if c['exact'] else ''}{'-u' if c['unaligned'] else ''}")


def form_of(c) -> int:
    base = {("ll", "cov"): QUAD_LL, ("ll", "grid"): GRID_LL, ("r", "cov"): QUAD_R, ("r", "grid"): GRID_R}[(c["loader"], c["epi"])]
    return base | (BIAS if c["bias"] else 0)


def n_params(c) -> int:
    return c["C"] * c["DP"] + (c["C"] if c["bias"] else 0) if c["loader"] == "ll" else c["DP"]


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _randint(lo, hi, *shape, seed):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed)).double()


@lru_cache(maxsize=None)
def _operands_cached(idx: int):
    c = CASES[idx]
    N, C, DP, P, G = c["N"], c["C"], c["DP"], n_params(c), c["G"]
    seed = 7000 + idx
    if c["exact"]:
        lam = (2.0 ** _randint(1, 5, P, seed=seed)) - 1.0          # 1, 3, 7, 15
        hfac, deltas = 1.0, torch.ones(G, dtype=torch.float64)     # mu = 2, 4, 8, 16
        if G > 1:
            lam = torch.full((P,), 3.0, dtype=torch.float64)
            deltas = torch.tensor([1.0, 5.0, 13.0, 29.0, 61.0], dtype=torch.float64)[:G]  # mu = 4, 8, 16, ...
        X = _randint(-3, 4, N, DP, seed=seed + 1) if c["loader"] == "ll" else _randint(-3, 4, N, C, P, seed=seed + 1)
        Q = _randint(-2, 3, P, P, seed=seed + 2) if c["loader"] == "ll" else None
    else:
        lam = eigs(c["family"], P).clone()
        hfac = c["hfac"]
        if G == 1:
            deltas = torch.tensor([c["delta"]], dtype=torch.float64)
        else:
            deltas = torch.logspace(-4, 4, G, dtype=torch.float64)
        scale = torch.logspace(-1, 1, N, dtype=torch.float64)[torch.randperm(N, generator=torch.Generator().manual_seed(seed))]
        if c["loader"] == "ll":
            X = _randn(N, DP, seed=seed + 1) * scale[:, None]
            Q = orthogonal(P, seed + 2)
        else:
            X = _randn(N, C, P, seed=seed + 1) * scale[:, None, None]
            Q = None
    f32 = lambda t: None if t is None else t.float().double()  # noqa: E731
    return f32(X), f32(Q), f32(lam), float(np.float32(hfac)), f32(deltas)


def operands(idx: int):
    """``(X, Q, lam, hfac, deltas)`` as fp64 tensors that hold fp32 values: X = phi [N, D] or R [N, C, P]"""
    return _operands_cached(idx)


def rotated(c, X, Q, drop_bias=False, row_shift=0):
    """exact R [N, C, P] and the loader's error scale a [N, C, P] (zero for the R loader), fp64"""
    if c["loader"] == "r":
        return X, torch.zeros_like(X)
    C, D, P = c["C"], c["DP"], n_params(c)
    rows = (torch.arange(C)[:, None] * D + torch.arange(D)[None, :] + row_shift).clamp(max=P - 1)
    W = Q[rows]                                   # [C, D, P]
    R = torch.einsum("nd,cdj->ncj", X, W)
    a = torch.einsum("nd,cdj->ncj", X.abs(), W.abs())
    if c["bias"] and not drop_bias:
        R = R + Q[C * D:][None]
        a = a + Q[C * D:].abs()[None]
    return R, a


@lru_cache(maxsize=None)
def reference(idx: int):
    """``(want, bound)`` in fp64: COV [N, C, C], GRID [G, N, C]"""
    c = CASES[idx]
    X, Q, lam, hfac, deltas = operands(idx)
    P = n_params(c)
    R, a = rotated(c, X, Q)
    e = (c["DP"] + 3) * U * a if c["loader"] == "ll" else a
    Ra, Re = R.abs(), R.abs() + e
    tiny = P * 2.0 ** -126
    if c["epi"] == "cov":
        w = 1.0 / (hfac * lam + deltas[0])
        want = torch.einsum("ncj,nkj,j->nck", R, R, w)
        mag = torch.einsum("ncj,nkj,j->nck", Ra, Ra, w)
        pert = torch.einsum("ncj,nkj,j->nck", Re, Re, w) - mag
    else:
        w = 1.0 / (hfac * lam[None, :] + deltas[:, None])  # [G, P]
        want = torch.einsum("ncj,gj->gnc", R * R, w)
        mag = want
        pert = torch.einsum("ncj,gj->gnc", Re * Re, w) - mag
    return want, pert + (P + 13) * U * mag + tiny


def ratio(got, idx: int) -> float:
    """worst |got - want| / bound over the elements (inf for a non-finite output)"""
    want, bound = reference(idx)
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - want).abs() / bound).max())


# ---- fp32 restatements in numpy (two blockings) and the mutants the bound must catch ------------------------------------------
def restate(idx: int, block: int = 128, mutant: str | None = None):
    """the kernels' arithmetic in fp32 numpy: R by sequential accumulation over d, the weighted sum over blocks of ``block``
    columns (each block summed in order, the blocks added in order)"""
    c = CASES[idx]
    X, Q, lam, hfac, deltas = (None if t is None else (t if isinstance(t, float) else t.numpy()) for t in operands(idx))
    f = np.float32
    C, P = c["C"], n_params(c)
    if c["loader"] == "ll":
        D = c["DP"]
        phi, Q32 = X.astype(f), Q.astype(f)
        shift = 1 if mutant == "panel_off_by_one" else 0
        R = np.zeros((c["N"], C, P), dtype=f)
        for d in range(D):
            rows = np.minimum(np.arange(C) * D + d + shift, P - 1)
            R += phi[:, d][:, None, None] * Q32[rows][None]
        if c["bias"] and mutant != "bias_dropped":
            R += Q32[C * D:][None]
    else:
        R = X.astype(f)
    lam32, h32, d32 = lam.astype(f), f(hfac), deltas.astype(f)

    def weights(d):
        if mutant == "hfac_dropped":
            return f(1) / (lam32 + d)
        if mutant == "delta_before_hfac":
            return f(1) / (h32 * (lam32 + d))
        return f(1) / (h32 * lam32 + d)

    def blocked(terms):  # [..., P] -> [...]
        out = np.zeros(terms.shape[:-1], dtype=f)
        for j0 in range(0, P, block):
            part = np.zeros(terms.shape[:-1], dtype=f)
            for j in range(j0, min(j0 + block, P)):
                part += terms[..., j]
            out += part
        return out

    if c["epi"] == "cov":
        w = weights(d32[0])
        return torch.from_numpy(blocked((R * w)[:, :, None, :] * R[:, None, :, :]))
    sq = np.abs(R) if mutant == "grid_not_squared" else R * R
    return torch.from_numpy(np.stack([blocked(sq * weights(d)) for d in d32]))


MUTANTS = ("hfac_dropped", "grid_not_squared", "bias_dropped", "panel_off_by_one", "delta_before_hfac")


def emulate(idx: int) -> torch.Tensor:
    """the fp64 reference rounded to fp32: what an exact kernel would return"""
    return reference(idx)[0].float()


# ---- grid against loop on the mlp golden (all weights: the R loader) --------------------------------------------------------
GRID_LOOP = torch.logspace(-2, 2, 9)


@lru_cache(maxsize=None)
def grid_loop_case():
    """fp64, on the CPU: the validation NLL (probit link) of the ``mlp`` classification golden at every prior precision of
    ``GRID_LOOP`` under the dense posterior over all weights, and the largest difference ``tol`` the batched grid and the
    per-point loop of the spectral route may show in it.

    Both device routes weight the SAME rotated Jacobians R (one deterministic ``lk_gemm_f32``) with the same spectrum, so their
    variances differ from the exact weighted sum by at most the GRID and the COV kernel bound, each ``(P + 13) u var + P 2^-126``
    (R loader: e = 0, and the magnitude sum of a diagonal entry is the entry itself; 1 % is added for ``var`` being the fp64
    value, not the device's).  The loss of a sample is ``-log softmax(z)[y]``, ``z_c = f_c / sqrt(1 + pi/8 var_c)``:
    ``|d loss / d z_c| = |p_c - [c = y]| <= 1`` and ``|d z_c / d var_c| = |f_c| (pi/16) (1 + pi/8 var_c)^-3/2``, so the variance
    bounds move a sample's loss by at most ``sum_c |f_c| (pi/16) (1 + pi/8 var_c)^-3/2 dvar_c``.  Either route then evaluates
    the link in fp32: z (a square root, a division, two products: <= 5 u |z|), a softmax over C terms and a logarithm
    (<= (C + 6) u (1 + |loss|) with |d loss / d z| <= 1 counted twice for max-subtraction), taken as ``(C + 16) u (1 + max|z| +
    loss)`` per route.  The mean over the samples is a fp64 sum.  Nothing here looks at what the device returns.

    Asserted here, on the CPU: the two best fp64 losses of the grid differ by more than ``2 tol``, so the argmin of two loss
    vectors that agree within ``tol`` is the same point."""
    from math import pi

    from oracle import curvature_oracle as co
    from tests.conftest import golden_model, load_golden

    g = load_golden("mlp", "classification")
    m64, X64, y = golden_model("mlp", g, dtype=torch.float64, device="cpu")
    with torch.enable_grad():
        Js, f = co.jacobians(m64, X64)
    Js, f = Js.detach().double(), f.detach().double()
    H = torch.as_tensor(g["la.all.full.H"], dtype=torch.float64)
    P, C = H.shape[0], f.shape[1]
    losses, tols = [], []
    for d in GRID_LOOP.double():
        Sigma = torch.linalg.inv(H + d * torch.eye(P, dtype=torch.float64))
        var = torch.einsum("ncp,pq,ncq->nc", Js, Sigma, Js)
        kappa = 1.0 / torch.sqrt(1.0 + pi / 8 * var)
        z = kappa * f
        nll = -torch.log_softmax(z, dim=-1)[torch.arange(len(y)), y]
        dvar = 2 * ((P + 13) * U * var * 1.01 + P * 2.0 ** -126)
        moved = (f.abs() * (pi / 16) * (1.0 + pi / 8 * var) ** -1.5 * dvar).sum(-1)
        link = 2 * (C + 16) * U * (1.0 + z.abs().max(-1).values + nll)
        losses.append(float(nll.mean()))
        tols.append(float((moved + link).mean()))
    losses = torch.tensor(losses, dtype=torch.float64)
    tol = max(tols)
    two = torch.sort(losses).values[:2]
    assert float(two[1] - two[0]) > 2 * tol, (losses, tol)
    return {"grid": GRID_LOOP, "losses": losses, "tol": tol, "argmin": int(losses.argmin())}
