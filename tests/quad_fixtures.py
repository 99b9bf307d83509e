"""Seeded operands, the fp64 reference and the table of shapes for the weight-sharing predictive kernels
(``quadform_conv_kernel``, ``quadform_conv_planes_kernel``, ``diag_ggn_shared_kernel``, ``quadform_shared_grid_kernel`` and
``quadform_linear_grid_kernel`` of laplace_amd/csrc/lk_quadconv.hip, lk_grid.hip).  tests/test_quad_fixtures.py pins, on the
CPU, that the table reaches EVERY instantiation the launchers can pick (through ``lk_quadform_shared_variant``) and that the
inputs leave room under the tolerance; tests/test_gpu_quadform_instances.py holds the kernels to it on the device.

TEST INFRASTRUCTURE, in the style of tests/eig_fixtures.py: everything is drawn on a seeded CPU generator; the reference is
the definition as plain fp64 einsums and shares no code with tests/emulated_kernels.py.

Operands (``operands``):
  * ``u [C, B, Do, L]``  output gradients, CORRELATED across outputs and differently scaled:
                         u_c = (0.6 shared + 0.8 own_c) (1 + c) 3e-3 — every one of the C (C + 1) / 2 pair sums is a
                         distinct large number (off-diagonal / diagonal of the reference: 2 - 5), so a swapped pair index
                         moves it; with independent outputs the off-diagonal sums are noise next to the diagonal
  * ``v [B, Dk, L]``     post-ReLU, one magnitude per sample over five decades (what the per-image scales exist for)
  * spectra ``flat``     l = rand + 0.1, delta = 0.7 (what the older tests draw)
            ``kfac``     l1 = 10^linspace(-8, 2), lowest quarter exactly 0; l2 = 10^linspace(-9, 3), lowest third exactly 0;
                         delta = 1e-3 (a clamped KFAC posterior: ten decades, exact zeros, a small prior precision)
  * ``var_w [Do, Dk]``   1 / (outer(l1, l2) + delta), the diagonal posterior of the same problem
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

SPECTRA = ("flat", "kfac")
#: prior precisions of the grid kernels (tests/test_gpu_prior_grid.py uses the same)
DELTAS = torch.logspace(-4, 4, 9)
#: |got - want| <= RTOL |want| + ATOL max|want|, element-wise (README: the criterion the factors are held to)
RTOL, ATOL = 1e-4, 1e-6

# forms of lk_quadform_shared_variant (LK_QF_* of include/laplace_hip.h)
QF_KRON, QF_KRON_SEEDMAJOR, QF_DIAG, QF_PLANES, QF_DIAG_GGN, QF_GRID = range(6)
CLASS_TILES = (1, 2, 3, 4, 5, 6, 8, 10)
GRID_CLASS_TILES = (1, 2, 5, 10)


def operands(C, B, Do, Dk, L, seed, spectrum="flat"):
    """fp32 CPU tensors ``u [C, B, Do, L]``, ``v [B, Dk, L]``, ``l1 [Do]``, ``l2 [Dk]``, ``delta [1]``, ``var_w [Do, Dk]``"""
    g = torch.Generator().manual_seed(int(seed))
    shared = torch.randn(B, Do, L, generator=g)
    own = torch.randn(C, B, Do, L, generator=g)
    scale = (1.0 + torch.arange(C, dtype=torch.float32)).reshape(C, 1, 1, 1)
    u = (0.6 * shared[None] + 0.8 * own) * scale * 3e-3
    mag = 10.0 ** torch.linspace(-3, 2, B)
    v = torch.randn(B, Dk, L, generator=g).relu_() * mag.reshape(B, 1, 1)
    l1f, l2f = torch.rand(Do, generator=g) + 0.1, torch.rand(Dk, generator=g) + 0.1
    return SimpleNamespace(u=u.contiguous(), v=v.contiguous(), flat_l1=l1f, flat_l2=l2f, **_spectrum(spectrum, Do, Dk, l1f, l2f))


def _spectrum(spectrum, Do, Dk, l1f, l2f):
    if spectrum == "flat":
        l1, l2, delta = l1f, l2f, 0.7
    elif spectrum == "kfac":
        l1 = (10.0 ** torch.linspace(-8, 2, Do, dtype=torch.float64)).float()
        l2 = (10.0 ** torch.linspace(-9, 3, Dk, dtype=torch.float64)).float()
        l1[: Do // 4] = 0.0
        l2[: Dk // 3] = 0.0
        delta = 1e-3
    else:
        raise ValueError(spectrum)
    delta = torch.tensor([delta], dtype=torch.float32)
    var_w = (1.0 / (torch.outer(l1.double(), l2.double()) + delta.double())).float()
    return dict(l1=l1.contiguous(), l2=l2.contiguous(), delta=delta, var_w=var_w.contiguous(), spectrum=spectrum)


def with_spectrum(ops, spectrum):
    """the same u, v (shared, not copied) under the other spectrum, on the device the operands live on"""
    Do, Dk = ops.u.shape[2], ops.v.shape[1]
    sp = _spectrum(spectrum, Do, Dk, ops.flat_l1.cpu(), ops.flat_l2.cpu())
    sp = {k: (t.to(ops.u.device) if torch.is_tensor(t) else t) for k, t in sp.items()}
    return SimpleNamespace(u=ops.u, v=ops.v, flat_l1=ops.flat_l1, flat_l2=ops.flat_l2, **sp)


def first_positions(ops, L):
    """the operands restricted to their first L shared positions (a shorter map of the same draw)"""
    d = dict(vars(ops))
    d["u"], d["v"] = ops.u[..., :L].contiguous(), ops.v[..., :L].contiguous()
    return SimpleNamespace(**d)


# ---- the fp64 reference: the definition, evaluated in chunks of samples --------------------------------------------------
def _chunks(B, per_sample_elems, budget_bytes=200e6):
    nb = max(1, int(budget_bytes // (8 * max(1, per_sample_elems))))
    return [(n0, min(B, n0 + nb)) for n0 in range(0, B, nb)]


def kron_weights(l1, l2, delta):
    """[Do, Dk] fp64 weights of the Kronecker posterior from the fp32 eigenvalues the kernel is given"""
    return 1.0 / (torch.outer(l1.double(), l2.double()) + delta.double().reshape(()))


def reference_fvar(u, v, w):
    """``fvar [B, C, C]`` (fp64) of ``u [C, B, Do, L]``, ``v [B, Dk, L]`` under the weights ``w [Do, Dk]``:
    f_var[n][c][k] = sum_{o,i} J_c[o,i] J_k[o,i] w[o,i],  J_c = sum_l u_c[:, l] v[:, l]^T.  Runs where ``u`` lives."""
    C, B, Do, L = u.shape
    Dk = v.shape[1]
    w = w.double().to(u.device)
    out = torch.empty(B, C, C, dtype=torch.float64, device=u.device)
    for n0, n1 in _chunks(B, 2 * C * Do * Dk):
        un = u[:, n0:n1].double().permute(1, 0, 2, 3)
        M = torch.einsum("ncol,nil->ncoi", un, v[n0:n1].double())
        out[n0:n1] = torch.einsum("ncoi,nkoi->nck", M * w, M)  # (= "ncoi,nkoi,oi->nck" without its [n, c, k, o, i] intermediate)
    return out


def reference_diag_ggn(u, v):
    """``h [Do * Dk]`` (fp64) = sum over (sample, seed) of the squared per-sample Jacobian; ``u [S, B, Do, L]``"""
    S, B, Do, L = u.shape
    Dk = v.shape[1]
    h = torch.zeros(Do, Dk, dtype=torch.float64, device=u.device)
    for n0, n1 in _chunks(B, 2 * S * Do * Dk):
        M = torch.einsum("ncol,nil->ncoi", u[:, n0:n1].double().permute(1, 0, 2, 3), v[n0:n1].double())
        h += (M * M).sum((0, 1))
    return h.reshape(-1)


def grid_weights(mode, l1, l2, deltas):
    """[G, Do, Dk] fp64 weights of the grid kernels: 0 Kron, 1 damped Kron, 2 diagonal with h = outer(l1, l2) rounded to
    fp32 (what the kernel is given)"""
    d = deltas.double().reshape(-1, 1, 1).to(l1.device)
    if mode == 0:
        return 1.0 / (torch.outer(l1.double(), l2.double())[None] + d)
    if mode == 1:
        sd = d.sqrt()
        return 1.0 / ((l1.double()[None, :, None] + sd) * (l2.double()[None, None, :] + sd))
    return 1.0 / (grid_diag_h(l1, l2).double()[None] + d)


def grid_diag_h(l1, l2):
    return torch.outer(l1, l2).float().contiguous()


def reference_grid_var(u, v, W):
    """``var [G, B, C]`` (fp64): the diagonal of ``reference_fvar`` under each of the weights ``W [G, Do, Dk]``"""
    C, B, Do, L = u.shape
    Dk = v.shape[1]
    out = torch.empty(W.shape[0], B, C, dtype=torch.float64, device=u.device)
    for n0, n1 in _chunks(B, 2 * C * Do * Dk):
        M = torch.einsum("ncol,nil->ncoi", u[:, n0:n1].double().permute(1, 0, 2, 3), v[n0:n1].double())
        out[:, n0:n1] = torch.einsum("ncoi,goi->gnc", M * M, W)
    return out


def reference_linear_grid_var(u, v, W, ub=None, wb=None, deltas=None):
    """nn.Linear layer: ``u [C, B, Do]``, ``v [B, Di]``, ``W [G, Do, Di]``; optional bias block ``ub [C, B, Do]``, ``wb [Do]``"""
    out = torch.einsum("cno,ni,goi->gnc", u.double() ** 2, v.double() ** 2, W)
    if ub is not None:
        out = out + torch.einsum("cno,go->gnc", ub.double() ** 2,
                                 1.0 / (wb.double()[None] + deltas.double().to(wb.device)[:, None]))
    return out


def tolerance_ratio(got, want, scope):
    """worst |got - want| / (RTOL |want| + ATOL max|want|); the max is taken over the last ``scope`` dimensions (fvar
    [B, C, C]: 2, per sample; grid var [G, B, C]: 1, per (grid point, sample); the diag-GGN vector: 1).  <= 1 passes."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    top = want.abs().flatten(want.dim() - scope).amax(-1).reshape(*want.shape[: want.dim() - scope], *([1] * scope))
    bound = RTOL * want.abs() + ATOL * top
    ratio = (got - want).abs() / bound.clamp_min(1e-300)
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    return ratio.max().item()


# ---- the table -----------------------------------------------------------------------------------------------------------
def _row(family, variant, C, Bs, Do, Dk, Ls, **kw):
    return dict(family=family, variant=variant, C=C, Bs=tuple(Bs), Do=Do, Dk=Dk, Ls=tuple(Ls), **kw)


def row_id(row):
    return f"{row['family']}-{row['variant']}-C{row['C']}-Do{row['Do']}-Dk{row['Dk']}-B{'x'.join(map(str, row['Bs']))}"


def _planes_rows():
    rows = []
    sweep = (16, 32, 48, 64, 80, 96, 112, 128)  # one tile per workgroup: Q = 1 ... 8 chunks, both sides of every ring depth
    for C in range(1, 11):
        rows.append(_row("planes", "occ2", C, (3, 8), 64, 200, sweep[1:]))           # ragged 128-column tile
        rows.append(_row("planes", "occ2+sub", C, (3, 8), 32, 160, (16,)))           # one-chunk tiles
        rows.append(_row("planes", "occ1+ldsw", C, (3, 8), 32, 6208, sweep))         # eigenvalues behind the ring
        rows.append(_row("planes", "occ1+memw", C, (3, 8), 32, 10304, sweep))        # eigenvalues from memory
    for C in (2, 5, 6):  # the chunk stream crosses tile boundaries with several chunks per tile (split 8 < ntiles)
        rows.append(_row("planes", "occ2", C, (264,), 64, 640, (48,), stream=True))
        rows.append(_row("planes", "occ1+ldsw", C, (264,), 32, 6208, (32,), stream=True))
    return rows


def _fp32_rows():
    rows = []
    for C in range(1, 11):
        for route in ("kron", "kron-seedmajor", "diag"):
            # ARITH 1: whole float4s; ARITH 0: L % 4 != 0, and L = 16 behind a 4-byte offset (the alignment test)
            rows.append(_row("fp32", f"{route}-arith1", C, (3,), 33, 135, (16,), route=route, arith=1))
            rows.append(_row("fp32", f"{route}-arith0", C, (3,), 33, 135, (9,), route=route, arith=0, offset_Ls=(16,)))
    for C in (1, 6, 10):  # several tiles per workgroup: the `t += split` walk and its next-tile prefetch
        for route in ("kron", "kron-seedmajor", "diag"):
            rows.append(_row("fp32", f"{route}-arith1", C, (264,), 64, 640, (20,), route=route, arith=1, multitile=True))
            rows.append(_row("fp32", f"{route}-arith0", C, (264,), 64, 640, (18,), route=route, arith=0, multitile=True))
    return rows


def _diag_ggn_rows():
    rows = []
    for S in range(1, 11):
        rows.append(_row("diag_ggn", "b6", S, (5,), 33, 129, (16,), arith=1))
        rows.append(_row("diag_ggn", "fp32", S, (5,), 33, 129, (17,), arith=0))
    for S in (1, 5, 10):  # many samples per workgroup: ntiles = 4, nsplit = 256 < B
        rows.append(_row("diag_ggn", "b6", S, (300,), 33, 129, (16,), arith=1, manysamples=True))
        rows.append(_row("diag_ggn", "fp32", S, (300,), 33, 129, (17,), arith=0, manysamples=True))
    return rows


def _grid_rows():
    rows = []
    for C in (1, 2, 3, 4, 5, 13):  # 13: a short second block inside CT = 10
        for mode in (0, 1, 2):
            for seed_major in (False, True):
                lay = "seedmajor" if seed_major else "samplemajor"
                rows.append(_row("grid", f"mode{mode}-{lay}-arith1", C, (3,), 33, 135, (16,), mode=mode, seed_major=seed_major, arith=1))
                rows.append(_row("grid", f"mode{mode}-{lay}-arith0", C, (3,), 33, 135, (9,), mode=mode, seed_major=seed_major, arith=0))
    for mode in (0, 1, 2):  # several tiles per workgroup
        rows.append(_row("grid", f"mode{mode}-samplemajor-arith1", 5, (264,), 64, 640, (16,), mode=mode, seed_major=False, arith=1,
                         multitile=True))
    return rows


def _linear_grid_rows():
    rows = []
    for mode in (0, 1, 2):
        for bias in (False, True):
            b = "bias" if bias else "nobias"
            # GS = 4 < G = 9: the walk over the grid points in LDS pieces;  Di = 4608: more than 64 KiB of LDS, GS = 1
            rows.append(_row("linear_grid", f"mode{mode}-{b}-pieces", 3, (5,), 512, 2048, (1,), mode=mode, bias=bias))
            rows.append(_row("linear_grid", f"mode{mode}-{b}-bigLDS", 2, (5,), 64, 4608, (1,), mode=mode, bias=bias))
    return rows


#: family -> rows; a row is one GPU test case: (family, variant, C) at one layer shape, swept over ``Bs`` x ``Ls``
CASES = {
    "planes": _planes_rows(),
    "fp32": _fp32_rows(),
    "diag_ggn": _diag_ggn_rows(),
    "grid": _grid_rows(),
    "linear_grid": _linear_grid_rows(),
}

FORM_OF_ROUTE = {"kron": QF_KRON, "kron-seedmajor": QF_KRON_SEEDMAJOR, "diag": QF_DIAG}


def row_form(row):
    return {"planes": QF_PLANES, "diag_ggn": QF_DIAG_GGN, "grid": QF_GRID}.get(row["family"]) \
        if row["family"] != "fp32" else FORM_OF_ROUTE[row["route"]]


def class_tile(C, tiles=CLASS_TILES):
    """the padded output count the test expects (checked against the query, never used in its place)"""
    return next(t for t in tiles if C <= t)


def planes_expectation(row):
    """what a planes row's variant name promises of the query's answer"""
    v = row["variant"]
    return dict(occ=2 if v.startswith("occ2") else 1, sub=v.endswith("+sub"), w_in_lds=not v.endswith("memw"))


def planes_ring_depth(var):
    """NS of QcPlanesCfg (lk_quadconv.hip)"""
    return 2 if var["occ"] == 2 else (6 if var["ct"] <= 5 else 4)


def ntiles(Do, Dk):
    return ((Do + 31) // 32) * ((Dk + 127) // 128)


def planes_chunk_counts(Do, Dk, L, split):
    """Q of every workgroup of one sample: its tiles sp, sp + split, ... times the chunks of a tile"""
    nt = ntiles(Do, Dk)
    return [((nt - sp + split - 1) // split if sp < nt else 0) * (L // 16) for sp in range(split)]


# ---- one launch of each family through a kernel provider (the HIP library, or its CPU emulation) ----------------------------
def to_device(ops, dev):
    return SimpleNamespace(**{k: (t.to(dev) if torch.is_tensor(t) else t) for k, t in vars(ops).items()})


def run_planes(K, ops, per_image, fvar=None):
    """lk_kron_quadform_shared_planes_f16x2 on the operands split as the rotation convolutions leave them: u with one scale,
    v with one scale per sample (``per_image``) or one for the tensor"""
    C, B, Do, L = ops.u.shape
    us = K.split_f16x2(ops.u.reshape(C * B, Do, L).contiguous())
    vs = K.split_images_f16x2(ops.v) if per_image else K.split_f16x2(ops.v)
    if fvar is None:
        fvar = torch.zeros(B, C, C, device=ops.u.device)
    return K.kron_quadform_shared_planes(us, vs, ops.l1, ops.l2, ops.delta, fvar, C)


def sample_major(u):
    return u.permute(1, 0, 2, 3).contiguous()


def run_fp32(K, ops, route, fvar=None, u=None):
    """the fp32-operand quadratic forms; ``u``: the operand already laid out for the route (e.g. a misaligned copy)"""
    C, B = ops.u.shape[:2]
    if fvar is None:
        fvar = torch.zeros(B, C, C, device=ops.u.device)
    if route == "kron-seedmajor":
        return K.kron_quadform_shared(ops.u if u is None else u, ops.v, ops.l1, ops.l2, ops.delta, fvar, seed_major=True)
    u = sample_major(ops.u) if u is None else u
    if route == "kron":
        return K.kron_quadform_shared(u, ops.v, ops.l1, ops.l2, ops.delta, fvar)
    return K.diag_quadform_shared(u, ops.v, ops.var_w, fvar)


def run_diag_ggn(K, ops, alpha=1.0, h=None):
    Do, Dk = ops.u.shape[2], ops.v.shape[1]
    if h is None:
        h = torch.zeros(Do * Dk, device=ops.u.device)
    return K.diag_ggn_shared(sample_major(ops.u), ops.v, alpha, h)


def grid_operand_weights(ops, mode):
    """(w0, w1) as the grid kernels take them"""
    return (grid_diag_h(ops.l1, ops.l2), None) if mode == 2 else (ops.l1, ops.l2)


def run_grid(K, ops, mode, seed_major, deltas):
    C, B = ops.u.shape[:2]
    w0, w1 = grid_operand_weights(ops, mode)
    var = torch.zeros(deltas.numel(), B, C, device=ops.u.device)
    return K.quadform_shared_grid(ops.u if seed_major else sample_major(ops.u), ops.v, w0, w1, deltas, mode, var,
                                  seed_major=seed_major)


def linear_operands(C, B, Do, Di, seed, spectrum):
    """the nn.Linear layer of the same draw (one position): ``u [C, B, Do]``, ``v [B, Di]``, a bias block ``ub``, ``wb``"""
    ops = operands(C, B, Do, Di, 1, seed, spectrum)
    ops.ub = operands(C, B, Do, 1, 1, seed + 1).u[..., 0].contiguous()
    ops.wb = ops.flat_l1.clone()
    ops.u, ops.v = ops.u[..., 0].contiguous(), ops.v[..., 0].contiguous()
    return ops


def run_linear_grid(K, ops, mode, bias, deltas):
    C, B = ops.u.shape[:2]
    w0, w1 = grid_operand_weights(ops, mode)
    var = torch.zeros(deltas.numel(), B, C, device=ops.u.device)
    return K.quadform_linear_grid(ops.u, ops.v, w0.reshape(-1) if mode == 2 else w0, w1, deltas, mode, var,
                                  ops.ub if bias else None, ops.wb if bias else None)


def row_seed(row):
    """one seed per row, stable under reordering of the table"""
    import zlib

    return zlib.crc32(row_id(row).encode()) % (1 << 31)
