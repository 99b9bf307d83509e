"""Shapes, inputs, references and acceptance criteria for the product kernel (csrc/lk_mul.hip) and the small squeeze-and-excitation
/ SwiGLU networks of the end-to-end tests - shared by tests/test_mul_fixtures.py (CPU: the table reaches every path, the criteria
bite), tests/emulated_mul_kernels.py (the kernel emulation states its rule through `torch_math`), tests/test_sweep_mul.py and
tests/test_gpu_mul.py (the device).

A kernel case is a dict: ``row`` (the row-gate form: ``b`` is ``[R]``; else the full form, ``b`` is ``[R, L]``), seeds ``S``, rows
``R``, row length ``L``, ``off`` (1: every buffer starts one element past an aligned address, which forces the 4-byte path),
``want`` (``"da"``, ``"db"`` or ``"both"``) and ``wide`` (an element offset passes 2^31: checked by shape only, never run).  The
shapes are the smallest at which a path can go wrong: L in {1, 3, 4, 49, 64, 256, 260} and the L that give a row 2, 8 and 32 lanes,
the resident limit of a row (8 vectors on each of 64 lanes: 2048 floats with 16-byte loads, 512 with 4-byte ones) and the first L
past it, 4096 (the longest), one row and five, a row count that is no multiple of the rows of a workgroup, more than one workgroup,
one row / one vector past a full stride of the grid (2048 workgroups), one to nine seeds, few rows (the seeds go over grid.y), no
rows at all.
"""
import torch
from torch import nn

from tests.slice_fixtures import E2E_CLASSES, _seeded, rel, run_curvature_checks, taps  # noqa: F401  (shared with the slicing tests)

MAX_BLOCKS = 2048  # STREAM_MAX_BLOCKS of csrc/lk_stream.h
RESIDENT_VECTORS = 64 * 8  # vectors of a row that stay in registers (64 lanes x MUL_NV)


def _case(row, S, R, L, off=0, want="both", wide=False):
    return dict(row=bool(row), S=S, R=R, L=L, off=off, want=want, wide=wide)


CASES = [
    # ---- the row gate ---------------------------------------------------------------------------------------------------------------
    # every L of the list (1, 2, 4 lanes; 64 lanes with 4-byte loads; 16 and 64 lanes with one and with two vectors per lane)
    *[_case(1, 3, 5, L) for L in (1, 3, 4, 49, 64, 256, 260)],
    *[_case(1, 3, 5, L) for L in (8, 32, 128)],  # 2, 8 and 32 lanes per row
    *[_case(1, 3, 5, L, off=1) for L in (4, 64, 256)],  # an unaligned base: the 4-byte path on multiples of four
    _case(1, 1, 1, 3), _case(1, 9, 1, 64), _case(1, 9, 1, 260, off=1),  # one row; nine seeds over grid.y
    *[_case(1, 3, 5, L, want=w) for L in (49, 64) for w in ("da", "db")],
    # the resident limit and one vector past it, on both paths; the longest row
    _case(1, 3, 5, 2048), _case(1, 3, 5, 2052), _case(1, 3, 5, 511), _case(1, 3, 5, 513), _case(1, 1, 1, 513, want="db"),
    _case(1, 3, 1, 4096), _case(1, 3, 5, 4096, off=1, want="db"),
    # rows that do not fill the last workgroup (4 rows of 64 lanes each), two workgroups of one-lane rows
    _case(1, 3, 67, 49), _case(1, 3, 257, 4), _case(1, 9, 67, 64, want="da"),
    # one row past a full stride of the grid (2048 workgroups of 4 rows), on both paths
    _case(1, 1, 4 * MAX_BLOCKS + 1, 49), _case(1, 1, 4 * MAX_BLOCKS + 1, 132),
    _case(1, 3, 0, 64),
    # ---- the full form --------------------------------------------------------------------------------------------------------------
    *[_case(0, S, R, L) for (S, R, L) in ((1, 1, 1), (3, 5, 3), (9, 1, 4), (3, 5, 49), (9, 5, 64), (1, 5, 260), (3, 1, 256))],
    _case(0, 3, 5, 64, off=1), _case(0, 9, 1, 4, off=1),
    *[_case(0, 3, 5, L, want=w) for L in (49, 64) for w in ("da", "db")],
    _case(0, 3, 5, 4096), _case(0, 1, 67, 513),
    # one vector past a full stride of the grid (2048 workgroups of 256 lanes), on both paths
    _case(0, 1, 174763, 12), _case(0, 1, 174763, 3),  # (3 x 174763 = 2048 x 256 + 1)
    _case(0, 3, 0, 64),
    # ---- an element offset passes 2^31 (by shape only) ----------------------------------------------------------------------------------
    _case(1, 9, 1 << 20, 256, wide=True), _case(0, 9, 1 << 20, 256, wide=True), _case(1, 9, 1 << 22, 63, wide=True),
]


def case_id(c):
    return (f"{'row' if c['row'] else 'full'}-S{c['S']}-R{c['R']}-L{c['L']}-{c['want']}" + ("-unaligned" if c["off"] else "")
            + ("-wide" if c["wide"] else ""))


def wants(c):
    return c["want"] in ("da", "both"), c["want"] in ("db", "both")


def full_mantissa(shape, gen):
    """fp32 values ``+-m 2^e`` with ``m`` a full 24-bit mantissa in [1, 2) and ``e`` in [-10, 9]: magnitudes in [2^-10, 2^10), mixed
    signs; no product of two of them leaves [2^-20, 2^20)"""
    m = 1.0 + torch.randint(0, 1 << 23, shape, generator=gen).double() * 2.0 ** -23
    e = torch.randint(-10, 10, shape, generator=gen).double()
    sign = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    return (sign * m * torch.exp2(e)).float()


def make_inputs(c, gen):
    """``(g [S, R, L], a [R, L], b [R, L] or [R])`` of a case on the CPU"""
    S, R, L = c["S"], c["R"], c["L"]
    return full_mantissa((S, R, L), gen), full_mantissa((R, L), gen), full_mantissa((R,) if c["row"] else (R, L), gen)


def vjp_reference(g, a, b, row):
    """fp64: ``da = g * b`` (``b[r]`` for a row gate), ``db = g * a`` - summed over ``l`` for a row gate -, and ``mag = sum_l |g * a|``
    (what the bound of a row sum is relative to)"""
    g, a, b = g.double(), a.double(), b.double()
    prod = g * a
    return dict(da=g * (b[:, None] if row else b), db=prod.sum(-1) if row else prod, mag=prod.abs().sum(-1))


MUTANTS = ("wrong-sample", "dropped-tail", "swapped", "fp16-sum")


def torch_math(g, a, b, row, want=(True, True), mutant=None):
    """``(da, db)`` by the rule of lk_mul_vjp_f32 in torch fp32 (``None`` for an output that is not wanted).  MUTANTS:
    ``"wrong-sample"`` takes the row of ``b`` from the seed-major row ``s R + r`` of ``g`` (seed ``s`` reads the gate ``s`` rows on);
    ``"dropped-tail"`` leaves the last ``L % 4`` elements of a row out (NaN in ``da`` and in an element-wise ``db``, missing from a
    row sum); ``"swapped"`` hands ``g * a`` out as ``da`` and ``g * b`` as ``db`` (full form); ``"fp16-sum"`` accumulates the row sum
    in fp16."""
    S, R, L = g.shape
    bs = b.unsqueeze(0).expand(S, *b.shape)
    if mutant == "wrong-sample" and R:
        bs = torch.stack([b.roll(-s, 0) for s in range(S)])
    be = bs[:, :, None] if row else bs
    first, second = (a, be) if mutant == "swapped" and not row else (be, a)
    da, prod = g * first, g * second
    if row:
        if mutant == "fp16-sum":
            db = prod.half().sum(-1, dtype=torch.float16).float()
        else:
            db = (prod[:, :, :L - L % 4] if mutant == "dropped-tail" else prod).sum(-1)
    else:
        db = prod.clone()
    if mutant == "dropped-tail" and L % 4:
        da[:, :, L - L % 4:] = float("nan")
        if not row:
            db[:, :, L - L % 4:] = float("nan")
    return (da if want[0] else None), (db if want[1] else None)


def violations(c, da, db, ref):
    """what the outputs of a case break of the device test's criteria (an empty list: none): ``da``, and ``db`` of the full form,
    are the fp32 product - the exact fp64 product rounded once - bit for bit; ``db`` of a row gate lies within
    ``(L + 1) 2^-24 sum_l |g a|`` of the exact sum (any order of the sum, products fused into it or not)"""
    out, (want_da, want_db) = [], wants(c)
    if (da is not None) != want_da or (db is not None) != want_db:
        return [f"outputs {da is not None, db is not None} for want = {c['want']}"]
    if want_da and not torch.equal(da.cpu().reshape(ref["da"].shape), ref["da"].float()):
        out.append("da is not the fp32 product g * b")
    if want_db and not c["row"] and not torch.equal(db.cpu().reshape(ref["db"].shape), ref["db"].float()):
        out.append("db is not the fp32 product g * a")
    if want_db and c["row"]:
        err = (db.cpu().double().reshape(ref["db"].shape) - ref["db"]).abs()
        bound = (c["L"] + 1) * 2.0 ** -24 * ref["mag"]
        if not bool((err <= bound).all()):  # (a NaN fails)
            out.append(f"db: row sum off by {float((err / ref['mag']).max()):.3e} of sum|g a| (bound {(c['L'] + 1) * 2.0 ** -24:.3e})")
    return out


# ---- end-to-end fixtures ---------------------------------------------------------------------------------------------------------
# An SEResNetSmall of widths 8 / 16 with one block per stage on 8 x 8 inputs, B = 4, tanh (row gates [4, 8, 1, 1] on 8 x 8 maps and
# [4, 16, 1, 1] on 4 x 4 ones); a ViTSwiGLU of dim 32 on 4 x 20 images in five patches (T = 5), 85 hidden units, B = 3 (the full
# form on [3, 5, 85], which is no multiple of four).  Smooth activations only: nothing is decided by a sign, so fp32 against
# float64 holds at the project's 1e-4 without a lattice.
def se_fixture(widths=(8, 16), depth=1, B=4, hw=8, classes=E2E_CLASSES, seed=41):
    """``(float64 CPU model, X, y)``: a small SEResNetSmall (tanh), deterministic"""
    from laplace_amd.nets import SEResNetSmall

    m = _seeded(seed, lambda: SEResNetSmall(classes, widths=widths, depth=depth, act=nn.Tanh))
    gen = torch.Generator().manual_seed(seed)
    return m, torch.randn(B, 3, hw, hw, generator=gen).double(), torch.randint(classes, (B,), generator=gen)


def swiglu_fixture(dim=32, depth=1, heads=2, B=3, classes=E2E_CLASSES, seed=42):
    """``(float64 CPU model, X, y)``: a small ViTSwiGLU (4 x 20 images in five patches: T = 5)"""
    from laplace_amd.nets import ViTSwiGLU

    m = _seeded(seed, lambda: ViTSwiGLU(classes, image=(4, 20), patch=4, dim=dim, depth=depth, heads=heads))
    gen = torch.Generator().manual_seed(seed)
    return m, torch.randn(B, 3, 4, 20, generator=gen).double(), torch.randint(classes, (B,), generator=gen)
