"""Shapes, inputs, references and acceptance criteria for the softmax and matrix-product VJP kernels (csrc/lk_softmax.hip,
csrc/lk_matmul.hip) and the small hand-written-attention transformer of the end-to-end tests - shared by
tests/test_eager_attn_fixtures.py (CPU: the tables reach every launch path, the criteria accept every order of an fp32 evaluation
and reject the mutants), tests/emulated_softmax_kernels.py and tests/emulated_matmul_kernels.py (the emulations state the kernels'
rules through `softmax_math` / `matmul_math`), tests/test_sweep_eager_attn.py and tests/test_gpu_eager_attn.py (the device).

The criteria are bounds of the standard rounding-error analysis, ``u = 2^-24`` (Higham, Accuracy and Stability of Numerical
Algorithms, ch. 3: a sum of ``n`` fp32 terms in ANY order, with or without fused multiply-adds, errs by at most
``gamma_n sum|terms|``, ``gamma_n = n u / (1 - n u) <= (n + 1) u`` for the ``n <= 4096`` used here).

matmul.  An element is a dot product of depth ``D`` (``N`` for ``da``, ``M`` for ``db``): ``|got - exact| <= (D + 1) u sum|x||y|``.
On small-integer operands (|.| <= 8: every partial sum is an integer below 2^24) the result is exact: bit-equal.

softmax, ``dx = y (g - d)``, ``d = sum_j g_j y_j``, ``A = sum_j |g_j y_j|``:
  ``|d^ - d| <= (L + 1) u A``; the subtraction adds ``u |g - d^| <= u (|g| + A) + O(u^2)``; the product adds ``u |y| |g - d^|``:
  ``|dx^ - dx| <= u |y| ((L + 3) A + 2 |g|) + O(u^2)``.  The criterion is ``u |y| ((L + 4) A + 3 |g|) + 2^-149`` (the slack of one
  ``A`` and one ``|g|`` covers the second-order terms; 2^-149 is the gradual underflow of the last product).  It is zero where ``y``
  is zero: a masked key gets an exact zero.
log-softmax, ``dx = g - e s``, ``e = exp(y)``, ``s = sum_j g_j``, ``G = sum_j |g_j|``:
  ``|s^ - s| <= (L + 1) u G``; the device's ``expf`` errs by at most ``C_EXP u`` relative; the product (fused or not) adds
  ``u e |s|``, the subtraction ``u (|g| + e G)``: ``|dx^ - dx| <= u (e G (L + C_EXP + 3) + |g|) + O(u^2)``.  The criterion is
  ``u (e G (L + C_EXP + 4) + 2 |g|)``.
  ``C_EXP``: no ulp bound of the device's ``expf`` can be derived here, so it is twice the measured error of torch's CPU fp32 ``exp``
  against fp64 on the ``y`` of every log case of the table (`softmax_case_inputs`): measured 1.026 u, recorded as
  ``MEASURED_EXP_ERROR = 1.03`` and re-measured by tests/test_eager_attn_fixtures.py; ``C_EXP = 2.06``.

A softmax case is a dict: seeds ``S``, rows ``R``, row length ``L``, ``log``, ``off`` (1: every buffer starts one element past an
aligned address, which forces the 4-byte path), ``kind`` (``"random"``, ``"masked"``: a third of the keys of every row have
probability exactly zero, ``"saturated"``: one probability is exactly one, the others exactly zero) and ``wide`` (an element offset
passes 2^31: by shape only, never run).  A matmul case: ``S``, ``NB``, ``M``, ``K``, ``N``, ``want`` and ``wide``.
"""
import torch

from tests.mul_fixtures import full_mantissa
from tests.slice_fixtures import E2E_CLASSES, _seeded, rel, run_curvature_checks, taps  # noqa: F401  (shared with the slicing tests)

U = 2.0 ** -24
SMX_MAX_BLOCKS = 2048  # STREAM_MAX_BLOCKS of csrc/lk_stream.h
MM_RES_DEPTH = 128  # MM_RES_DEPTH of csrc/lk_matmul.hip
#: twice the measured relative error, in units of u, of torch's CPU fp32 exp against fp64 on the log cases (see the docstring)
MEASURED_EXP_ERROR = 1.03
C_EXP = 2.0 * MEASURED_EXP_ERROR


# ---- softmax -------------------------------------------------------------------------------------------------------------------------
def _smx(S, R, L, log=False, off=0, kind="random", wide=False):
    return dict(S=S, R=R, L=L, log=bool(log), off=off, kind=kind, wide=wide)


SOFTMAX_CASES = [
    # every L of the list on both forms: 1, 2 (scalar: 4), 16, 64 lanes; the scalar path where L is no multiple of four
    *[_smx(2, 5, L, log) for L in (1, 3, 4, 5, 63, 64, 65, 255, 256, 257) for log in (False, True)],
    *[_smx(2, 5, L, off=1) for L in (4, 64, 256)],  # an unaligned base: the 4-byte path on multiples of four
    _smx(2, 5, 64, log=True, off=1),
    _smx(2, 5, 2), _smx(2, 5, 8), _smx(2, 5, 128), _smx(2, 5, 18, log=True),  # 2 and 32 lanes per row, on both paths
    # either side of the resident limit (8 vectors on each of 64 lanes: 2048 floats with 16-byte loads, 512 with 4-byte ones)
    _smx(2, 3, 2048), _smx(2, 3, 2052), _smx(2, 3, 2048, log=True), _smx(2, 3, 2052, log=True),
    _smx(2, 3, 511), _smx(2, 3, 513), _smx(2, 3, 512, off=1), _smx(2, 3, 516, off=1), _smx(2, 3, 511, log=True), _smx(2, 3, 513, log=True),
    # R: none, one, one either side of the rows of a workgroup (16 lanes per row: 16 rows; 64 lanes: 4 rows; one lane: 256 rows)
    _smx(2, 0, 64), _smx(1, 1, 64), _smx(2, 15, 64), _smx(2, 17, 64), _smx(2, 3, 256), _smx(9, 5, 256), _smx(1, 255, 4), _smx(2, 257, 4),
    # S in {1, 2, 9}; few rows and many seeds (the seeds go over grid.y); enough rows that they do not (512 workgroups)
    _smx(1, 5, 65), _smx(9, 5, 64), _smx(9, 1, 64, log=True), _smx(9, 1, 5), _smx(2, 2048, 256), _smx(2, 2048, 256, log=True),
    # one row past a full stride of the grid (2048 workgroups of 4 rows)
    _smx(1, 4 * SMX_MAX_BLOCKS + 1, 256),
    # masked keys and a saturated row, on the vector and the scalar path, resident and not
    _smx(2, 5, 64, kind="masked"), _smx(9, 5, 65, kind="masked"), _smx(2, 3, 2052, kind="masked"), _smx(2, 5, 64, kind="saturated"),
    _smx(2, 5, 5, kind="saturated"), _smx(2, 3, 513, kind="saturated"),
    # an element offset passes 2^31 (by shape only)
    _smx(9, 1 << 20, 256, wide=True), _smx(9, 1 << 22, 63, log=True, wide=True),
]


def softmax_case_id(c):
    return (f"{'log-' if c['log'] else ''}S{c['S']}-R{c['R']}-L{c['L']}-{c['kind']}" + ("-unaligned" if c["off"] else "")
            + ("-wide" if c["wide"] else ""))


def softmax_inputs(c, gen):
    """``(g [S, R, L], y [R, L])`` of a case on the CPU, fp32: ``y`` is the fp64 softmax (log-softmax) of random logits rounded once;
    a masked key has probability exactly zero, a saturated row one probability of exactly one"""
    S, R, L = c["S"], c["R"], c["L"]
    logits = torch.randn(R, L, generator=gen, dtype=torch.float64) * 2.0
    if c["kind"] == "masked" and L > 1:
        logits[:, torch.arange(L) % 3 == 1] = float("-inf")
    if c["kind"] == "saturated" and R:
        logits[torch.arange(R), torch.arange(R) % L] = 400.0
    y = torch.log_softmax(logits, -1) if c["log"] else torch.softmax(logits, -1)
    return full_mantissa((S, R, L), gen), y.float()


def softmax_case_inputs(i):
    """the inputs of ``SOFTMAX_CASES[i]`` as every test draws them"""
    return softmax_inputs(SOFTMAX_CASES[i], torch.Generator().manual_seed(11 + i))


def softmax_reference(g, y, log):
    """fp64 from the fp32 inputs: ``dx`` and what the bound is relative to"""
    g, y = g.double(), y.double()
    if log:
        e = torch.exp(y)
        return dict(dx=g - e * g.sum(-1, keepdim=True), e=e, G=g.abs().sum(-1, keepdim=True), g=g.abs())
    return dict(dx=y * (g - (g * y).sum(-1, keepdim=True)), y=y.abs(), A=(g * y).abs().sum(-1, keepdim=True), g=g.abs())


def softmax_bound(c, ref):
    """the criterion of the docstring, per element"""
    L = c["L"]
    if c["log"]:
        return U * (ref["e"] * ref["G"] * (L + C_EXP + 4) + 2 * ref["g"])
    return U * ref["y"] * ((L + 4) * ref["A"] + 3 * ref["g"]) + 2.0 ** -149


def measured_exp_error(ys):
    """largest relative error, in units of u, of torch's CPU fp32 ``exp`` against fp64 on the fp32 tensors ``ys``"""
    worst = 0.0
    for y in ys:
        if y.numel():
            want = torch.exp(y.double())
            err = ((torch.exp(y).double() - want).abs() / want)
            worst = max(worst, float(err[want > 2.0 ** -100].max()) / U)
    return worst


ORDERS = ("forward", "reversed", "pairwise")


def _ordered_sum(t, order):
    """fp32 sum over the last dim of ``t`` in a fixed order: one accumulator walking forward or backward, or pairwise halves"""
    n = t.shape[-1]
    if n == 0:
        return t.new_zeros(t.shape[:-1])
    if order == "pairwise":
        while t.shape[-1] > 1:
            if t.shape[-1] % 2:
                t = torch.cat([t[..., :-2], t[..., -2:-1] + t[..., -1:]], -1)
            t = t[..., 0::2] + t[..., 1::2]
        return t[..., 0]
    idx = range(n) if order == "forward" else range(n - 1, -1, -1)
    acc = torch.zeros_like(t[..., 0])
    for i in idx:
        acc = acc + t[..., i]
    return acc


SOFTMAX_MUTANTS = ("no-sum", "dot-without-y", "log-y-for-exp")


def softmax_math(g, y, log, order="forward", mutant=None):
    """``dx`` by the rule of lk_softmax_vjp_f32 in torch fp32, the row sum in ``order``.  SOFTMAX_MUTANTS: ``"no-sum"`` leaves the
    ``- sum g y`` term out (``y * g``), ``"dot-without-y"`` subtracts ``sum g`` for ``sum g y``, ``"log-y-for-exp"`` multiplies the
    log form's sum by ``y`` for ``exp(y)``."""
    S, R, L = g.shape
    if log:
        p = y if mutant == "log-y-for-exp" else torch.exp(y)
        return g - p * _ordered_sum(g, order).unsqueeze(-1)
    if mutant == "no-sum":
        return y * g
    d = _ordered_sum(g if mutant == "dot-without-y" else g * y, order).unsqueeze(-1)
    return y * (g - d)


def softmax_violations(c, dx, ref):
    """what ``dx`` breaks of the device test's criterion (an empty list: nothing); a NaN fails"""
    err = (dx.cpu().double().reshape(ref["dx"].shape) - ref["dx"]).abs()
    bound = softmax_bound(c, ref)
    if bool((err <= bound).all()):
        return []
    worst = float((err / bound.clamp_min(1e-300))[~(err <= bound)].max()) if bool(torch.isfinite(err).all()) else float("nan")
    return [f"dx: {int((~(err <= bound)).sum())} elements past the bound, the worst by a factor of {worst:.3g}"]


# ---- matmul --------------------------------------------------------------------------------------------------------------------------
def _mm(S, NB, M, K, N, want="both", wide=False):
    return dict(S=S, NB=NB, M=M, K=K, N=N, want=want, wide=wide)


MATMUL_CASES = [
    # M, K, N from {1, 2, 31, 32, 33, 63, 64, 65, 129}: every tile edge (32 per wave, 64 per workgroup) and the resident limit of the
    # reduction depth (128: N for da, M for db) is crossed on each side; NB in {1, 3}, S in {1, 2, 5}
    _mm(1, 1, 1, 1, 1), _mm(2, 3, 2, 31, 33), _mm(5, 1, 31, 2, 32), _mm(2, 3, 32, 33, 2), _mm(5, 3, 33, 32, 31), _mm(2, 1, 63, 65, 64),
    _mm(2, 3, 64, 63, 65), _mm(5, 1, 65, 64, 63), _mm(2, 1, 129, 1, 2), _mm(2, 3, 2, 64, 129), _mm(2, 1, 129, 65, 129), _mm(1, 3, 64, 129, 64),
    _mm(5, 3, 64, 64, 64), _mm(2, 1, 1, 129, 1), _mm(2, 3, 128, 2, 128),
    # one output only (the other pointer is null), resident and not
    _mm(2, 3, 33, 32, 31, want="da"), _mm(2, 3, 33, 32, 31, want="db"), _mm(2, 1, 129, 65, 129, want="da"), _mm(2, 1, 129, 65, 129, want="db"),
    # enough sample matrices that the seeds are not split over grid.y (512 workgroups); none at all
    _mm(2, 512, 2, 2, 2), _mm(2, 0, 4, 4, 4),
    # an element offset passes 2^31 (by shape only)
    _mm(9, 1 << 15, 256, 64, 256, wide=True),
]


def matmul_case_id(c):
    return f"S{c['S']}-NB{c['NB']}-M{c['M']}-K{c['K']}-N{c['N']}-{c['want']}" + ("-wide" if c["wide"] else "")


def matmul_wants(c):
    return c["want"] in ("da", "both"), c["want"] in ("db", "both")


def matmul_inputs(c, gen, ints=False):
    """``(g [S, NB, M, N], a [NB, M, K], b [NB, K, N])`` of a case on the CPU, fp32: full 24-bit mantissas, or integers in [-8, 8]"""
    shapes = ((c["S"], c["NB"], c["M"], c["N"]), (c["NB"], c["M"], c["K"]), (c["NB"], c["K"], c["N"]))
    if ints:
        return tuple(torch.randint(-8, 9, s, generator=gen).float() for s in shapes)
    return tuple(full_mantissa(s, gen) for s in shapes)


def matmul_case_inputs(i, ints=False):
    """the inputs of ``MATMUL_CASES[i]`` as every test draws them"""
    return matmul_inputs(MATMUL_CASES[i], torch.Generator().manual_seed(101 + 2 * i + int(ints)), ints)


def matmul_reference(g, a, b):
    """fp64 from the fp32 inputs: ``da = g b^T``, ``db = a^T g`` and the sums of absolute products the bounds are relative to"""
    g, a, b = g.double(), a.double(), b.double()
    return dict(da=g @ b.transpose(-1, -2), db=a.transpose(-1, -2) @ g, mag_da=g.abs() @ b.abs().transpose(-1, -2),
                mag_db=a.abs().transpose(-1, -2) @ g.abs())


MATMUL_MUTANTS = ("b-untransposed", "wrong-seed")


def matmul_math(g, a, b, want=(True, True), order="forward", mutant=None):
    """``(da, db)`` by the rule of lk_matmul_vjp_f32 in torch fp32, every dot product summed in ``order`` (``None``: torch's own
    matmul).  MATMUL_MUTANTS: ``"b-untransposed"`` forms ``da = g b`` (square ``b`` only), ``"wrong-seed"`` takes ``db`` of seed ``s``
    from the cotangent of seed ``s + 1``."""
    S = g.shape[0]
    da = db = None
    if want[0]:
        bt = b if mutant == "b-untransposed" and b.shape[-1] == b.shape[-2] else b.transpose(-1, -2)  # [NB, N, K]
        if order is None:
            da = g @ bt
        else:  # [S, NB, M, K, N]: the products of a dot, summed over the last dim
            da = _ordered_sum(g.unsqueeze(-2) * bt.transpose(-1, -2).unsqueeze(-3), order)
    if want[1]:
        gs = g.roll(-1, 0) if mutant == "wrong-seed" and S > 1 else g
        if order is None:
            db = a.transpose(-1, -2) @ gs
        else:  # [S, NB, K, N, M]
            db = _ordered_sum(a.transpose(-1, -2).unsqueeze(-2) * gs.transpose(-1, -2).unsqueeze(-3), order)
    return da, db


def matmul_violations(c, da, db, ref, ints=False):
    """what the outputs of a case break of the device test's criteria (an empty list: nothing): bit-equal to the exact result on
    small-integer operands, within ``(D + 1) u sum|x||y|`` of it on full-mantissa ones"""
    out, (want_da, want_db) = [], matmul_wants(c)
    if (da is not None) != want_da or (db is not None) != want_db:
        return [f"outputs {da is not None, db is not None} for want = {c['want']}"]
    for name, got, depth in (("da", da, c["N"]), ("db", db, c["M"])):
        if got is None:
            continue
        got = got.cpu().reshape(ref[name].shape)
        if ints:
            if not torch.equal(got, ref[name].float()):
                out.append(f"{name} is not the exact product on small integers")
            continue
        err, bound = (got.double() - ref[name]).abs(), (depth + 1) * U * ref["mag_" + name]
        if not bool((err <= bound).all()):  # (a NaN fails)
            out.append(f"{name}: off by {float((err / ref['mag_' + name]).max()):.3e} of sum|x||y| (bound {(depth + 1) * U:.3e})")
    return out


# ---- end-to-end fixture ---------------------------------------------------------------------------------------------------------
# A ViTEager of dim 32 with two heads (head dim 16) on 4 x 4T images in T patches, B = 3, GELU: nothing is decided by a sign, so
# fp32 against float64 holds at the project's 1e-4 without a lattice.  T = 5 (the scalar path of the softmax kernel, one wave's
# corner of a tile) and T = 17.
def vit_eager_fixture(T=5, rel_bias=True, dim=32, depth=1, heads=2, B=3, classes=E2E_CLASSES, seed=52, softmax_module=True):
    """``(float64 CPU model, X, y)``: a small ViTEager, deterministic"""
    from laplace_amd.nets import ViTEager

    m = _seeded(seed, lambda: ViTEager(classes, image=(4, 4 * T), patch=4, dim=dim, depth=depth, heads=heads, rel_bias=rel_bias,
                                       softmax_module=softmax_module))
    gen = torch.Generator().manual_seed(seed)
    return m, torch.randn(B, 3, 4, 4 * T, generator=gen).double(), torch.randint(classes, (B,), generator=gen)

