"""Shape table, float64 reference and error bounds of the nn.RMSNorm forward and VJP kernels (csrc/lk_rmsnorm.hip), and the small
LLaMA network of the end-to-end tests - shared by tests/test_rmsnorm_fixtures.py (CPU: the table reaches every launch variant; the
bounds hold for an fp32 evaluation of the formulas and fail for two mutants), tests/emulated_rmsnorm_kernels.py,
tests/test_sweep_llama.py and tests/test_gpu_rmsnorm.py (the kernels themselves).

TEST INFRASTRUCTURE.  A case is ``dict(S, rows, D, w, off)``: ``w`` in ``"rand"`` (entries of either sign and, from ``D = 2``, one
zero) or ``"none"`` (null pointer); ``off``: every tensor starts one float past a 16-byte boundary (forces 4-byte loads).  The
shapes are the smallest at which a path can go wrong: the number of vectors of a row (``D``, or ``D / 4`` with 16-byte loads) at
every doubling of the lane group 2 .. 64 and one to either side, around the limit of the on-chip path (64 lanes of ``RMS_NV``
vectors) one vector to either side, one, two, three and nine seeds (``RMS_SC`` = 2 in flight), one to three rows, and one shape per
path with enough rows (2048) that the seeds are not split over grid.y.

THE BOUNDS hold for ANY order of the sums, with or without fused multiply-adds, in the unit round-off ``U = 2^-24`` (first order,
with one or two ``U`` of slack for the second-order terms: ``N U < 2e-4`` here).
  forward: every ``x^2`` is rounded once and the ``N`` non-negative terms are summed with at most ``N - 1`` roundings, so the sum is
    off by at most ``N U`` of itself - no cancellation, unlike a variance; the division by ``N`` and the addition of ``eps >= 0`` add
    ``U`` each, the square root halves that and adds ``U``, the reciprocal adds ``U``:  ``|d rstd| <= rstd (N / 2 + 5) U``.
    ``y = w (x rstd)`` adds two roundings.
  VJP (``x``, ``rstd``, ``w``, ``g`` as given, in fp32): ``t = w g`` and ``xh = x rstd`` carry one rounding each - ``xh`` is formed
    inside the kernel, so its rounding is counted -, their product a third; the sum of ``N`` terms of either sign is off by at
    most ``(N - 1) U sum|t xh|``, the division by ``N`` adds ``U |m2|``:  ``|d m2| <= (N + 3) U mean|t xh|``.  Then
    ``dx = rstd (t - xh m2)``: ``U |t|`` from ``t``, ``2 U |xh m2| + |xh| |d m2|`` from the product, ``U (|t| + |xh m2|)`` from the
    difference and ``U |dx|`` from the last product, with ``|m2| <= mean|t xh|``:
    ``|d dx| <= U rstd (4 |t| + (N + 8) |xh| mean|t xh|)``.
"""
from __future__ import annotations

import os
import re

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RMS_SC, RMS_NV = 2, 8  # the kernel's constants (checked against the source by tests/test_rmsnorm_fixtures.py)
ROW_LANES = 64  # most lanes of a row
U = 2.0 ** -24
EPS = 1e-6


def kernel_constants() -> dict:
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_rmsnorm.hip")).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (RMS_\w+) = (\d+);", text)}


def _case(S, rows, D, w="rand", off=0):
    return dict(S=S, rows=rows, D=D, w=w, off=off)


def _around(values):
    return sorted({v + d for v in values for d in (-1, 0, 1) if v + d >= 1})


def _table():
    cases = []
    # vectors per row nvec = D (4-byte loads) or D / 4 (16-byte loads): the lane group doubles at nvec = 2, 4, .. 64 and the row
    # leaves the registers above 64 * RMS_NV vectors
    edges = _around([2, 4, 8, 16, 32, ROW_LANES, ROW_LANES * RMS_NV])
    for i, nvec in enumerate(edges):
        S, rows, w = (1, 2, 3, 9)[i % 4], (1, 2, 3)[i % 3], ("rand", "none")[i % 5 == 4]
        # 4-byte loads: D = nvec (a misaligned pointer where D is a multiple of 4); 16-byte loads: D = 4 * nvec
        cases.append(_case(S, rows, nvec, w, off=1 if nvec % 4 == 0 else 0))
        cases.append(_case((1, 2, 3, 9)[(i + 1) % 4], (1, 2, 3)[(i + 1) % 3], 4 * nvec, w))
    # every number of seeds and of rows on one small shape of each load width, without and with weight; a misaligned vector shape
    for S in (1, RMS_SC, RMS_SC + 1, 9):
        for rows in (1, 2, 3):
            cases.append(_case(S, rows, 12, "none" if (S + rows) % 2 else "rand"))
            cases.append(_case(S, rows, 7, "rand" if (S + rows) % 2 else "none"))
    cases += [_case(3, 2, 64, off=1), _case(9, 3, 4 * (ROW_LANES * RMS_NV + 1), off=1),
              _case(3, 2, 4 * (ROW_LANES * RMS_NV + 1)), _case(2, 5, 192)]
    # one vector per row (a lane group of one lane) with several seeds
    cases += [_case(3, 2, 1), _case(RMS_SC, 3, 4)]
    # enough rows that the seeds are NOT split over grid.y although S > 1 (rows of 64 lanes: 4 per workgroup, 512 workgroups):
    # on chip / two-pass, 16-byte / 4-byte loads
    on = ROW_LANES * RMS_NV
    cases += [_case(2, 2048, 4 * ROW_LANES, "none"), _case(2, 2048, ROW_LANES + 1), _case(2, 2048, 4 * (on + 1), "none"),
              _case(2, 2048, on + 1)]
    seen, out = set(), []
    for c in cases:
        key = tuple(sorted(c.items()))
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


CASES = _table()


def case_id(c) -> str:
    return f"S{c['S']}-rows{c['rows']}-D{c['D']}-w{c['w']}-off{c['off']}"


def make_weight(c, gen, device="cpu"):
    """``w`` ``[D]`` with a negative entry and (from ``D = 2``) a zero, or None"""
    if c["w"] == "none":
        return None
    w = torch.randn(c["D"], generator=gen).to(device)
    w[-1] = -abs(w[-1]) - 0.5
    if c["D"] > 1:
        w[0] = 0.0
    return w


def make_inputs(c, gen, device="cpu"):
    """``(x [rows, D], g [S, rows, D], w)`` in fp32, drawn as ``randn + 3``: a row mean far from zero is what tells the mean of
    squares from a variance, and ``mean_row(t) != 0`` what tells the VJP from LayerNorm's"""
    x = (torch.randn(c["rows"], c["D"], generator=gen) + 3.0).to(device)
    g = (torch.randn(c["S"], c["rows"], c["D"], generator=gen) + 3.0).to(device)
    return x, g, make_weight(c, gen, device)


def forward_reference(x, w, eps=EPS):
    """float64 from the fp32 inputs (``eps`` as the fp32 value the kernel receives): dict of ``y`` ``[rows, D]``, ``rstd``
    ``[rows]`` and their bounds ``b_y``, ``b_rstd``"""
    eps = float(torch.tensor(eps, dtype=torch.float32))
    xd, N = x.double(), x.shape[-1]
    rstd = 1.0 / torch.sqrt((xd * xd).mean(-1) + eps)
    y = xd * rstd.unsqueeze(-1)
    if w is not None:
        y = y * w.double()
    rel = (N / 2 + 5) * U
    return dict(y=y, rstd=rstd, b_rstd=rstd * rel, b_y=y.abs() * (rel + 2 * U))


def vjp_reference(g, x, rstd, w):
    """float64 from the fp32 inputs ``g [S, rows, D]``, ``x [rows, D]``, ``rstd [rows]`` (the fp32 values the forward wrote):
    ``(dx, bound)``, each ``[S, rows, D]``"""
    N = x.shape[-1]
    t = g.double() if w is None else g.double() * w.double()
    rs = rstd.double().unsqueeze(-1)
    xh = x.double() * rs
    m2 = (t * xh).mean(-1, keepdim=True)
    dx = rs * (t - xh * m2)
    bound = U * rs * (4 * t.abs() + (N + 8) * xh.abs() * (t * xh).abs().mean(-1, keepdim=True))
    return dx, bound


# ---- fp32 evaluations of the formulas, and the mutants the bounds must catch -----------------------------------------------------
def forward_fp32(x, w, eps=EPS, mutant=None):
    """``(y, rstd)`` in fp32.  MUTANT ``"centred"``: LayerNorm's statistics - the variance about the row mean instead of the mean
    of squares"""
    if mutant == "centred":
        d = x - x.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt((d * d).mean(-1) + eps)
    else:
        rstd = 1.0 / torch.sqrt((x * x).mean(-1) + eps)
    y = x * rstd.unsqueeze(-1)
    return (y if w is None else w * y), rstd


def vjp_fp32(g, x, rstd, w, mutant=None):
    """``dx [S, rows, D]`` in fp32.  MUTANT ``"mean-term"``: LayerNorm's VJP, which also subtracts ``mean_row(t)``"""
    t = g if w is None else g * w
    rs = rstd.unsqueeze(-1)
    xh = x * rs
    inner = t - xh * (t * xh).mean(-1, keepdim=True)
    if mutant == "mean-term":
        inner = inner - t.mean(-1, keepdim=True)
    return rs * inner


def violations(c, y, rstd, dx, x, g, w, eps=EPS):
    """what the outputs of a case break of the criteria (an empty list: none): ``y``, ``rstd`` inside the forward's bounds, ``dx``
    inside the VJP's bounds on the fp32 ``rstd`` that it was given.  A NaN fails."""
    out = []
    ref = forward_reference(x.cpu(), None if w is None else w.cpu(), eps)
    if rstd is not None:
        err = (rstd.cpu().double() - ref["rstd"]).abs()
        if not bool((err <= ref["b_rstd"]).all()):
            out.append(f"rstd off by {float((err / ref['b_rstd']).max()):.2f} of its bound")
    if y is not None:
        err = (y.cpu().double() - ref["y"]).abs()
        if not bool((err <= ref["b_y"]).all()):
            out.append(f"y off by {float((err / ref['b_y'].clamp_min(1e-300)).max()):.2f} of its bound")
    if dx is not None:
        rs32 = rstd.cpu() if rstd is not None else ref["rstd"].float()
        want, bound = vjp_reference(g.cpu(), x.cpu(), rs32, None if w is None else w.cpu())
        err = (dx.cpu().double().reshape(want.shape) - want).abs()
        if not bool((err <= bound).all()):
            out.append(f"dx off by {float((err / bound.clamp_min(1e-300)).max()):.2f} of its bound")
    return out


# ---- end-to-end fixture -------------------------------------------------------------------------------------------------------------
# A ViTLlama of dim 32 with two heads (head dim 16, rotary halves of 8) on 8 x 12 images in six patches (T = 6), one block, 85
# hidden units, B = 5, three classes.  SiLU and softmax only: nothing is decided by a sign or sits near a tie, so fp32 against
# float64 holds at the project's 1e-4 without a lattice.
E2E_CLASSES = 3


def rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return (got - want).abs().max().item() / (want.abs().max().item() + 1e-30)


def llama_fixture(dim=32, depth=1, heads=2, B=5, classes=E2E_CLASSES, seed=52, track_norm=False):
    """``(float64 CPU model, X, y)``: a small ViTLlama, deterministic; ``track_norm``: the RMSNorm weights (drawn around one, so that
    they matter) are Laplace parameters"""
    from laplace_amd.nets import ViTLlama

    prev = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        m = ViTLlama(classes, image=(8, 12), patch=4, dim=dim, depth=depth, heads=heads, freeze_norm=not track_norm).double().eval()
        for mod in m.modules():
            if isinstance(mod, nn.RMSNorm):
                mod.weight.data.uniform_(0.7, 1.3)
    finally:
        torch.random.set_rng_state(prev)
    gen = torch.Generator().manual_seed(seed)
    return m, torch.randn(B, 3, 8, 12, generator=gen).double(), torch.randint(classes, (B,), generator=gen)
