"""Shape table, float64 reference and error bounds of the GroupNorm / LayerNorm forward and VJP kernels
(csrc/lk_normvjp.hip), shared by tests/test_norm_sweep_fixtures.py (CPU: the table reaches every launch variant; the bounds
hold for a two-pass fp32 forward and fail for ``E[x^2] - mu^2``) and tests/test_gpu_norm_sweep.py (the kernels themselves).

TEST INFRASTRUCTURE.  A case is ``dict(S, B, L, Ch, G, layout, w, off)``: ``w`` in ``"rand"`` (entries of either sign and one
zero), ``"none"`` (null pointer); ``off``: every tensor starts one float past a 16-byte boundary (forces 4-byte loads).
"""
from __future__ import annotations

import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the kernel's constants (checked against the source by tests/test_norm_sweep_fixtures.py)
NVJP_SC, NVJP_NV, NVJP_WIDE, NVJP_TILE_LANES = 2, 8, 16, 16
ROW_LANES = 64  # most lanes of a statistics row
U = 2.0 ** -24


def kernel_constants() -> dict:
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_normvjp.hip")).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (NVJP_\w+) = (\d+);", text)}


def _case(S, B, L, Ch, G, layout, w="rand", off=0):
    return dict(S=S, B=B, L=L, Ch=Ch, G=G, layout=layout, w=w, off=off)


def _around(values):
    return sorted({v + d for v in values for d in (-1, 0, 1) if v + d >= 1})


def _table():
    cases = []
    # ---- ROW kernel: a lane group per row.  Vectors per row nvec = N (4-byte loads) or N / 4 (16-byte loads); the lane group
    # doubles at nvec = 2, 4, .. 64 and the row leaves the chip above 64 * NVJP_NV vectors
    edges = _around([2, 4, 8, 16, 32, ROW_LANES, ROW_LANES * NVJP_NV]) + [3]
    for layout in (0, 1):
        for i, nvec in enumerate(sorted(set(edges))):
            # 4-byte loads: N = nvec (a misaligned pointer where N is a multiple of 4); 16-byte loads: N = 4 * nvec
            for N, off in ((nvec, 1 if nvec % 4 == 0 else 0), (4 * nvec, 0)):
                if layout == 0 and i % 2 == 0:
                    cases.append(_case(3, 2, N, 2, 2, 0, off=off))  # Ch / G = 1: one channel per group, L = N positions
                elif layout == 0:
                    cases.append(_case(3, 2, 1, 3 * N, 3, 0, off=off))  # L = 1
                else:
                    cases.append(_case(3, 2, 1, 2 * N, 2, 1, off=off))  # LayerNorm-like rows of Ch / G contiguous floats
        # N = 4 through 16-byte loads, G = 1, B * G = 1, no affine, S in {1, SC - 1, SC + 1, 9}
        cases += [_case(1, 1, 4 if layout == 0 else 1, 1 if layout == 0 else 4, 1, layout, w="none"),
                  _case(NVJP_SC - 1, 1, 1, 12, 1, layout), _case(NVJP_SC + 1, 3, 5, 8, 1, layout, w="none"),
                  _case(9, 2, 7, 6, 3, layout), _case(9, 1, 1, 1, 1, layout)]
        # rows of several channels with L > 1 (layout 0: the channel of an element is e / L)
        cases += [_case(3, 2, 5, 12, 3, layout), _case(2, 2, 4, 8, 2, layout), _case(3, 1, 6, 6, 1, layout, off=1)]
    # layout 1, L > 1, at least NVJP_WIDE channels per group: the ROW kernel over runs of Ch / G floats
    W = NVJP_WIDE
    cases += [_case(3, 2, 3, 2 * W, 2, 1), _case(3, 2, 5, 20, 1, 1), _case(3, 2, 4, 17 * 2, 2, 1), _case(9, 1, 2, W, 1, 1, off=1),
              _case(2, 1, ROW_LANES * NVJP_NV * 4 // W, W, 1, 1), _case(2, 1, ROW_LANES * NVJP_NV * 4 // W + 1, 2 * W, 2, 1),
              _case(2, 1, ROW_LANES * NVJP_NV // W + 1, W + 1, 1, 1, w="none")]
    # ---- TILE kernel: layout 1, L > 1, fewer than NVJP_WIDE channels per group.  CXW lanes across the channel vectors, 256 / CXW
    # lane rows over the positions, NVJP_NV positions each on chip
    def tile(S, B, L, cpg, G, **kw):
        return _case(S, B, L, cpg * G, G, 1, **kw)

    def limit(cvt):  # positions that stay on chip with `cvt` channel vectors per workgroup
        p = 1
        while p < cvt:
            p *= 2
        return 256 // p * NVJP_NV

    cases += [tile(9, 4, 16, 2, 32),  # GroupNorm(32, 64) at L = 16
              tile(3, 2, 16, 2, 32, off=1), tile(1, 1, 5, 2, 32, w="none"),
              tile(3, 2, 3, 2, 64),  # two tiles of 32 groups
              tile(3, 2, 3, 2, 48),  # ... the last one with 16
              tile(3, 1, 4, 1, 8), tile(3, 1, 4, 1, 5), tile(3, 2, 2, 3, 4), tile(3, 2, 2, 3, 5), tile(2, 1, 3, 15, 8),
              tile(3, 2, 2, 4, 1), tile(9, 1, 2, 1, 1), tile(3, 1, 3, 1, 2), tile(3, 1, 3, 2, 2), tile(3, 1, 3, 1, 3, w="none"),
              tile(3, 1, 3, 2, 33), tile(1, 2, 7, 7, 3), tile(3, 1, 2, 4, 2), tile(3, 1, 2, 1, 16), tile(3, 1, 2, 5, 4),
              tile(3, 1, 2, 8, 4), tile(3, 1, 2, 15, 1)]
    for cpg, G, cvt_vec, cvt_sc in ((2, 32, 16, 16), (15, 8, 30, 30), (4, 1, 1, 4), (1, 1, None, 1), (8, 2, 4, 16), (1, 8, 2, 8),
                                    (2, 2, 1, 4), (1, 2, None, 2), (4, 8, 8, 16)):
        for cvt, off in ((cvt_vec, 0), (cvt_sc, 1)):
            if cvt is None:
                continue
            L0 = limit(cvt)
            cases += [tile(2, 1, L0 + d, cpg, G, off=off) for d in (-1, 0, 1)]
    # ---- enough rows that the seeds are NOT split over grid.y although S > 1 (512 workgroups), one per kernel and layout
    big, on = ROW_LANES * NVJP_NV * 4 + 4, ROW_LANES * NVJP_NV * 4  # (rows of 64 lanes: 4 per workgroup, 2048 rows)
    for layout in (0, 1):
        for N in (on, on // 4 - 1, big, big // 4):  # on chip / two-pass, 16-byte / 4-byte loads
            cases.append(_case(2, 2048, N if layout == 0 else 1, 1 if layout == 0 else N, 1, layout, w="none"))
    cases += [tile(2, 512, 2, 2, 32), tile(2, 512, 2, 2, 33), tile(2, 512, 2052, 4, 1, w="none"),
              tile(2, 512, 2049, 1, 1, off=1, w="none")]
    seen, out = set(), []
    for c in cases:
        key = tuple(sorted(c.items()))
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


CASES = _table()


def case_id(c) -> str:
    return f"S{c['S']}-B{c['B']}-L{c['L']}-Ch{c['Ch']}-G{c['G']}-lay{c['layout']}-w{c['w']}-off{c['off']}"


def shape_of(c):
    return (c["B"], c["Ch"], c["L"]) if c["layout"] == 0 else (c["B"], c["L"], c["Ch"])


# ---- rows view ----------------------------------------------------------------------------------------------------------------
def to_rows(t, G, layout):
    """``[.., B, Ch, L]`` / ``[.., B, L, Ch]`` -> ``[.., B, G, N]`` (the order inside a row does not matter to any statistic)"""
    lead = t.shape[:-2]
    if layout == 0:
        Ch, L = t.shape[-2:]
        return t.reshape(*lead, G, Ch // G * L)
    L, Ch = t.shape[-2:]
    return t.reshape(*lead, L, G, Ch // G).movedim(-3, -2).reshape(*lead, G, L * (Ch // G))


def affine_rows(v, c, default):
    """per-channel vector (or None) as ``[1, G, N]`` in the row order of `to_rows`"""
    Ch, L = c["Ch"], c["L"]
    if v is None:
        v = torch.full((Ch,), default, dtype=torch.float64)
    full = v.double().reshape(1, Ch, 1).expand(1, Ch, L) if c["layout"] == 0 else v.double().reshape(1, 1, Ch).expand(1, L, Ch)
    return to_rows(full.contiguous(), c["G"], c["layout"])


def forward_reference(x, w, b, c, eps):
    """float64 from the fp32 inputs: dict of rows-view tensors y, xhat, rstd ``[B, G, 1]`` and their bounds"""
    xr = to_rows(x.double(), c["G"], c["layout"])
    N = xr.shape[-1]
    mu = xr.mean(-1, keepdim=True)
    d = xr - mu
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    xhat = d * rstd
    wr, br = affine_rows(w, c, 1.0).to(x.device), affine_rows(b, c, 0.0).to(x.device)
    y = wr * xhat + br
    A = xr.abs().mean(-1, keepdim=True)
    dmu = (N + 2) * U * A
    rel = (N / 2 + 8) * U + 0.5 * (rstd * dmu) ** 2
    b_xhat = rstd * dmu + 2 * U * rstd * d.abs() + xhat.abs() * rel
    b_rstd = rstd * rel
    b_y = wr.abs() * b_xhat + U * (2 * (wr * xhat).abs() + y.abs())
    return dict(y=y, xhat=xhat, rstd=rstd, b_y=b_y, b_xhat=b_xhat, b_rstd=b_rstd)


def vjp_reference(g, xhat, rstd, w, c):
    """float64 from the fp32 inputs ``g [S, B, ..]``, ``xhat [B, ..]``, ``rstd [B, G]``: ``(dx, bound)`` as ``[S, B, G, N]``"""
    G, layout = c["G"], c["layout"]
    xr = to_rows(xhat.double(), G, layout)
    N = xr.shape[-1]
    t = to_rows(g.double(), G, layout) * affine_rows(w, c, 1.0).to(g.device)
    rs = rstd.double().reshape(1, -1, G, 1)
    dx = rs * (t - t.mean(-1, keepdim=True) - xr * (t * xr).mean(-1, keepdim=True))
    bound = U * rs * (4 * t.abs() + (N + 6) * t.abs().mean(-1, keepdim=True)
                      + (N + 8) * xr.abs() * (t * xr).abs().mean(-1, keepdim=True))
    return dx, bound


def make_affine(c, gen, device):
    if c["w"] == "none":
        return None, None
    w = torch.randn(c["Ch"], generator=gen, device=device)
    w[0] = 0.0
    if c["Ch"] > 1:
        w[-1] = -abs(w[-1]) - 0.5
    return w, torch.randn(c["Ch"], generator=gen, device=device)


# ---- fp32 forwards for the CPU check of the bounds ---------------------------------------------------------------------------
def forward_two_pass_fp32(xr, eps):
    """mean-shifted two-pass form on rows ``[.., N]`` in fp32 -> (xhat, rstd)"""
    mu = xr.mean(-1, keepdim=True)
    d = xr - mu
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    return d * rstd, rstd


def forward_mutant_fp32(xr, eps):
    """``var = E[x^2] - mu^2``: the form the kernel must NOT use (cancellation at a large mean)"""
    mu = xr.mean(-1, keepdim=True)
    var = (xr * xr).mean(-1, keepdim=True) - mu * mu
    rstd = 1.0 / torch.sqrt(var.clamp_min(0.0) + eps)
    return (xr - mu) * rstd, rstd


# ---- one autograd pass per seed, the reference of the sweep tests ---------------------------------------------------------------
def autograd_reference(model, taps, x, seeds):
    """one autograd pass per seed: ``(f, tap inputs, per tap [S, ..] cotangents of the tap's output)``"""
    ins, outs = {}, {}

    def keep(n):
        def hook(m_, i, o):
            # (the gradient EDGE of the output as it is now, as laplace_amd.capture.Tape takes it: an in-place ReLU behind the
            # module would otherwise hand back the gradient with respect to the mutated tensor)
            ins[n], outs[n] = i[0].detach().clone(), torch.autograd.graph.get_gradient_edge(o)

        return hook

    hooks = [m.register_forward_hook(keep(n)) for n, m in taps.items()]
    f = model(x)
    for h in hooks:
        h.remove()
    grads = {n: [] for n in taps}
    for s in range(seeds.shape[0]):
        want = torch.autograd.grad(f, [outs[n] for n in taps], grad_outputs=seeds[s], retain_graph=True)
        for n, w in zip(taps, want):
            grads[n].append(w)
    return f, ins, {n: torch.stack(v) for n, v in grads.items()}
