"""``EmulatedGConvKernels`` plus the three embedding entry points (csrc/lk_embed.hip) in stock torch, for the CPU test tier.

TEST INFRASTRUCTURE.  The emulations below this one deliberately have no ``jac_embed``: a backend on them sends a model with a
tracked nn.Embedding weight or a tracked lone parameter to the reference's generic route.

The emulation follows the kernels' contract, not their schedule: a one-hot ``index_add`` per sample.  Ids outside ``[0, V)`` and
the padding id write nothing; ``jac_embed`` touches only the columns of the ids that occur in the row.
"""
import torch

from tests.emulated_gconv_kernels import EmulatedGConvKernels


def run_sums(g, ids, V, padding_idx):
    """``R [S, B, V, D]``: per (seed, sample, id) the sum of ``g [S, B, T, D]`` over the positions that hold the id, and
    ``hit [B, V]``: the ids that occur in the row and are written (inside the table, not the padding row)"""
    S, B = g.shape[:2]
    D = g.shape[-1]
    T = 1
    for n in ids.shape[1:]:
        T *= int(n)
    g = g.reshape(S, B, T, D)
    ids = ids.reshape(B, T)
    pad = -1 if padding_idx is None else int(padding_idx)
    live = (ids >= 0) & (ids < V) & (ids != pad)
    safe = torch.where(live, ids, torch.zeros_like(ids))
    R = torch.zeros(S, B, V, D, dtype=g.dtype, device=g.device)
    hit = torch.zeros(B, V, dtype=torch.bool, device=g.device)
    for b in range(B):
        R[:, b].index_add_(1, safe[b], g[:, b] * live[b].to(g.dtype)[None, :, None])
        hit[b, safe[b][live[b]]] = True
    return R, hit


class EmulatedEmbedKernels(EmulatedGConvKernels):
    def jac_embed(self, g, ids, V, padding_idx, Js, col0):
        R, hit = run_sums(g, ids, V, padding_idx)
        S, B, _, D = R.shape
        block = Js[:, :, col0:col0 + V * D].reshape(B, S, V, D)
        mask = hit[:, None, :, None].expand(B, S, V, D)
        Js[:, :, col0:col0 + V * D] = torch.where(mask, R.permute(1, 0, 2, 3), block).reshape(B, S, V * D)

    def diag_embed(self, g, ids, V, padding_idx, alpha, h):
        R, _ = run_sums(g, ids, V, padding_idx)
        h += alpha * (R * R).sum((0, 1)).reshape(-1)

    def diag_quadform_embed(self, g, ids, V, padding_idx, var, fvar):
        R, _ = run_sums(g, ids, V, padding_idx)
        fvar += torch.einsum("cbvd,kbvd,vd->bck", R, R, var.reshape(V, -1))
        return fvar
