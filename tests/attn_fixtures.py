"""Case table, operands, float64 reference with analytic error bounds, fp32 restatements, mutants and end-to-end models of the
scaled dot-product attention kernels (csrc/lk_attn.hip) and of the ATTN / PERMUTE / CONST rules of the seed-batched sweep,
shared by tests/test_attn_fixtures.py, tests/test_sweep_attn.py (CPU) and tests/test_gpu_attn.py (the kernels themselves).

TEST INFRASTRUCTURE.  A case is ``dict(S, B, H, T, D, layout, causal, big)``; ``big``: ``q`` is scaled so that the largest scaled
score is 100, above log(FLT_MAX) = 88.7 - a softmax that does not subtract the row maximum overflows.

THE BOUNDS hold for any summation order and any blocking of the keys into runs of at least ``TILE`` (16) keys; ``u = 2^-24``,
first order in ``u`` with the slack constants written out.  With ``s = scale q k^T`` (float64 from the fp32 operands),
``a = s - rowmax(s)``, ``p = softmax(s)``, ``l = rowsum(exp(a))``, ``lse = rowmax(s) + log l``:

* score            ``e_ij = (D + 3) u |scale| sum_d |q_id k_jd|``  (a D-term dot product, the scale rounded to fp32, their product)
* probability      ``|p^ - p| <= p_ij rp_ij``,
  ``rp_ij = 2 E_i + u (|a_ij| + A_i + |lse_i| + (CLOG + 1) |log l_i|) + (T + (2 CEXP + 4) nb + 3 CEXP + 6) u`` with
  ``E_i = max_j e_ij``, ``A_i = sum_j p_ij |a_ij|``, ``nb = ceil(T / TILE)``:
  the argument of an exponential is rounded once where it is formed and once per rescale of the running maximum, and because
  the running maximum only rises these roundings add up to ``u |a_ij|`` (numerator) and ``u A_i`` (denominator); every
  exponential costs ``CEXP u`` and every rescale one more exponential and one product (``(2 CEXP + 4) nb`` for numerator and
  denominator together); the row sum costs ``(T + nb) u``; the division one ``u``.  The VJP rebuilds ``p = exp(s^ - lse^)``:
  ``lse^`` carries the relative error of the row sum, ``CLOG u |log l|`` of the logarithm and ``u |lse|`` of the addition, the
  subtraction ``u |s - lse| <= u (|a| + |log l|)``.  One ``rp`` covers both routes.
  ``CEXP = CLOG = 2``: ``expf`` / ``logf`` of the device library are accurate to 1 ulp = ``2 u`` (torch's CPU ones as well).
* o, lse, dq, dk, dv: the triangle inequality over the formulas, with ``(n + 2) u sum |terms|`` for an n-term sum (two more for
  the fp32 scale and its product in dq and dk).
* underflow: every exponential and every product may lose up to ``ETA = 2^-126`` absolutely (a result below the normal range,
  flushed or not); the big cases have probabilities of ``e^-200``.
"""
from __future__ import annotations

import math
import os
import re

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the kernel's constants (checked against the source by tests/test_attn_fixtures.py)
ATTN_BM, ATTN_BN, ATTN_TILE, ATTN_RESIDENT_MAX_T, ATTN_MAX_D = 64, 32, 16, 256, 128
U = 2.0 ** -24
ETA = 2.0 ** -126
CEXP = CLOG = 2.0
BIG_SCORE = 100.0


def kernel_constants() -> dict:
    text = open(os.path.join(ROOT, "laplace_amd", "csrc", "lk_attn.hip")).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (ATTN_\w+) = (\d+);", text)}


def _case(S, B, H, T, D, layout=0, causal=False, big=False):
    return dict(S=S, B=B, H=H, T=T, D=D, layout=layout, causal=bool(causal), big=bool(big))


def _table():
    cases = []
    Ts = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129]
    Ds = [4, 8, 12, 16, 20, 32, 64, 124, 128]
    for i, T in enumerate(Ts):  # every T, cycling through D, S, B, H, layout, causal
        cases.append(_case((1, 2, 9)[i % 3], (1, 2)[i % 2], (1, 3)[(i // 2) % 2], T, Ds[i % 9], i % 2, (i // 3) % 2))
    for T in (1, 17, 33, 65, 129):  # the block edges, causal and not, in the other layout
        for causal in (False, True):
            cases.append(_case(2, 1, 3, T, 8, 1 if T != 65 else 0, causal))
    for i, D in enumerate(Ds):  # every D at a T that is no multiple of the tile
        cases.append(_case(2, 2, 1, 33, D, i % 2, i % 2 == 0))
        cases.append(_case(1, 1, 3, 18, D, (i + 1) % 2, i % 2 == 1))
    for d in (-1, 0, 1):  # the resident-P limit of both owner passes, in every instantiation on the far side
        for causal in (False, True):
            cases.append(_case(2, 1, 1, ATTN_RESIDENT_MAX_T + d, 4, int(causal), causal))
        cases.append(_case(1, 1, 2, ATTN_RESIDENT_MAX_T + d, 64, 1, d == 0))
    for D in (20, 128):
        cases.append(_case(2, 1, 1, ATTN_RESIDENT_MAX_T + 1, D, 0, D == 20))
    # scores around 100
    cases += [_case(2, 2, 3, 33, 16, 1, False, True), _case(9, 1, 1, 129, 64, 0, True, True), _case(1, 1, 1, 1, 4, 0, False, True),
              _case(2, 1, 1, ATTN_RESIDENT_MAX_T + 1, 8, 1, False, True), _case(3, 2, 1, 64, 32, 0, True, True)]
    # enough (b, h, block) triples that the seeds are NOT split over grid.y although S > 1
    cases += [_case(2, 512, 4, 16, 8, 1, False), _case(3, 256, 2, 17, 4, 0, True)]
    seen, out = set(), []
    for c in cases:
        key = tuple(sorted(c.items()))
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


CASES = _table()


def case_id(c) -> str:
    return (f"S{c['S']}-B{c['B']}-H{c['H']}-T{c['T']}-D{c['D']}-lay{c['layout']}" + ("-causal" if c["causal"] else "")
            + ("-big" if c["big"] else ""))


def scale_of(c) -> float:
    return 1.0 / math.sqrt(c["D"])


def in_layout(t, layout):
    """``[N, H, T, D]`` values in memory layout 0 (contiguous) or 1 (``[N][T][H][D]``), as a ``[N, H, T, D]`` tensor"""
    return t.contiguous() if layout == 0 else t.transpose(1, 2).contiguous().transpose(1, 2)


def causal_mask(T, device):
    return torch.ones(T, T, dtype=torch.bool, device=device).tril()


def make_operands(c, device="cpu", seed=None):
    """``(q, k, v, go)``: seeded, full-mantissa fp32, ``v`` and ``go`` of either sign; ``q``, ``k``, ``v`` ``[B, H, T, D]`` and
    ``go`` ``[S*B, H, T, D]`` in the case's layout"""
    gen = torch.Generator().manual_seed(1234 + CASES.index(c) if seed is None and c in CASES else (seed or 7))
    B, H, T, D, S = c["B"], c["H"], c["T"], c["D"], c["S"]
    q, k, v = (torch.randn(B, H, T, D, generator=gen) for _ in range(3))
    go = torch.randn(S * B, H, T, D, generator=gen)
    if c["big"]:
        s = (q.double() @ k.double().transpose(-1, -2)) * scale_of(c)
        if c["causal"]:
            s = s.masked_fill(~causal_mask(T, s.device), float("nan"))
        hi, lo = s[~s.isnan()].max().item(), s[~s.isnan()].min().item()
        q = q * (BIG_SCORE / hi if hi > 0 else -BIG_SCORE / lo)  # (one rounding per element: the largest score is 100 (1 +- u))
    return tuple(in_layout(t, c["layout"]).to(device) for t in (q, k, v, go))


# ---- float64 reference and bounds ------------------------------------------------------------------------------------------------
def reference(c, q, k, v, go):
    """float64 from the fp32 operands: dict of ``o``, ``lse``, ``dq``, ``dk``, ``dv`` (the VJPs as ``[S*B, H, T, D]``) and their
    bounds ``b_*`` (see the module docstring)"""
    S, B, H, T, D = c["S"], c["B"], c["H"], c["T"], c["D"]
    scale = scale_of(c)
    q, k, v = q.double(), k.double(), v.double()
    g = go.double().reshape(S, B, H, T, D)
    s = (q @ k.transpose(-1, -2)) * scale
    e = (D + 3) * U * abs(scale) * (q.abs() @ k.abs().transpose(-1, -2))
    if c["causal"]:
        keep = causal_mask(T, s.device)
        s = s.masked_fill(~keep, float("-inf"))
        e = e * keep
    m = s.max(-1, keepdim=True).values
    a = s - m
    ex = torch.exp(a)
    l = ex.sum(-1, keepdim=True)
    p = ex / l
    lse = m + torch.log(l)
    absa = torch.where(p > 0, a.abs(), torch.zeros_like(a))  # (masked entries: p is exactly 0 on every route)
    E, A = e.max(-1, keepdim=True).values, (p * absa).sum(-1, keepdim=True)
    nb = -(-T // ATTN_TILE)
    row = 2 * E + U * (A + lse.abs() + (CLOG + 1) * torch.log(l).abs()) + (T + (2 * CEXP + 4) * nb + 3 * CEXP + 6) * U
    bP = p * (row + U * absa) + ETA
    o = p @ v
    b_o = bP @ v.abs() + (T + 2) * U * (p @ v.abs()) + T * ETA
    b_lse = (E + U * A + (T + (CEXP + 2) * nb + CEXP + 2) * U + (CLOG * torch.log(l).abs() + lse.abs()) * U).squeeze(-1)
    # VJP, for the seeds stacked in front
    pt = p.transpose(-1, -2)
    dv = pt @ g
    b_dv = bP.transpose(-1, -2) @ g.abs() + (T + 2) * U * (pt @ g.abs()) + T * ETA
    dP = g @ v.transpose(-1, -2)
    b_dP = (D + 2) * U * (g.abs() @ v.abs().transpose(-1, -2)) + D * ETA
    delta = (g * o).sum(-1, keepdim=True)
    b_delta = (g.abs() * b_o).sum(-1, keepdim=True) + (D + 2) * U * (g * o).abs().sum(-1, keepdim=True) + D * ETA
    diff = dP - delta
    dS = p * diff
    b_dS = bP * diff.abs() + p * (b_dP + b_delta) + 2 * U * dS.abs() + ETA
    dq = scale * (dS @ k)
    b_dq = abs(scale) * (b_dS @ k.abs() + (T + 4) * U * (dS.abs() @ k.abs()) + T * ETA) + ETA
    dk = scale * (dS.transpose(-1, -2) @ q)
    b_dk = abs(scale) * (b_dS.transpose(-1, -2) @ q.abs() + (T + 4) * U * (dS.abs().transpose(-1, -2) @ q.abs()) + T * ETA) + ETA
    flat = lambda t: t.reshape(S * B, H, T, D)  # noqa: E731
    return dict(o=o, lse=lse.squeeze(-1), dq=flat(dq), dk=flat(dk), dv=flat(dv), b_o=b_o, b_lse=b_lse, b_dq=flat(b_dq),
                b_dk=flat(b_dk), b_dv=flat(b_dv), max_score=s[s > float("-inf")].max().item())


def bound_ratio(got, want, bound) -> float:
    """worst ``|got - want| / bound`` (inf for a NaN or an error where the bound is 0)"""
    err = (got.double().cpu() - want.cpu()).abs()
    bound = bound.cpu()
    if torch.isnan(err).any():
        return float("inf")
    if ((bound == 0) & (err > 0)).any():
        return float("inf")
    live = bound > 0
    return (err[live] / bound[live]).max().item() if live.any() else 0.0


OUTPUTS = ("o", "lse", "dq", "dk", "dv")


def ratios(ref, got: dict) -> dict:
    return {n: bound_ratio(got[n], ref[n], ref["b_" + n]) for n in OUTPUTS if n in got}


# ---- fp32 restatements (and the mutants, which are the first restatement with one thing wrong) ------------------------------------
def rowwise_fp32(c, q, k, v, go, mutant=None):
    """whole rows at once with torch's matmul: ``exp(s - rowmax)``, then the VJP from ``p = exp(s - lse)``.
    ``mutant``: ``"no-max"`` (exp without the maximum subtraction), ``"no-delta"``, ``"strict-causal"`` (mask ``j < i``),
    ``"dk-unscaled"``"""
    S, B, H, T, D = c["S"], c["B"], c["H"], c["T"], c["D"]
    scale = torch.tensor(scale_of(c), dtype=torch.float32)
    s = (q @ k.transpose(-1, -2)) * scale
    if c["causal"]:
        keep = causal_mask(T, s.device).tril(-1) if mutant == "strict-causal" else causal_mask(T, s.device)
        s = s.masked_fill(~keep, float("-inf"))
    m = torch.zeros_like(s[..., :1]) if mutant == "no-max" else s.max(-1, keepdim=True).values
    ex = torch.exp(s - m)
    l = ex.sum(-1, keepdim=True)
    o = (ex @ v) / l
    lse = m + torch.log(l)
    p = torch.exp(s - lse)
    g = go.reshape(S, B, H, T, D)
    dv = p.transpose(-1, -2) @ g
    dP = g @ v.transpose(-1, -2)
    delta = torch.zeros_like(dP[..., :1]) if mutant == "no-delta" else (g * o).sum(-1, keepdim=True)
    dS = p * (dP - delta)
    dq = (dS @ k) * scale
    dk = dS.transpose(-1, -2) @ q
    if mutant != "dk-unscaled":
        dk = dk * scale
    return dict(o=o, lse=lse.squeeze(-1), dq=dq.reshape(S * B, H, T, D), dk=dk.reshape(S * B, H, T, D),
                dv=dv.reshape(S * B, H, T, D))


def _dot_chunks(x, y):
    """``sum_d x[.., i, d] y[.., j, d]`` with ``d`` summed in chunks of 4 from the top down"""
    D = x.shape[-1]
    acc = None
    for d0 in reversed(range(0, D, 4)):
        part = x[..., d0:d0 + 4] @ y[..., d0:d0 + 4].transpose(-1, -2)
        acc = part if acc is None else acc + part
    return acc


def blocked_fp32(c, q, k, v, go):
    """the running-maximum softmax over key blocks of ``ATTN_TILE`` from the LAST block to the first, dot products in chunks of
    4 from the top down; the VJP accumulates ``dq`` over key blocks and ``dk`` / ``dv`` over query blocks of 32"""
    S, B, H, T, D = c["S"], c["B"], c["H"], c["T"], c["D"]
    scale = torch.tensor(scale_of(c), dtype=torch.float32)
    keep = causal_mask(T, q.device) if c["causal"] else torch.ones(T, T, dtype=torch.bool, device=q.device)
    ninf = float("-inf")
    m = torch.full((B, H, T, 1), ninf)
    l = torch.zeros(B, H, T, 1)
    acc = torch.zeros(B, H, T, D)
    blocks = [(j0, min(j0 + ATTN_TILE, T)) for j0 in range(0, T, ATTN_TILE)]
    for j0, j1 in reversed(blocks):
        s = (_dot_chunks(q, k[..., j0:j1, :]) * scale).masked_fill(~keep[:, j0:j1], ninf)
        mn = torch.maximum(m, s.max(-1, keepdim=True).values)
        safe = torch.where(mn == ninf, torch.zeros_like(mn), mn)  # (a row that has seen no visible key yet)
        alpha, ex = torch.exp(m - safe), torch.exp(s - safe)
        l = l * alpha + ex.sum(-1, keepdim=True)
        acc = acc * alpha + ex @ v[..., j0:j1, :]
        m = mn
    o, lse = acc / l, m + torch.log(l)
    g = go.reshape(S, B, H, T, D)
    delta = (g * o).sum(-1, keepdim=True)
    dq, dk, dv = torch.zeros_like(g), torch.zeros_like(g), torch.zeros_like(g)
    for j0, j1 in blocks:
        s = (_dot_chunks(q, k[..., j0:j1, :]) * scale).masked_fill(~keep[:, j0:j1], ninf)
        dS = torch.exp(s - lse) * (_dot_chunks(g, v[..., j0:j1, :]) - delta)
        dq += dS @ k[..., j0:j1, :]
    for i0 in range(0, T, 32):
        i1 = min(i0 + 32, T)
        s = (_dot_chunks(q[..., i0:i1, :], k) * scale).masked_fill(~keep[i0:i1], ninf)
        p = torch.exp(s - lse[..., i0:i1, :])
        dS = p * (_dot_chunks(g[..., i0:i1, :], v) - delta[..., i0:i1, :])
        dv += p.transpose(-1, -2) @ g[..., i0:i1, :]
        dk += dS.transpose(-1, -2) @ q[..., i0:i1, :]
    return dict(o=o, lse=lse.squeeze(-1), dq=(dq * scale).reshape(S * B, H, T, D), dk=(dk * scale).reshape(S * B, H, T, D),
                dv=dv.reshape(S * B, H, T, D))


MUTANTS = ("no-max", "no-delta", "strict-causal", "dk-unscaled")


# ---- end-to-end models -----------------------------------------------------------------------------------------------------------
class AttnSeq(nn.Module):
    """[B, 4, 5] -> Linear(5, 8) + positional buffer -> one pre-LN block (2 heads of 4, GELU) -> mean over positions -> Linear"""

    def __init__(self, C=3, causal=False):
        super().__init__()
        from laplace_amd.nets import AttentionBlock, sincos_positions

        self.embed = nn.Linear(5, 8)
        self.register_buffer("pos", sincos_positions(4, 8))
        self.block = AttentionBlock(8, 2, mlp_ratio=2.0, act=nn.GELU, causal=causal)
        self.head = nn.Linear(8, C)

    def forward(self, x):
        return self.head(self.block(self.embed(x) + self.pos).mean(1))


class AttnViT(nn.Module):
    """4 x 4 images -> Conv2d(2, 8, 2, 2) patches -> flatten(2) -> transpose(1, 2) -> one block -> LayerNorm -> mean -> Linear"""

    def __init__(self, C=3):
        super().__init__()
        from laplace_amd.nets import AttentionBlock

        self.embed = nn.Conv2d(2, 8, 2, 2)
        self.block = AttentionBlock(8, 2, mlp_ratio=2.0, act=nn.GELU)
        self.norm = nn.LayerNorm(8)
        self.head = nn.Linear(8, C)

    def forward(self, x):
        return self.head(self.norm(self.block(self.embed(x).flatten(2).transpose(1, 2))).mean(1))


MODELS = ("attnseq", "attnseq-causal", "attnvit")


def make_model(name, C=3, seed=3, freeze_norm=True):
    """``(model fp32, its fp64 twin, inputs [9, ..] fp32)``; the LayerNorm affines are frozen (KFAC refuses tracked ones)"""
    torch.manual_seed(seed)
    model = AttnViT(C) if name == "attnvit" else AttnSeq(C, causal=name.endswith("causal"))
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.LayerNorm):  # (affines away from the identity, so that they matter)
                m.weight.add_(0.3 * torch.randn_like(m.weight))
                m.bias.add_(0.3 * torch.randn_like(m.bias))
                if freeze_norm:
                    m.weight.requires_grad_(False), m.bias.requires_grad_(False)
    model.eval()
    X = torch.randn(9, 2, 4, 4) if name == "attnvit" else torch.randn(9, 4, 5)
    import copy

    return model, copy.deepcopy(model).double(), X


class _Loader(list):
    pass


def rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return (got - want).abs().max().item() / (want.abs().max().item() + 1e-30)


def run_curvature_checks(dev, name, lik, configure=None):
    """the ``_run`` body of tests/test_weight_sharing.py on a fixture model: jacobians, diag, full, a two-minibatch kron fit, the
    Kron and the diagonal predictive against the fp64 oracle at the project's tolerances - and the proof that the SWEEP produced
    them.  ``configure(backend)`` sets switches on every backend object; returns what the routes are compared by."""
    from laplace_amd import HipGGN
    from laplace_amd.laplace import HipLaplace
    from oracle import curvature_oracle as co

    C = 3 if lik == "classification" else 2
    model, m64, X = make_model(name, C)
    model, X = model.to(dev), X.to(dev)
    torch.manual_seed(11)
    y = torch.randint(C, (9,)).to(dev) if lik == "classification" else torch.randn(9, C).to(dev)
    X64, y64 = X.double().cpu(), (y.cpu() if lik == "classification" else y.double().cpu())
    Js64, f64 = co.jacobians(m64, X64)
    Hl = co.functional_hessian(f64, lik)
    configure = configure or (lambda b: None)

    def swept(backend):
        tape = backend._tape()
        assert getattr(tape, "sweep_reason", None) is None, tape.sweep_reason
        assert any(tape.sweeps.get(r) not in (None, False) for r in (frozenset(), frozenset({"norm"}))), "no sweep was built"

    backend = HipGGN(model, lik)
    configure(backend)
    Js, f = backend.jacobians(X)
    assert rel(f, f64) < 1e-5 and rel(Js, Js64) < 1e-4
    _, h = backend.diag(X, y)
    assert rel(h, co.ggn_diag(Js64, Hl)) < 1e-4
    _, H = backend.full(X, y)
    assert rel(H, co.ggn_full(Js64, Hl)) < 1e-4
    swept(backend)

    loader = _Loader([(X[:5], y[:5]), (X[5:], y[5:])])
    loader.dataset = range(9)
    la = HipLaplace(model, lik, "all", "kron", prior_precision=0.7)
    configure(la.backend)
    la.fit(loader)
    want = None
    for xb, yb in ((X64[:5], y64[:5]), (X64[5:], y64[5:])):
        _, kf = co.kfac_ggn(m64, xb, yb, 9, lik)
        want = kf if want is None else co.kron_add(want, kf)
    for F_, G_ in zip(la.H_facs.kfacs, want):
        for a_, w_ in zip(F_, G_):
            assert rel(a_, w_) < 1e-4
    swept(la.backend)
    f_mu, f_var = la._glm_predictive_distribution(X)
    Qs, ls = co.kron_decompose(want)
    sig = float(la.sigma_noise)
    assert rel(f_var, co.functional_variance_kron(Js64, Qs, ls, 0.7, h_factor=1.0 / sig**2)) < 1e-4
    ld = HipLaplace(model, lik, "all", "diag", prior_precision=0.7)
    configure(ld.backend)
    ld.fit(loader)
    _, f_var_d = ld._glm_predictive_distribution(X)
    post_var = 1.0 / (co.ggn_diag(Js64, Hl) / sig**2 + 0.7)
    assert rel(f_var_d, co.functional_variance_diag(Js64, post_var)) < 1e-4
    swept(ld.backend)
    return dict(Js=Js, f=f, h=h, H=H, f_var=f_var, f_var_d=f_var_d, kfacs=[t for F_ in la.H_facs.kfacs for t in F_])
