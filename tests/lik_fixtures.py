"""Seeded fp64 logit batches, squared-error vectors, their fp64 references and the per-sample metrics for the likelihood
kernels of csrc/lk_lik.hip (tests/test_lik_fixtures.py pins every case as well-posed for a careful fp32 evaluation on the
CPU; tests/test_gpu_lik.py holds ``lk_softmax_hess_sqrt_f32``, ``lk_softmax_hess_chol_f32`` and ``lk_sq_err_sum_f32`` to
the same bound on the device).

TEST INFRASTRUCTURE, in the style of tests/eig_fixtures.py: everything is built on the CPU in fp64 from fixed seeds, nothing
needs a GPU.  Every logit is an fp64 number that fp32 holds exactly (the common shift is added first, then the sum is
rounded to fp32), so the kernels and the fp64 reference read the same inputs.

Row families (``FAMILIES``), one row of ``[C]`` logits and one label each:

  * ``moderate``      randn * 3, a random label
  * ``correct<m>``    randn * 2 with the label's logit raised to ``max + m``, m in 7, 15, 30: p ~ one-hot on the label
  * ``wrong<m>``      the same with a class that is not the label
  * ``first`` / ``middle`` / ``last``  margin 15 with the dominant class at index 0, C // 2, C - 1 (the Cholesky root
                      eliminates the classes in index order)
  * ``tie_all``       every logit equal;  ``tie_two``: two equal maxima, 2 above the rest
  * ``masked1``       one class that is not the label at -inf;  ``maskedN``: every other class (never the label, never a
                      whole row)

A *mixed* batch cycles through all of them, so that rows whose root entries lie many decades apart share one call: the
per-sample metrics below exist for that batch.  ``shift`` adds one constant to every logit of the batch.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

#: the tolerance the existing tests of these kernels use (``test_softmax_hess_*`` / ``test_sq_err_sum`` of tests/test_gpu_kernels.py)
BOUND = 1e-5
MARGINS = (7, 15, 30)
FAMILIES = ("moderate",) + tuple(f"correct{m}" for m in MARGINS) + tuple(f"wrong{m}" for m in MARGINS) + (
    "first", "middle", "last", "tie_all", "tie_two", "masked1", "maskedN")
SHIFTS = (0, 60, -60, 1000)
BATCHES = (1, 3, 5, 130)              # B % 4 != 0, one wave per sample, four samples per workgroup
CLASSES = (2, 3, 10, 63, 64, 65, 130)  # both roots
CHOL_ONLY = ((5, 1000),)              # (the symmetric root writes C * B * C floats)
#: what ``loss_accum`` holds before each call (the kernels accumulate)
LOSS_BASE = 0.75
IGNORE = -100
#: the rest of a saturated row is randn * 2: with margin 30 on top, the smallest root entry p_j sqrt(p_c) of a 130-class row
#: stays above 1e-30 (randn * 3 reaches 4e-31)
SAT_SPREAD = 2.0


@dataclass(frozen=True)
class LikCase:
    name: str
    f: torch.Tensor        # [B, C] float64, exactly representable in fp32
    y: torch.Tensor        # [B] int64, IGNORE for rows that do not count
    families: tuple        # the family of each row

    def __repr__(self):
        return self.name


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _row(family: str, C: int, g: torch.Generator):
    f = torch.randn(C, generator=g, dtype=torch.float64) * 3
    lab = int(torch.randint(C, (1,), generator=g))
    other = (lab + 1 + int(torch.randint(C - 1, (1,), generator=g))) % C  # a class that is not the label
    if family == "moderate":
        pass
    elif family.startswith("correct") or family.startswith("wrong"):
        m = int(family[7:] if family.startswith("correct") else family[5:])
        k = lab if family.startswith("correct") else other
        f *= SAT_SPREAD / 3
        f[k] = -1e9
        f[k] = f.max() + m
    elif family in ("first", "middle", "last"):
        k = {"first": 0, "middle": C // 2, "last": C - 1}[family]
        f *= SAT_SPREAD / 3
        f[k] = -1e9
        f[k] = f.max() + 15
        lab = k
    elif family == "tie_all":
        f[:] = 0.5
    elif family == "tie_two":
        top = f.max() + 2
        f[lab], f[other] = top, top
    elif family == "masked1":
        f[other] = float("-inf")
    elif family == "maskedN":
        keep = torch.arange(C) % 2 == lab % 2
        f[~keep] = float("-inf")
    else:
        raise ValueError(family)
    return f, lab


def batch(B: int, C: int, shift: float = 0, families=None, ignore="some", first: int = 0) -> LikCase:
    """``families`` None: the mixed batch, row r of family ``FAMILIES[(first + r) % len]``.  ``ignore``: "some" (every
    fifth row, from row 2 on), "all" or "none"."""
    fams = tuple(FAMILIES[(first + r) % len(FAMILIES)] for r in range(B)) if families is None else tuple(
        families[r % len(families)] for r in range(B))
    g = _gen(100003 * C + 1009 * B + 17 * first + sum(map(ord, "".join(fams))) % 997)
    rows = [_row(fm, C, g) for fm in fams]
    f = torch.stack([r[0] for r in rows])
    y = torch.tensor([r[1] for r in rows], dtype=torch.int64)
    if ignore == "all":
        y[:] = IGNORE
    elif ignore == "some":
        y[2::5] = IGNORE
    f = (f + float(shift)).float().double()  # the shift first, then ONE rounding to fp32: these are the inputs
    kind = "mixed" if families is None else "+".join(dict.fromkeys(fams))
    return LikCase(f"{kind}-B{B}-C{C}-shift{shift}-ign{ignore}", f, y, fams)


def _shapes():
    return [(B, C) for C in CLASSES for B in BATCHES]


def cases(cholesky: bool) -> list:
    """the batches of one root: every (B, C) as a mixed batch -- all four shifts at B = 130 (every family present, nine
    times over) and at B = 5, one shift per shape elsewhere, cycling so that each shift meets each small B -- plus, at
    (5, 10), each family alone at shift 1000, a batch whose labels are all ignored, and the Cholesky-only C = 1000"""
    out = []
    for i, (B, C) in enumerate(_shapes()):
        shifts = SHIFTS if B in (5, 130) else (SHIFTS[i % 4],)
        for s in shifts:
            out.append(batch(B, C, s, first=(3 * i) % len(FAMILIES)))
    for fm in FAMILIES:
        out.append(batch(5, 10, 1000, families=(fm,), ignore="none"))
    out.append(batch(5, 10, 60, ignore="all"))
    out.append(batch(130, 65, 0, ignore="all"))
    if cholesky:
        for B, C in CHOL_ONLY:
            fams = ("moderate", "first", "wrong15", "maskedN", "tie_two")
            for s in (0, 1000):
                out.append(batch(B, C, s, families=fams, ignore="some"))
            out.append(batch(B, C, -60, families=("last", "correct30", "middle", "masked1", "tie_all"), ignore="none"))
    return out


# ---- fp64 reference ------------------------------------------------------------------------------------------------------
def _softmax64(f):
    """p and the per-row log-partition relative to the row maximum, log(sum_k exp(f_k - m)), as log1p of the terms other
    than one maximum: exact to fp64 for rows whose partition sum is 1 + 1e-13"""
    m = f.max(1, keepdim=True).values
    e = torch.exp(f - m)
    am = f.argmax(1)
    rest = e.clone()
    rest[torch.arange(f.shape[0]), am] = 0.0
    logz = torch.log1p(rest.sum(1))
    return e / e.sum(1, keepdim=True), logz, m.squeeze(1)


def _others(p):
    """sum_{k != i} p_k without forming 1 - p_i"""
    C = p.shape[1]
    return p @ (1.0 - torch.eye(C, dtype=p.dtype))


def reference(case: LikCase, cholesky: bool):
    """(S [S, B, C], Lambda [B, C, C], loss) in fp64.  Lambda = diag(p) - p p^T with the diagonal in the cancellation-free
    form p_i * sum_{k != i} p_k; the symmetric root's diagonal sqrt(p_c) (1 - p_c) likewise."""
    f, y = case.f, case.y
    B, C = f.shape
    p, logz, m = _softmax64(f)
    oth = _others(p)
    Lam = -p.unsqueeze(2) * p.unsqueeze(1)
    idx = torch.arange(C)
    Lam[:, idx, idx] = p * oth
    valid = y >= 0
    fl = f.gather(1, y.clamp(min=0).view(-1, 1)).squeeze(1)
    loss = torch.where(valid, logz - (fl - m), torch.zeros_like(logz)).sum().item()
    S = roots_from_p(p, cholesky, diag=p.sqrt() * oth)
    return S, Lam, loss


def roots_from_p(p, cholesky: bool, diag=None, top=None):
    """the closed forms of the two kernels, in the dtype of ``p`` ([B, C]):
      symmetric  S[c][n][j] = (j == c ? sqrt(p_c) : 0) - p_j sqrt(p_c)            (``diag``: the entries j == c, if given;
                 ``top``: the entry j == c of one class per row, if given)
      Cholesky   S[c][n][c] = sqrt(p_c / s_c) sqrt(s_{c+1}),  S[c][n][i > c] = -(p_i / sqrt(s_{c+1})) sqrt(p_c / s_c),
                 s_j = sum_{k >= j} p_k; a column whose s_{c+1} is 0 is 0"""
    B, C = p.shape
    if not cholesky:
        sp = p.sqrt()
        S = torch.diag_embed(sp) - p.unsqueeze(2) * sp.unsqueeze(1)  # [B, j, c]
        if diag is not None:
            idx = torch.arange(C)
            S[:, idx, idx] = diag
        if top is not None:  # (am [B], sqrt(p_am) * sum_{k != am} p_k [B]): the one diagonal entry that would cancel
            S[torch.arange(B), top[0], top[0]] = top[1]
        return S.permute(2, 0, 1).contiguous()
    sfx = torch.flip(torch.cumsum(torch.flip(p, [1]), 1), [1])
    sfx = torch.cat([sfx, torch.zeros(B, 1, dtype=p.dtype)], 1)
    sc, sn = sfx[:, :C - 1], sfx[:, 1:C]                              # [B, c]
    ok = (sn > 0) & (sc > 0)
    one = torch.ones_like(sc)
    r0 = torch.where(ok, torch.sqrt(p[:, :C - 1] / torch.where(ok, sc, one)), torch.zeros_like(sc))
    rs = torch.where(ok, 1.0 / torch.sqrt(torch.where(ok, sn, one)), torch.zeros_like(sc))
    low = -(p.unsqueeze(1) * rs.unsqueeze(2)) * r0.unsqueeze(2)       # [B, c, i]
    ci, ii = torch.arange(C - 1).view(1, -1, 1), torch.arange(C).view(1, 1, -1)
    dg = (r0 * torch.sqrt(sn)).unsqueeze(2).expand(B, C - 1, C)
    S = torch.where(ii > ci, low, torch.where(ii == ci, dg, torch.zeros_like(low)))
    return S.permute(1, 0, 2).contiguous()                            # [c, B, i]


def careful_f32(case: LikCase, cholesky: bool, base: float = LOSS_BASE):
    """what a careful fp32 evaluation gives: the kernels' closed forms in torch float32 with the shift taken first,
    p_j = exp((f_j - m) - log z), nll = log z - (f_label - m).  Returns (S, loss_accum after the call)."""
    f = case.f.float()
    m = f.max(1, keepdim=True).values
    t = f - m
    e = torch.exp(t)
    z = e.sum(1, keepdim=True)
    lz = torch.log(z)
    p = torch.exp(t - lz)
    # the diagonal entry of the row's (first) maximum, the only class whose p can approach 1, without forming 1 - p:
    # sqrt(p) * (sum of the other classes' exp) / z; every other class has p <= 1/2
    am = f.argmax(1)
    rest = e.clone()
    rest[torch.arange(f.shape[0]), am] = 0.0
    top = (am, p[torch.arange(f.shape[0]), am].sqrt() * (rest.sum(1) / z.squeeze(1)))
    valid = case.y >= 0
    tl = t.gather(1, case.y.clamp(min=0).view(-1, 1))
    nll = torch.where(valid, (lz - tl).squeeze(1), torch.zeros(f.shape[0]))
    return roots_from_p(p, cholesky, top=top), (torch.tensor(base, dtype=torch.float32) + nll.sum()).item()


# ---- metrics -------------------------------------------------------------------------------------------------------------
def sample_err(got, want) -> float:
    """``got``, ``want`` [B, ...]: per sample, the largest absolute error over the sample's entries divided by the largest
    magnitude of the sample's expected entries; the maximum over the samples.  A sample whose expected entries are all 0
    must come back as exact zeros (inf otherwise).  NaN anywhere in ``got`` is NaN."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    B = want.shape[0]
    if B == 0:
        return 0.0
    if bool(torch.isnan(got).any()):
        return float("nan")
    err = (got - want).abs().reshape(B, -1).amax(1)
    mag = want.abs().reshape(B, -1).amax(1)
    rel = torch.where(mag > 0, err / torch.where(mag > 0, mag, torch.ones_like(mag)),
                      torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return rel.max().item()


def row_err(got, want) -> float:
    """:func:`sample_err` of a root ``[S, B, C]``: sample n is the slice ``[:, n, :]``"""
    return sample_err(got.permute(1, 0, 2), want.permute(1, 0, 2))


def lam_err(S, Lam) -> float:
    """:func:`sample_err` of ``S S^T`` (formed in fp64 from the root as returned) against Lambda ``[B, C, C]``"""
    R = S.detach().double().cpu().permute(1, 2, 0)  # [B, i, c]
    return sample_err(R @ R.transpose(1, 2), Lam)


def loss_err(got: float, want: float) -> float:
    """|got - want| / want, for a positive expected value"""
    assert want > 0
    return abs(float(got) - want) / want


def structure_ok(S, C: int, cholesky: bool) -> bool:
    """C seeds, or C - 1 with every column exactly zero above its diagonal (S[c][n][i] = 0 for i < c)"""
    if not cholesky:
        return S.shape[0] == C
    if S.shape[0] != C - 1:
        return False
    Sc = S.detach().cpu().permute(1, 0, 2)  # [B, c, i]
    return bool((torch.tril(Sc, -1) == 0).all())


def errors(case: LikCase, cholesky: bool, S, loss_after: float, base: float = LOSS_BASE):
    """(root, S S^T, loss) of one call; the loss figure is None for a batch whose labels are all ignored (the caller then
    checks that ``loss_accum`` came back bit for bit)"""
    Sw, Lam, loss = reference(case, cholesky)
    return row_err(S, Sw), lam_err(S, Lam), (loss_err(loss_after, base + loss) if loss > 0 else None)


# ---- squared error -----------------------------------------------------------------------------------------------------------
SQ_NUMELS = (1, 255, 257, 1024 * 256 + 3)  # the last: more 256-element blocks than the 1024 partials
SQ_KINDS = ("random", "equal", "offset")


def sq_case(numel: int, kind: str):
    """(f, y) fp64 vectors that fp32 holds exactly: ``random`` randn, ``equal`` y = f (an exact zero), ``offset`` both
    moved by 1e3 before the rounding"""
    g = _gen(7919 + numel)
    f = torch.randn(numel, generator=g, dtype=torch.float64)
    y = f.clone() if kind == "equal" else torch.randn(numel, generator=g, dtype=torch.float64)
    off = 1e3 if kind == "offset" else 0.0
    return (f + off).float().double(), (y + off).float().double()


SQ_SCALE = 0.5


def sq_reference(f, y) -> float:
    return (SQ_SCALE * ((f - y) ** 2).sum()).item()


def sq_careful_f32(f, y, base: float = LOSS_BASE) -> float:
    d = f.float() - y.float()
    return (torch.tensor(base, dtype=torch.float32) + SQ_SCALE * (d * d).sum()).item()
