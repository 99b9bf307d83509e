"""Cases, fp64 references, per-element bounds, a plain fp32 evaluation, mutants and the checks themselves for the dense
last-layer, Jacobian, diagonal and element-wise kernels of csrc/lk_ll.hip, csrc/lk_diag.hip and csrc/lk_vjp.hip.

TEST INFRASTRUCTURE, in the style of tests/lik_fixtures.py and tests/kronalg_fixtures.py: everything is built on the CPU in
fp64 from fixed seeds and every input is an fp64 number that fp32 holds exactly.  Each ``check_*`` takes a kernels object and
a ``dev`` function that places a tensor where those kernels read it, runs every case of its table and returns
``{case name: worst |got - ref| / bound}``.  tests/test_dense_fixtures.py passes :class:`Fp32Kernels` (torch float32 on the
CPU) and the mutants below; tests/test_gpu_dense.py passes the HIP library behind the C ABI.

Bounds.  An accumulated output element is held to ``|got - ref| <= gamma(n + e) * sum |terms|`` with ``gamma(k) = k u /
(1 - k u)``, ``u = 2^-24``, ``n`` the number of terms accumulated (any summation order), ``sum |terms|`` the fp64 sum of the
same terms' magnitudes and ``e`` the number of fp32 roundings one term passes through before and after it is accumulated.
The counts, from the formulas:

  ``ll_ggn_full``, class pair j != k   term  alpha * (p_j pt_a) * (p_k pt_b):  round p_j, round p_k (the kernel is handed the
        fp32 rounding of the fp64 softmax), p_j * pt_a, p_k * pt_b, their product, the scale by alpha, the add into H: e = 7
  ``ll_ggn_full``, class pair j == j   term  alpha * (sqrt(p_j s_j) pt_a) * (sqrt(p_j s_j) pt_b),  s_j = sum_{k != j} p_k:
        the argument of the root carries round p_j (1), the C - 1 rounded p_k of s_j (1: all positive) and its C - 2 additions,
        and the product p_j * s_j (1): C + 1 in all, which the root halves and the square restores; then the root itself in
        each of the two factors (2), the two products with pt (2), their product (1), alpha (1), the add into H (1):
        e = C + 8
  ``ll_ggn_full``, regression          term  alpha * pt_a * pt_b: the product, alpha, the add: e = 3
  ``dense_quadform_ll``                term  pt_p * Sigma * pt_q, n = 2 Dt (a sum over q of sums over p): two products, e = 2
  ``diag_ggn_linear`` h_w              term  alpha * g^2 * a^2, n = B + Cc (a sum over the batch of sums over the seeds):
        g^2, a^2, their product, alpha, the add into h_w: e = 5;      h_b: term alpha * g^2: e = 3
  ``jac_conv``                         term  g * patch, n = L: the product, e = 1;  bias column: term g, e = 0
  ``sq_colsum``                        term  alpha * Js^2, n = rows: the square, alpha, the add: e = 3
A non-zero starting value of an accumulated output adds ``u |start|``.  Where ``sum |terms|`` is 0 the bound is 0: an expected
exact zero must come back as exactly zero.  A NaN anywhere fails.  Outputs that are one product or a copy (``jac_linear``,
``jac_last_layer``) are compared for equality with the fp32 value.  ``vjp_scale_mask``: ``3 u |value|`` (the sum g + g2, the
product multiplier * scale, their product); ``bn_act_forward``: ``3 u (|x sc| + |sh| + |addend|)``.
"""
from __future__ import annotations

from functools import lru_cache

import torch
import torch.nn.functional as F

from tests import lik_fixtures as LF

U = 2.0 ** -24
NAN = float("nan")


def gamma(k):
    return k * U / (1.0 - k * U)


def f32(t):
    """round to what fp32 holds, keep fp64"""
    return t.float().double()


def _randn(*shape, seed):
    return f32(torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64))


def cpu_dev(t):
    return t.float() if t.dtype == torch.float64 else t


def ratio(got, ref, bound) -> float:
    """worst |got - ref| / bound; inf where the bound is 0 and the element differs; NaN for a NaN in ``got``"""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if got.numel() == 0:
        return 0.0
    if bool(got.isnan().any()):
        return NAN
    err = (got - ref).abs()
    pos = bound > 0
    r = torch.where(pos, err / torch.where(pos, bound, torch.ones_like(bound)),
                    torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return r.max().item()


def same(got, want32) -> float:
    """0 if ``got`` holds the fp32 values of ``want32`` (NaN where it has NaN), inf otherwise"""
    got, want32 = got.detach().cpu(), want32.detach().cpu()
    assert got.shape == want32.shape and got.dtype == want32.dtype, (got.shape, want32.shape)
    ok = (got == want32) | (got.isnan() & want32.isnan()) if got.is_floating_point() else got == want32
    return 0.0 if bool(ok.all()) else float("inf")


def ok(r) -> bool:
    return r <= 1.0  # False for NaN


def ceil_div(a, b):
    return -(-a // b)


# ============================================================================================================================
# ll_ggn_full
# ============================================================================================================================
LL_KINDS = ("moderate", "correct7", "correct15", "correct30", "mixed")
SATURATED = ("correct15", "correct30")


def ref_index(j, a, C, D):
    """augmented index (class j, feature a; a == D is the bias) -> the reference's parameter index"""
    return j * D + a if a < D else C * D + j


def ref_perm(C, D, Dt):
    return torch.tensor([ref_index(j, a, C, D) for j in range(C) for a in range(Dt)])


def _ll(B, C, Dt, bias, kind, alpha=1.0, base=False):
    return dict(B=B, C=C, D=Dt - int(bias), bias=bias, kind=kind, alpha=alpha, base=base)


def ll_id(c):
    return (f"{c['kind']}-B{c['B']}-C{c['C']}-D{c['D']}" + ("-bias" if c["bias"] else "") +
            (f"-alpha{c['alpha']}" if c["alpha"] != 1.0 else "") + ("-base" if c["base"] else ""))


def _ll_cases():
    out = []
    shapes = [(16, True), (17, False), (33, True), (17, True), (16, False), (33, False)]  # (Dt, bias)
    i = 0
    for kind in LL_KINDS:
        for C in (2, 3, 10):
            for B in (1, 5, 130):
                Dt, bias = (33, True) if (B, C) == (130, 10) else shapes[i % len(shapes)]
                out.append(_ll(B, C, Dt, bias, kind))
                i += 1
        out.append(_ll(5, 3, 1, False, kind))
    for B, C, Dt, bias in ((1, 1, 1, False), (5, 2, 16, True), (130, 3, 17, False), (130, 10, 33, True), (5, 1, 33, True)):
        out.append(_ll(B, C, Dt, bias, "regression"))
    for B, Dt, bias in ((1, 1, False), (5, 17, True), (130, 33, False)):   # C = 1 with probabilities: every entry is 0
        out.append(_ll(B, 1, Dt, bias, "one_class"))
    out.append(_ll(130, 10, 33, True, "correct15", alpha=0.75))
    out.append(_ll(5, 3, 17, True, "mixed", alpha=1.5))
    out.append(_ll(130, 2, 16, False, "regression", alpha=0.375))
    out.append(_ll(130, 10, 33, True, "correct30", base=True))
    out.append(_ll(5, 2, 17, True, "moderate", alpha=0.75, base=True))
    out.append(_ll(5, 3, 16, True, "regression", base=True))
    return out


LL_CASES = _ll_cases()


def ll_form(c):
    """which path of ``lk_ll_ggn_full_f32`` the case takes and how many launches it makes there"""
    if c["B"] == 0:
        return ("empty", 0)
    if c["kind"] == "regression":
        return ("regression", 1)
    return ("classification", 1 + c["C"])  # Gram(Y) + C block Grams


def ll_logits(c):
    B, C = c["B"], c["C"]
    if c["kind"] == "regression":
        return None
    if C == 1:
        return torch.zeros(B, 1, dtype=torch.float64)
    fams = None if c["kind"] == "mixed" else (c["kind"],)
    return LF.batch(B, C, 0, families=fams, ignore="none").f


@lru_cache(maxsize=None)
def _ll_reference(B, C, D, bias, kind, alpha, base):
    c = dict(B=B, C=C, D=D, bias=bias, kind=kind, alpha=alpha, base=base)
    Dt = D + int(bias)
    P = C * Dt
    phi = _randn(B, D, seed=11 + 7 * B + 3 * C + D)
    pt = torch.cat([phi, torch.ones(B, 1, dtype=torch.float64)], 1) if bias else phi
    f = ll_logits(c)
    idx = torch.arange(C)
    if f is None:
        p32 = None
        Lam = torch.eye(C, dtype=torch.float64).expand(B, C, C).clone()
        e = torch.full((C, C), 3.0)
    else:
        p = LF._softmax64(f)[0]
        p32 = f32(p)
        Lam = -p.unsqueeze(2) * p.unsqueeze(1)
        Lam[:, idx, idx] = p * LF._others(p)
        e = torch.full((C, C), 7.0)
        e[idx, idx] = C + 8.0
    PP = (pt.unsqueeze(2) * pt.unsqueeze(1)).reshape(B, Dt * Dt)

    def aug(L_, PP_):
        return (L_.reshape(B, C * C).T @ PP_).reshape(C, C, Dt, Dt).permute(0, 2, 1, 3).reshape(P, P)

    perm = ref_perm(C, D, Dt)
    H0 = torch.zeros(P, P, dtype=torch.float64)
    if base:
        G = _randn(P, 3, seed=5 + P)
        H0 = f32(G @ G.T + torch.eye(P, dtype=torch.float64))
    H = torch.zeros(P, P, dtype=torch.float64)
    A = torch.zeros(P, P, dtype=torch.float64)
    k = torch.zeros(P, P, dtype=torch.float64)
    H[perm[:, None], perm[None, :]] = alpha * aug(Lam, PP)
    A[perm[:, None], perm[None, :]] = abs(alpha) * aug(Lam.abs(), PP.abs())
    k[perm[:, None], perm[None, :]] = (B + e.double()).repeat_interleave(Dt, 0).repeat_interleave(Dt, 1)
    bound = gamma(k) * A + U * H0.abs()
    return dict(phi=phi, p32=p32, H0=H0, H=H0 + H, ggn=H, bound=bound)


def ll_reference(c):
    return _ll_reference(c["B"], c["C"], c["D"], c["bias"], c["kind"], c["alpha"], c["base"])


def ll_figures(c, got):
    """(element error / bound, -lambda_min / ||bound||_F, number of negative diagonal entries) of a returned H"""
    r = ll_reference(c)
    got64 = got.detach().double().cpu()
    el = ratio(got64, r["H"], r["bound"])
    if el != el:
        return el, NAN, 0
    lam = torch.linalg.eigvalsh((got64 + got64.T) / 2).min().item()
    nb = torch.linalg.norm(r["bound"]).item()
    eig = 0.0 if lam >= 0 else (-lam / nb if nb > 0 else float("inf"))
    return el, eig, int((got64.diagonal() < 0).sum())


#: (element figure, eigenvalue figure, negative diagonal entries) of the last :func:`check_ll_ggn`, per case
LL_FIGURES = {}


def check_ll_ggn(K, dev, cases=None) -> dict:
    """per case the larger of the element figure and the eigenvalue figure; inf for a negative diagonal entry"""
    out = {}
    for c in (LL_CASES if cases is None else cases):
        r = ll_reference(c)
        got = K.ll_ggn_full(dev(r["phi"]), None if r["p32"] is None else dev(r["p32"]), c["C"], c["bias"], c["alpha"],
                            dev(r["H0"]))
        el, eig, neg = ll_figures(c, got)
        if c["kind"] == "one_class" and not c["base"] and bool((got != 0).any()):
            el = float("inf")
        out[ll_id(c)] = max(el, eig, float("inf") if neg else 0.0) if el == el else el
        LL_FIGURES[ll_id(c)] = (el, eig, neg)
    return out


# ============================================================================================================================
# dense_quadform_ll
# ============================================================================================================================
def _qf(B, C, Dt, bias, kind, delta):
    return dict(B=B, C=C, D=Dt - int(bias), bias=bias, kind=kind, delta=delta)


QF_CASES = [
    _qf(1, 1, 1, False, "regression", 1.0),
    _qf(127, 2, 15, True, "moderate", 1.0),
    _qf(128, 3, 16, False, "correct15", 1e-4),
    _qf(129, 10, 17, True, "correct30", 1e4),
    _qf(129, 10, 33, True, "correct15", 1e-4),
    _qf(128, 2, 128, True, "mixed", 1.0),
    _qf(129, 2, 129, False, "correct30", 1e-4),
    _qf(128, 3, 129, True, "moderate", 1e4),
    _qf(127, 1, 257, True, "regression", 1e-4),
    _qf(1, 2, 257, False, "correct7", 1.0),
    _qf(129, 3, 1, False, "mixed", 1.0),
]


def qf_id(c):
    return f"{c['kind']}-B{c['B']}-C{c['C']}-D{c['D']}" + ("-bias" if c["bias"] else "") + f"-delta{c['delta']:g}"


def qf_form(c):
    """grid and loop extents of ``dense_quadform_ll_kernel``: (128-sample tiles, samples in the last tile, class pairs,
    128-column steps of q, entries of the last 16-row chunk of p)"""
    Dt = c["D"] + int(c["bias"])
    return (ceil_div(c["B"], 128), c["B"] % 128 or 128, c["C"] * (c["C"] + 1) // 2, ceil_div(Dt, 128), Dt % 16 or 16)


@lru_cache(maxsize=None)
def _qf_reference(B, C, D, bias, kind, delta):
    ll = _ll_reference(B, C, D, bias, kind, 1.0, False)
    Dt = D + int(bias)
    P = C * Dt
    S = torch.linalg.inv(ll["ggn"] + delta * torch.eye(P, dtype=torch.float64))
    Sigma = f32((S + S.T) / 2)
    assert torch.equal(Sigma, Sigma.T)
    phi = ll["phi"]
    pt = torch.cat([phi, torch.ones(B, 1, dtype=torch.float64)], 1) if bias else phi
    perm = ref_perm(C, D, Dt)
    Sa = Sigma[perm[:, None], perm[None, :]].reshape(C, Dt, C, Dt)
    fvar = torch.einsum("np,cpkq,nq->nck", pt, Sa, pt)
    mag = torch.einsum("np,cpkq,nq->nck", pt.abs(), Sa.abs(), pt.abs())
    return dict(phi=phi, Sigma=Sigma, fvar=fvar, bound=gamma(2 * Dt + 2) * mag)


def qf_reference(c):
    return _qf_reference(c["B"], c["C"], c["D"], c["bias"], c["kind"], c["delta"])


def check_quadform(K, dev, cases=None) -> dict:
    out = {}
    for c in (QF_CASES if cases is None else cases):
        r = qf_reference(c)
        got = K.dense_quadform_ll(dev(r["phi"]), dev(r["Sigma"]), c["C"], c["bias"])
        v = ratio(got, r["fvar"], r["bound"])
        if v == v and not torch.equal(got, got.transpose(1, 2)):
            v = float("inf")  # fvar[n][c][k] and fvar[n][k][c] are the same bits
        out[qf_id(c)] = v
    return out


# ============================================================================================================================
# jac_last_layer
# ============================================================================================================================
JLL_CASES = [  # B, C, D, bias
    (1, 1, 1, False), (3, 1, 4, True), (5, 3, 4, False), (5, 3, 4, True), (2, 10, 33, True), (7, 2, 6, True), (4, 4, 5, False),
    (96, 10, 512, True),   # B C ceil(P / 4) = 1 231 680 > 4096 * 256: the grid-stride loop takes a second trip
]


def jll_form(B, C, D, bias):
    """(float4 stores?, trips of the grid-stride loop) of ``lk_jac_last_layer_f32``"""
    P = C * D + (C if bias else 0)
    work = B * C * ceil_div(P, 4)
    grid = min(4096, max(1, ceil_div(work, 256)))
    return (P % 4 == 0, ceil_div(work, grid * 256))


def jll_reference(B, C, D, bias):
    phi = _randn(B, D, seed=B + C + D)
    P = C * D + (C if bias else 0)
    Js = torch.zeros(B, C, P, dtype=torch.float64)
    for i in range(C):
        Js[:, i, i * D:(i + 1) * D] = phi
        if bias:
            Js[:, i, C * D + i] = 1.0
    return phi, Js


def check_jac_last_layer(K, dev, cases=None) -> dict:
    out = {}
    for B, C, D, bias in (JLL_CASES if cases is None else cases):
        phi, Js = jll_reference(B, C, D, bias)
        got = K.jac_last_layer(dev(phi), C, bias)
        out[f"B{B}-C{C}-D{D}" + ("-bias" if bias else "")] = same(got, Js.float())
    return out


# ============================================================================================================================
# diag_ggn_linear
# ============================================================================================================================
def _dg_cases():
    out, dims = [], (1, 15, 16, 17, 33)
    for i, B in enumerate((1, 63, 64, 65, 130)):
        for j, Di in enumerate(dims):
            Do = dims[(i + j) % 5]
            out.append(dict(B=B, S=3 if (i + j) % 2 else 1, Di=Di, Do=Do, hb=(i + 2 * j) % 3 != 0, start=(i + j) % 4 == 1))
    out.append(dict(B=65, S=3, Di=33, Do=33, hb=True, start=True))
    out.append(dict(B=130, S=1, Di=17, Do=17, hb=False, start=True))
    return out


DG_CASES = _dg_cases()
DG_ALPHA = 0.75


def dg_id(c):
    return f"B{c['B']}-S{c['S']}-Di{c['Di']}-Do{c['Do']}" + ("-hb" if c["hb"] else "") + ("-start" if c["start"] else "")


def dg_form(c):
    """(64-sample chunks, samples in the last chunk, grid.x, grid.y, h_b given)"""
    return (ceil_div(c["B"], 64), c["B"] % 64 or 64, ceil_div(c["Di"], 16), ceil_div(c["Do"], 16), c["hb"])


def dg_reference(c):
    B, S, Di, Do = c["B"], c["S"], c["Di"], c["Do"]
    a, g = _randn(B, Di, seed=B + Di), _randn(S, B, Do, seed=B + Do + S)
    hw0 = f32(_randn(Do, Di, seed=3).abs() * 50) if c["start"] else torch.zeros(Do, Di, dtype=torch.float64)
    hb0 = f32(_randn(Do, seed=4).abs() * 50) if c["start"] else torch.zeros(Do, dtype=torch.float64)
    gsq = (g ** 2).sum(0)
    tw, tb = DG_ALPHA * gsq.T @ a ** 2, DG_ALPHA * gsq.sum(0)  # all terms are non-negative: they are their own magnitudes
    return dict(a=a, g=g, hw0=hw0, hb0=hb0, hw=hw0 + tw, hb=hb0 + tb, bw=gamma(B + S + 5) * tw + U * hw0,
                bb=gamma(B + S + 3) * tb + U * hb0)


def check_diag_linear(K, dev, cases=None) -> dict:
    out = {}
    for c in (DG_CASES if cases is None else cases):
        r = dg_reference(c)
        hw, hb = K.diag_ggn_linear(dev(r["a"]), dev(r["g"]), DG_ALPHA, dev(r["hw0"]), dev(r["hb0"]) if c["hb"] else None)
        v = ratio(hw, r["hw"], r["bw"])
        if c["hb"]:
            v = max(v, ratio(hb, r["hb"], r["bb"])) if v == v else v
        else:
            assert hb is None
        out[dg_id(c)] = v
    return out


# ============================================================================================================================
# jac_linear
# ============================================================================================================================
JLIN_CASES = [  # B, S, Di, Do, col0, bias columns, columns after
    (3, 2, 5, 7, 0, True, 0), (3, 2, 5, 7, 3, True, 2), (2, 1, 16, 16, 1, False, 3), (1, 3, 1, 1, 2, True, 1),
    (130, 2, 3, 5, 4, True, 4), (2, 3, 17, 33, 0, False, 0),
    (1, 1, 512, 513, 2, True, 3),   # Do * Di = 262 656 > 1024 * 256: a second trip of the grid-stride loop
]


def jlin_form(Di, Do, bias):
    """(trips of the grid-stride loop, bias columns written)"""
    bx = min(1024, ceil_div(Do * Di, 256))
    return (ceil_div(Do * Di, bx * 256), bias)


def jlin_layout(Di, Do, col0, bias, after):
    """(P, bcol0): the bias columns, if any, follow the weight columns after a gap of one column"""
    bcol0 = col0 + Do * Di + 1 if bias else -1
    return col0 + Do * Di + ((1 + Do) if bias else 0) + after, bcol0


def check_jac_linear(K, dev, cases=None) -> dict:
    out = {}
    for B, S, Di, Do, col0, bias, after in (JLIN_CASES if cases is None else cases):
        a, g = _randn(B, Di, seed=B + Di), _randn(S, B, Do, seed=S + Do)
        P, bcol0 = jlin_layout(Di, Do, col0, bias, after)
        want = torch.full((B, S, P), NAN, dtype=torch.float32)
        want[:, :, col0:col0 + Do * Di] = (g.float().permute(1, 0, 2).unsqueeze(3) * a.float()[:, None, None, :]).reshape(B, S, -1)
        if bias:
            want[:, :, bcol0:bcol0 + Do] = g.float().permute(1, 0, 2)
        got = K.jac_linear(dev(a), dev(g), dev(torch.full((B, S, P), NAN, dtype=torch.float64)), col0, bcol0)
        out[f"B{B}-S{S}-Di{Di}-Do{Do}-col{col0}" + ("-bias" if bias else "")] = same(got, want)
    return out


# ============================================================================================================================
# jac_conv
# ============================================================================================================================
def _cv(B, S, Cin, H, W, Do, k, s, p, d, bias):
    pair = lambda v: v if isinstance(v, tuple) else (v, v)
    return dict(B=B, S=S, Cin=Cin, H=H, W=W, Do=Do, k=pair(k), s=pair(s), p=pair(p), d=pair(d), bias=bias)


CV_CASES = [
    _cv(2, 2, 8, 9, 7, 5, (3, 2), (2, 1), (1, 0), (1, 2), True),   # the anisotropic row of CONV_CASES
    _cv(2, 1, 2, 3, 3, 1, 3, 1, 0, 1, True),                       # L = 1
    _cv(2, 3, 3, 5, 5, 17, 3, 1, 1, 1, False),                     # L = 25, Dk = 27
    _cv(1, 2, 2, 4, 4, 3, 2, 1, 2, 1, True),                       # padding larger than the kernel needs: L = 49
    _cv(2, 1, 3, 7, 6, 17, 3, 1, 2, 2, True),                      # dilation 2
    _cv(3, 2, 1, 6, 6, 1, 3, 2, 1, 1, False),                      # stride 2, Do = 1, Dk = 9
    _cv(1, 1, 4, 8, 8, 2, 2, 2, 0, 1, True),                       # L = 16, Dk = 16: whole chunks only
]


def cv_geom(c):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = c["k"], c["s"], c["p"], c["d"]
    OH = (c["H"] + 2 * ph - dh * (kh - 1) - 1) // sh + 1
    OW = (c["W"] + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    return OH, OW, c["Cin"] * kh * kw


def cv_form(c):
    """(16-position chunks of L, positions in the last chunk, grid.x, columns in the last block, grid.y, bias column)"""
    OH, OW, Dk = cv_geom(c)
    L = OH * OW
    return (ceil_div(L, 16), L % 16 or 16, ceil_div(Dk, 16), Dk % 16 or 16, ceil_div(c["Do"], 16), c["bias"])


def cv_id(c):
    return "B{B}-S{S}-Cin{Cin}-{H}x{W}-Do{Do}-k{k}-s{s}-p{p}-d{d}".format(**c).replace(" ", "") + ("-bias" if c["bias"] else "")


def cv_layout(c):
    """(P, col0, bcol0): two untouched columns in front, one between the ranges, two behind"""
    Dk = cv_geom(c)[2]
    n = c["Do"] * Dk
    return 2 + n + ((1 + c["Do"]) if c["bias"] else 0) + 2, 2, (2 + n + 1 if c["bias"] else -1)


def patches(x, c, clamp_top=False):
    """F.unfold of the zero-padded input, ``[B, Dk, L]``; ``clamp_top``: the first padding row above the image repeats the
    image's first row (the mutant that reads an out-of-image tap as its clamped neighbour)"""
    ph, pw = c["p"]
    xp = F.pad(x, (pw, pw, ph, ph))
    if clamp_top and ph > 0:
        xp[:, :, ph - 1, :] = xp[:, :, ph, :]
    return F.unfold(xp, c["k"], dilation=c["d"], padding=0, stride=c["s"])


def cv_reference(c):
    OH, OW, Dk = cv_geom(c)
    L = OH * OW
    x = _randn(c["B"], c["Cin"], c["H"], c["W"], seed=c["H"] + c["Cin"])
    g = _randn(c["S"], c["B"], c["Do"], OH, OW, seed=c["Do"] + L)
    cols, gl = patches(x, c), g.reshape(c["S"], c["B"], c["Do"], L)
    P, col0, bcol0 = cv_layout(c)
    ref = torch.full((c["B"], c["S"], P), NAN, dtype=torch.float64)
    bound = torch.zeros_like(ref)
    n = c["Do"] * Dk
    ref[:, :, col0:col0 + n] = torch.einsum("sbol,bkl->bsok", gl, cols).reshape(c["B"], c["S"], n)
    bound[:, :, col0:col0 + n] = gamma(L + 1) * torch.einsum("sbol,bkl->bsok", gl.abs(), cols.abs()).reshape(c["B"], c["S"], n)
    if c["bias"]:
        ref[:, :, bcol0:bcol0 + c["Do"]] = gl.sum(-1).permute(1, 0, 2)
        bound[:, :, bcol0:bcol0 + c["Do"]] = gamma(L) * gl.abs().sum(-1).permute(1, 0, 2)
    return x, g, ref, bound


def filled_ratio(got, ref, bound) -> float:
    """:func:`ratio` on the written columns; the others must still hold the NaN fill"""
    got = got.detach().double().cpu()
    keep = ref.isnan()
    if not bool(got[keep].isnan().all()):
        return float("inf")
    return ratio(got[~keep], ref[~keep], bound[~keep])


def check_jac_conv(K, dev, cases=None) -> dict:
    out = {}
    for c in (CV_CASES if cases is None else cases):
        x, g, ref, bound = cv_reference(c)
        P, col0, bcol0 = cv_layout(c)
        got = K.jac_conv(dev(x), dev(g), c, dev(torch.full(ref.shape, NAN, dtype=torch.float64)), col0, bcol0)
        out[cv_id(c)] = filled_ratio(got, ref, bound)
    return out


# ============================================================================================================================
# sq_colsum
# ============================================================================================================================
SQ_ALPHA = 1.25
SQ_CASES = [(rows, width, col0, after, start) for rows in (0, 1, 7) for width, col0, after, start in
            ((0, 0, 3, False), (255, 0, 0, True), (256, 2, 3, False), (257, 1, 5, True))]


def sq_form(rows, width):
    """(workgroups launched, rows summed)"""
    return (ceil_div(width, 256), rows)


def check_sq_colsum(K, dev, cases=None) -> dict:
    out = {}
    for rows, width, col0, after, start in (SQ_CASES if cases is None else cases):
        P = col0 + width + after
        Js = _randn(rows, P, seed=rows + width)
        h0 = f32(_randn(width, seed=width) * 20) if start else torch.zeros(width, dtype=torch.float64)
        t = SQ_ALPHA * (Js[:, col0:col0 + width] ** 2).sum(0)
        got = K.sq_colsum(dev(Js), rows, P, col0, width, SQ_ALPHA, dev(h0))
        out[f"rows{rows}-width{width}-col{col0}-P{P}" + ("-start" if start else "")] = ratio(
            got, h0 + t, gamma(rows + 3) * t + U * h0.abs())
    return out


# ============================================================================================================================
# vjp_scale_mask
# ============================================================================================================================
M_KINDS = ("bool", "u8", "float", None)
#: why a call takes the form it takes: name -> (B, C, HW, operand offset by one element)
VJP_REASONS = {
    "vec": (2, 3, 4, None),
    "vec-many": (2, 3, 172, None),       # per / 4 = 258 > 256: two workgroups
    "per%4": (1, 3, 5, None),
    "hw%4": (2, 2, 3, None),             # per = 12: the vector form unless a scale needs the channel
    "hw%4-many": (4, 2, 129, None),      # per = 1032, HW = 129
    "mis-g": (2, 3, 4, "g"), "mis-g2": (2, 3, 4, "g2"), "mis-out": (2, 3, 4, "out"), "mis-m": (2, 3, 4, "m"),
    "mis-g-many": (2, 3, 172, "g"),
}


def _vjp_cases():
    out, i = [], 0
    for reason, (B, C, HW, mis) in VJP_REASONS.items():
        for m in M_KINDS:
            for scale in (True, False):
                for g2 in (True, False):
                    if (mis == "g2" and not g2) or (mis == "m" and m is None):
                        continue
                    out.append(dict(reason=reason, S=(1, 3, 4, 2)[i % 4], B=B, C=C, HW=HW, mis=mis, m=m, scale=scale, g2=g2))
                    i += 1
    out.append(dict(reason="S0", S=0, B=2, C=3, HW=4, mis=None, m="bool", scale=True, g2=True))
    out.append(dict(reason="per0", S=2, B=0, C=3, HW=4, mis=None, m="float", scale=True, g2=False))
    return out


VJP_CASES = _vjp_cases()


def vjp_id(c):
    return f"{c['reason']}-S{c['S']}-m{c['m']}" + ("-scale" if c["scale"] else "") + ("-g2" if c["g2"] else "")


def vjp_form(c):
    """the form ``lk_vjp_scale_mask_f32`` launches: (None | "vec" | "scalar", workgroups).  Buffers start 16-byte aligned;
    an operand offset by one element (4 bytes; 1 byte for a byte multiplier) breaks its 16-byte (4-byte) requirement."""
    per = c["B"] * c["C"] * c["HW"]
    if c["S"] == 0 or per == 0:
        return (None, 0)
    mis = c["mis"] is not None and not (c["mis"] == "g2" and not c["g2"]) and not (c["mis"] == "m" and c["m"] is None)
    vec = per % 4 == 0 and (not c["scale"] or c["HW"] % 4 == 0) and not mis
    return ("vec", ceil_div(per // 4, 256)) if vec else ("scalar", ceil_div(per, 256))


def vjp_reference(c):
    S, C, HW = c["S"], c["C"], c["HW"]
    per = c["B"] * C * HW
    g = _randn(S, per, seed=per + S)
    g2 = _randn(S, per, seed=per + S + 1) if c["g2"] else None
    gen = torch.Generator().manual_seed(per + 2)
    m = m64 = None
    if c["m"] == "float":
        m = m64 = _randn(per, seed=per + 3)
    elif c["m"] is not None:
        bits = torch.rand(per, generator=gen) < 0.6
        m = bits if c["m"] == "bool" else bits.to(torch.uint8) * 255  # every non-zero byte is 255
        m64 = bits.double()
    scale = _randn(C, seed=C + 5) if c["scale"] else None
    v = g if g2 is None else g + g2
    if m64 is not None:
        v = v * m64
    if scale is not None:
        v = v * scale[(torch.arange(per) // HW) % C]
    return g, g2, m, scale, v


def check_vjp(K, dev, cases=None) -> dict:
    out = {}
    for c in (VJP_CASES if cases is None else cases):
        g, g2, m, scale, v = vjp_reference(c)
        per = c["B"] * c["C"] * c["HW"]
        got = K.vjp_scale_mask(dev(g), None if g2 is None else dev(g2), None if m is None else dev(m),
                               None if scale is None else dev(scale), c["S"], per, c["C"], c["HW"], mis=c["mis"])
        out[vjp_id(c)] = ratio(got, v, 3 * U * v.abs())
    return out


# ============================================================================================================================
# bn_act_forward
# ============================================================================================================================
BN_REASONS = {
    "vec": (2, 3, 4, None), "vec-many": (2, 3, 172, None), "hw%4": (2, 3, 5, None), "hw%4-many": (2, 4, 129, None),
    "mis-x": (2, 3, 4, "x"), "mis-y": (2, 3, 4, "y"), "mis-addend": (2, 3, 4, "addend"), "mis-mask": (2, 3, 4, "mask"),
}


def _bn_cases():
    out = []
    for reason, (B, C, HW, mis) in BN_REASONS.items():
        for relu in (True, False):
            for addend in (True, False):
                for want_mask in (True, False):
                    if (mis == "addend" and not addend) or (mis == "mask" and not (want_mask and relu)):
                        continue
                    out.append(dict(reason=reason, B=B, C=C, HW=HW, mis=mis, relu=relu, addend=addend, want_mask=want_mask))
    return out


BN_CASES = _bn_cases()


def bn_id(c):
    return c["reason"] + ("-relu" if c["relu"] else "") + ("-addend" if c["addend"] else "") + ("-mask" if c["want_mask"] else "")


def bn_form(c):
    """("vec" | "scalar", workgroups, relu): the mask pointer must be 4-byte aligned for the vector form, the others 16"""
    total = c["B"] * c["C"] * c["HW"]
    vec = c["HW"] % 4 == 0 and c["mis"] is None
    return ("vec" if vec else "scalar", ceil_div(total // 4 if vec else total, 256), c["relu"])


def bn_reference(c):
    B, C, HW = c["B"], c["C"], c["HW"]
    total = B * C * HW
    x = _randn(total, seed=total + 1)
    scale, shift = _randn(C, seed=C + 1), _randn(C, seed=C + 2)
    addend = _randn(total, seed=total + 2) if c["addend"] else None
    shift[0] = 0.0
    x[:2] = 0.0        # channel 0: a pre-activation of exactly 0
    if addend is not None:
        addend[:2] = 0.0
    ch = (torch.arange(total) // HW) % C
    pre = x * scale[ch] + shift[ch]
    mag = (x * scale[ch]).abs() + shift[ch].abs()
    if addend is not None:
        pre, mag = pre + addend, mag + addend.abs()
    return x, scale, shift, addend, pre, 3 * U * mag


def check_bn_act(K, dev, cases=None) -> dict:
    out = {}
    for c in (BN_CASES if cases is None else cases):
        x, scale, shift, addend, pre, bound = bn_reference(c)
        y, mask = K.bn_act_forward(dev(x), dev(scale), dev(shift), None if addend is None else dev(addend), c["C"], c["HW"],
                                   c["relu"], c["want_mask"], mis=c["mis"])
        v = ratio(y, pre.clamp_min(0) if c["relu"] else pre, bound)
        if c["relu"] and c["want_mask"]:
            mask = mask.detach().cpu()
            assert mask.dtype == torch.uint8
            y_pos = y.detach().cpu() > 0
            good = bool((mask <= 1).all()) and torch.equal(mask.bool(), y_pos)
            # the mask may differ from the reference's only where the pre-activation is within the bound of 0
            good = good and bool(((mask.bool() == (pre > 0)) | (pre.abs() <= bound)).all())
            if not good and v == v:
                v = float("inf")
        else:
            assert mask is None
        out[bn_id(c)] = v
    return out


# ============================================================================================================================
# a plain fp32 evaluation, and the mutants
# ============================================================================================================================
class Fp32Kernels:
    """torch float32 on the CPU, the formulas of the kernels; every method returns its outputs (``H0``, ``Js0``, ``h0``, ...
    are the contents the outputs start from).  ``mis`` (which operand the device test offsets by one element) is ignored."""

    #: the class-diagonal blocks of the last-layer GGN as Gram(sqrt(p_j) Pt) - Gram(p_j Pt) instead of Gram(sqrt(p_j s_j) Pt)
    subtracting = False

    # -- hooks the mutants override
    def _ref_index(self, j, a, C, D):
        return ref_index(j, a, C, D)

    def _mirror(self):
        return True

    def _channel(self, e, C, HW):
        return (e // HW) % C

    def _batch_end(self, B, chunk):
        return B

    def ll_ggn_full(self, phi, probs, C, has_bias, alpha, H0):
        B, D = phi.shape
        pt = torch.cat([phi, torch.ones(B, 1)], 1) if has_bias else phi
        Dt = pt.shape[1]
        P = C * Dt
        a32 = torch.tensor(alpha, dtype=torch.float32)
        Haug = torch.zeros(C, Dt, C, Dt)
        if probs is None:
            T = a32 * (pt.T @ pt)
            for j in range(C):
                Haug[j, :, j, :] = T
        else:
            Y = (probs.unsqueeze(2) * pt.unsqueeze(1)).reshape(B, P)
            G = (-a32) * (Y.T @ Y)
            Haug = G.reshape(C, Dt, C, Dt).clone()
            s = probs @ (1.0 - torch.eye(C))
            for j in range(C):
                if self.subtracting:
                    X = probs[:, j].sqrt().unsqueeze(1) * pt
                    Haug[j, :, j, :] += a32 * (X.T @ X)
                else:
                    X = (probs[:, j] * s[:, j]).sqrt().unsqueeze(1) * pt
                    Haug[j, :, j, :] = a32 * (X.T @ X)
            if not self._mirror():
                for j in range(C):
                    for k in range(j):
                        Haug[j, :, k, :] = 0.0
        perm = torch.tensor([self._ref_index(j, a, C, D) for j in range(C) for a in range(Dt)])
        H = H0.clone()
        H[perm[:, None], perm[None, :]] += Haug.reshape(P, P)
        return H

    def dense_quadform_ll(self, phi, Sigma, C, has_bias):
        B, D = phi.shape
        pt = torch.cat([phi, torch.ones(B, 1)], 1) if has_bias else phi
        Dt = pt.shape[1]
        perm = torch.tensor([self._ref_index(j, a, C, D) for j in range(C) for a in range(Dt)])
        Sa = Sigma[perm[:, None], perm[None, :]].reshape(C, Dt, C, Dt)
        fv = torch.einsum("np,cpkq,nq->nck", pt, Sa, pt)
        up = torch.triu(torch.ones(C, C, dtype=torch.bool))
        fv = torch.where(up, fv, fv.transpose(1, 2)) if self._mirror() else torch.where(up, fv, torch.zeros(()))
        end = self._batch_end(B, 128)
        fv[end:] = 0.0
        return fv

    def jac_last_layer(self, phi, C, has_bias):
        B, D = phi.shape
        P = C * D + (C if has_bias else 0)
        Js = torch.zeros(B, C, P)
        for i in range(C):
            Js[:, i, i * D:(i + 1) * D] = phi
            if has_bias:
                Js[:, i, self._ref_index(i, D, C, D)] = 1.0
        return Js

    def diag_ggn_linear(self, a, g, alpha, hw0, hb0):
        end = self._batch_end(a.shape[0], 64)
        a, g = a[:end], g[:, :end]
        gsq = (g * g).sum(0)
        a32 = torch.tensor(alpha, dtype=torch.float32)
        hw = hw0 + a32 * (gsq.T @ (a * a))
        return hw, (None if hb0 is None else hb0 + a32 * gsq.sum(0))

    def jac_linear(self, a, g, Js0, col0, bcol0):
        S, B, Do = g.shape
        Js = Js0.clone()
        Js[:, :, col0:col0 + Do * a.shape[1]] = (g.permute(1, 0, 2).unsqueeze(3) * a[:, None, None, :]).reshape(B, S, -1)
        if bcol0 >= 0:
            Js[:, :, bcol0:bcol0 + Do] = g.permute(1, 0, 2)
        return Js

    def _patches(self, x, c):
        return patches(x, c)

    def jac_conv(self, x, g, c, Js0, col0, bcol0):
        S, B, Do = g.shape[:3]
        cols = self._patches(x, c)
        gl = g.reshape(S, B, Do, -1)
        end = self._batch_end(gl.shape[-1], 16)
        cols, gl = cols[:, :, :end], gl[..., :end]
        Js = Js0.clone()
        Js[:, :, col0:col0 + Do * cols.shape[1]] = torch.einsum("sbol,bkl->bsok", gl, cols).reshape(B, S, -1)
        if bcol0 >= 0:
            Js[:, :, bcol0:bcol0 + Do] = gl.sum(-1).permute(1, 0, 2)
        return Js

    def _rows(self, rows):
        return rows

    def sq_colsum(self, Js, rows, P, col0, width, alpha, h0):
        v = Js.reshape(rows, P)[:self._rows(rows), col0:col0 + width]
        return h0 + torch.tensor(alpha, dtype=torch.float32) * (v * v).sum(0)

    def vjp_scale_mask(self, g, g2, m, scale, S, per, C, HW, mis=None):
        mult = torch.ones(per) if m is None else (m if m.dtype == torch.float32 else (m != 0).float())
        if scale is not None:
            mult = mult * scale[self._channel(torch.arange(per), C, HW)]
        v = g if g2 is None else g + g2
        return v.reshape(S, per) * mult

    def bn_act_forward(self, x, scale, shift, addend, C, HW, relu, want_mask, mis=None):
        ch = self._channel(torch.arange(x.numel()), C, HW)
        y = x * scale[ch] + shift[ch]
        if addend is not None:
            y = y + addend
        if relu:
            y = y.clamp_min(0)
        return y, ((y > 0).to(torch.uint8) if relu and want_mask else None)


class SubtractingGGN(Fp32Kernels):
    """the class-diagonal blocks as a difference of two separately rounded fp32 Grams"""
    subtracting = True


class DropsLastChunk(Fp32Kernels):
    """the last partial batch chunk is dropped: 64 samples in diag_ggn_linear, 16 positions in jac_conv, the tail of a
    128-sample tile in dense_quadform_ll"""

    def _batch_end(self, B, chunk):
        return B - B % chunk


class BiasInAugmentedColumn(Fp32Kernels):
    """the bias entry lands at j * Dt + D instead of C * D + j"""

    def _ref_index(self, j, a, C, D):
        return j * (D + 1) + a if a == D else ref_index(j, a, C, D)


class NotMirrored(Fp32Kernels):
    """a class pair (c, k), c < k, is not mirrored to (k, c)"""

    def _mirror(self):
        return False


class ChannelFromElement(Fp32Kernels):
    """the channel of the element-wise kernels taken as e % C"""

    def _channel(self, e, C, HW):
        return e % C


class ClampedTap(Fp32Kernels):
    """the out-of-image row just above the image is read as the image's first row instead of 0"""

    def _patches(self, x, c):
        return patches(x, c, clamp_top=True)


class SkipsLastRow(Fp32Kernels):
    """the squared-column sum skips its last row"""

    def _rows(self, rows):
        return max(rows - 1, 0)


#: mutant -> the checks at least one of whose cases must leave its bound
MUTANTS = {
    DropsLastChunk: ("check_diag_linear", "check_jac_conv", "check_quadform"),
    BiasInAugmentedColumn: ("check_ll_ggn", "check_jac_last_layer", "check_quadform"),
    NotMirrored: ("check_ll_ggn", "check_quadform"),
    ChannelFromElement: ("check_vjp", "check_bn_act"),
    ClampedTap: ("check_jac_conv",),
    SkipsLastRow: ("check_sq_colsum",),
}
CHECKS = ("check_ll_ggn", "check_quadform", "check_jac_last_layer", "check_diag_linear", "check_jac_linear", "check_jac_conv",
          "check_sq_colsum", "check_vjp", "check_bn_act")


# ============================================================================================================================
# a model whose forward pass is exact in fp32
# ============================================================================================================================
MODEL_C, MODEL_D, MODEL_B = 5, 12, 16
#: head scale -> logit margin on the model's own inputs: 2^4 gives a median margin of 15, 1 moderate logits (median margin 1)
MODEL_SCALES = {"saturated": 16.0, "moderate": 1.0}


def exact_mlp(kind: str):
    """``(model64, X64, y)``: Linear(6, 12) - ReLU - Linear(12, 5) whose inputs are multiples of 1/4 in [-2, 2] and whose
    weights are multiples of 1/8 (the head's times a power of two), so that every product and partial sum of the forward
    pass is a number fp32 holds: the fp32 model returns the features and logits of the fp64 model bit for bit and the
    GGN's only inexact inputs are the probabilities"""
    from torch import nn

    g = torch.Generator().manual_seed(31)
    q = lambda *s, step, lim: torch.randint(-lim, lim + 1, s, generator=g).double() * step
    model = nn.Sequential(nn.Linear(6, MODEL_D), nn.ReLU(), nn.Linear(MODEL_D, MODEL_C)).double()
    with torch.no_grad():
        model[0].weight.copy_(q(MODEL_D, 6, step=0.125, lim=8))
        model[0].bias.copy_(q(MODEL_D, step=0.125, lim=8))
        model[2].weight.copy_(q(MODEL_C, MODEL_D, step=0.125, lim=8) * MODEL_SCALES[kind])
        model[2].bias.copy_(q(MODEL_C, step=0.125, lim=8) * MODEL_SCALES[kind])
    pool = q(40 * MODEL_B, 6, step=0.25, lim=8)
    y = torch.randint(MODEL_C, (MODEL_B,), generator=g)
    # the inputs whose margin at the saturated scale lies in [10, 20] (the same inputs for both scales): past a margin of ~25
    # the fp64 oracle's own diag(p) - p p^T has no digits left to compare with
    with torch.no_grad():
        top = (model(pool) * (MODEL_SCALES["saturated"] / MODEL_SCALES[kind])).topk(2, 1).values
    keep = ((top[:, 0] - top[:, 1]) >= 10) & ((top[:, 0] - top[:, 1]) <= 20)
    X = pool[keep][:MODEL_B]
    assert X.shape[0] == MODEL_B
    return model.eval(), X, y


def model_bound(phi, p, bias=True):
    """the element bound of ``ll_ggn_full`` for one minibatch whose probabilities are the device's fp32 softmax of exact
    logits instead of the rounding of the fp64 softmax.  Each probability then carries C + 4 roundings where the kernel
    cases count 1: f - max is exact, exp is within one ulp (2 u), the partition sum carries that and C - 1 additions, and the
    division 1.  Class pairs j != k: 7 - 2 + 2 (C + 4) = 2 C + 13; j == j: the root's argument carries p_j (C + 4), s_j
    (C + 4 and its C - 2 additions) and the product (1), 3 C + 7, plus the 7 that follow as in the kernel cases: 3 C + 14.

    A model's unlikely classes reach p ~ 1e-30 and products of two of them leave fp32's range (the kernel cases keep every
    entry above 1e-30, tests/lik_fixtures.py), which no relative bound covers: every rounding may in addition lose up to the
    smallest normal number, 2^-126, carried to the output by factors that are at most max(1, |pt_a|) max(1, |pt_b|)."""
    B, D = phi.shape
    C = p.shape[1]
    pt = torch.cat([phi, torch.ones(B, 1, dtype=torch.float64)], 1) if bias else phi
    Dt = pt.shape[1]
    idx = torch.arange(C)
    Lam = -p.unsqueeze(2) * p.unsqueeze(1)
    Lam[:, idx, idx] = p * LF._others(p)
    e = torch.full((C, C), 2.0 * C + 13)
    e[idx, idx] = 3.0 * C + 14
    PP = (pt.unsqueeze(2) * pt.unsqueeze(1)).abs().reshape(B, Dt * Dt)
    A = (Lam.abs().reshape(B, C * C).T @ PP).reshape(C, C, Dt, Dt).permute(0, 2, 1, 3).reshape(C * Dt, C * Dt)
    perm = ref_perm(C, D, Dt)
    out = torch.zeros_like(A)
    k = (B + e.double()).repeat_interleave(Dt, 0).repeat_interleave(Dt, 1)
    big = pt.abs().clamp(min=1.0)
    under = (big.T @ big).repeat(C, C) * 2.0 ** -126
    out[perm[:, None], perm[None, :]] = gamma(k) * A + k * under
    return out


def model_figures(kind: str, run_batch):
    """``run_batch(X, y, phi, f) -> H`` of one minibatch (fp64 arguments; ``phi``, ``f`` the exact features and logits).  Two
    minibatches of 8, summed in fp64, against the oracle's dense GGN: (element error / summed bound, smallest eigenvalue,
    ||bound||_F, negative diagonal entries, log det (H + 1e-4 I), the oracle's)"""
    from oracle import curvature_oracle as co

    m64, X, y = exact_mlp(kind)
    with torch.no_grad():
        f, phi = m64(X), m64[:2](X)
    H = want = bound = 0.0
    for s in (slice(0, 8), slice(8, 16)):
        H = H + run_batch(X[s], y[s], phi[s], f[s]).detach().double().cpu()
        Js = co.last_layer_jacobians(phi[s], MODEL_C, True)
        want = want + co.ggn_full(Js, co.functional_hessian(f[s], "classification"))
        bound = bound + model_bound(phi[s], torch.softmax(f[s], 1))
    eye = 1e-4 * torch.eye(H.shape[0], dtype=torch.float64)
    return (ratio(H, want, bound), torch.linalg.eigvalsh((H + H.T) / 2).min().item(), torch.linalg.norm(bound).item(),
            int((H.diagonal() < 0).sum()), torch.linalg.slogdet(H + eye)[1].item(), torch.linalg.slogdet(want + eye)[1].item())
