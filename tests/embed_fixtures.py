"""Two tiny token models with a TRACKED nn.Embedding weight and a tracked lone parameter, for the embedding goldens
(tools/make_embed_golden.py) and their parity tests, and the table of kernel cases of tests/test_gpu_embed.py.

TEST INFRASTRUCTURE, in the style of tests/gconv_fixtures.py (batch 10, seed 711, 3 outputs; weights and data are stored inside
the golden files):
  * ``tok_mean`` (P = 159): ``Embedding(11, 6, padding_idx=0)`` plus a ``[1, 5, 6]`` position parameter, ``Linear(6, 6)`` with tanh,
    the mean over the tokens, ``Linear(6, 3)``
  * ``tok_cls`` (P = 227): ``Embedding(9, 4)`` without a padding row, a trainable class token through ``expand`` + ``cat``, one
    pre-LN attention block (one head, every LayerNorm parameter tracked), the head on ``x[:, 0]``
The ids are drawn so that every row repeats an id, rows share ids and (``tok_mean``) a row holds the padding id; `make_fixture`
asserts it.
"""
from __future__ import annotations

import os

import torch
from torch import nn

from tests.gconv_fixtures import load_golden  # noqa: F401  (re-exported: the same file layout)
from tests.norm_fixtures import ef_gradients_from_golden, forbid_generic_route, rel  # noqa: F401  (re-exported)

EMBED_FIXTURES = ("tok_mean", "tok_cls")
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_PARAMS = {"tok_mean": 159, "tok_cls": 227}
VOCAB = {"tok_mean": 11, "tok_cls": 9}
T_TOKENS = 5
#: attribute path of each fixture's lone parameter
LONE = {"tok_mean": "pos", "tok_cls": "cls"}


class TokMean(nn.Module):
    def __init__(self):
        super().__init__()
        self.embed = nn.Embedding(11, 6, padding_idx=0)
        self.pos = nn.Parameter(torch.randn(1, T_TOKENS, 6) * 0.5)
        self.fc = nn.Linear(6, 6)
        self.head = nn.Linear(6, 3)

    def forward(self, ids):
        x = self.embed(ids) + self.pos
        return self.head(torch.tanh(self.fc(x)).mean(1))


class TokCls(nn.Module):
    def __init__(self):
        super().__init__()
        self.embed = nn.Embedding(9, 4)
        from laplace_amd.nets import AttentionBlock  # (not at import time: the package is imported when a test runs, as elsewhere)

        self.cls = nn.Parameter(torch.randn(1, 1, 4) * 0.5)
        self.block = AttentionBlock(4, 1, mlp_ratio=2.0)
        self.head = nn.Linear(4, 3)

    def forward(self, ids):
        x = self.embed(ids)
        x = torch.cat([self.cls.expand(x.size(0), -1, -1), x], 1)
        return self.head(self.block(x)[:, 0])


def build_model(name: str) -> nn.Module:
    if name == "tok_mean":
        return TokMean().eval()
    if name == "tok_cls":
        return TokCls().eval()
    raise KeyError(name)


def draw_ids(name: str, batch: int = 10, seed: int = 711) -> torch.Tensor:
    """ids ``[batch, 5]``: random, then position 3 of every row repeats position 1 and (``tok_mean``) row 0 starts with the
    padding id; the properties the goldens are meant to pin are asserted"""
    V = VOCAB[name]
    gen = torch.Generator().manual_seed(seed)
    ids = torch.randint(1 if name == "tok_mean" else 0, V, (batch, T_TOKENS), generator=gen)
    ids[:, 3] = ids[:, 1]
    if name == "tok_mean":
        ids[0, 0] = 0
        ids[4, 2] = 0
        ids[4, 4] = 0
    rows = [set(r.tolist()) for r in ids]
    assert all(len(r) < T_TOKENS for r in rows), "every row repeats at least one id"
    assert sum(len(rows[i] & rows[j]) > 0 for i in range(batch) for j in range(i)) >= 1, "at least two rows share an id"
    if name == "tok_mean":
        assert any(0 in r for r in rows), "a row holds the padding id"
    return ids


def make_fixture(name: str, dtype=torch.float64, batch: int = 10, seed: int = 711):
    """Fresh model + (ids, y_cls, y_reg), as oracle/fixtures.py:make_fixture."""
    torch.manual_seed(seed)
    model = build_model(name).to(dtype)
    with torch.no_grad():  # (an untrained embedding's padding row is zero; every other row is what the seed gave)
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))  # (LayerNorm affines off their 1 / 0 defaults)
    X = draw_ids(name, batch, seed)
    torch.manual_seed(seed + 1)
    y_cls = torch.randint(3, (batch,))
    y_reg = torch.randn(batch, 3, dtype=dtype)
    return model, X, y_cls, y_reg


def golden_model(name: str, g: dict, dtype=torch.float32, device="cpu"):
    """the fixture with the golden file's weights, ``(model, ids, y)``: the model in ``dtype``, the ids int64, on ``device``"""
    model = build_model(name).to(torch.float64)
    model.load_state_dict({k[2:]: torch.as_tensor(v) for k, v in g.items() if k.startswith("w.")})
    model = model.to(dtype).to(device).eval()
    X = torch.as_tensor(g["X"], dtype=torch.int64, device=device)
    y = torch.as_tensor(g["y"])
    y = y.to(device) if not y.is_floating_point() else y.to(dtype).to(device)
    return model, X, y


# ---- kernel cases (tests/test_gpu_embed.py runs them on the device, tests/test_embed_fixtures.py proves what they reach) ----
def _case(name, S=2, B=3, T=7, D=4, V=5, pad=None, ids="random", misalign=False, col0=0, tail=0, kernels=("jac", "diag", "quad")):
    return dict(name=name, S=S, B=B, T=T, D=D, V=V, pad=pad, ids=ids, misalign=misalign, col0=col0, tail=tail, kernels=kernels)


#: one value per axis varied at a time around S=2, B=3, T=7, D=4, V=5; ``ids``: "random" (ids 0 and V-1 forced in), "equal",
#: "distinct", "oob" (one id outside the table), "skew" (a single id everywhere)
KERNEL_CASES = [
    _case("base"),
    _case("T1", T=1), _case("T7_equal", ids="equal"), _case("T7_distinct", V=9, ids="distinct"), _case("T64", T=64),
    _case("D1", D=1), _case("D3", D=3), _case("D64", D=64), _case("D65", D=65), _case("D260", D=260),
    _case("S1", S=1), _case("S9", S=9),
    _case("B1", B=1),
    _case("V1", V=1), _case("V2", V=2), _case("V1000", V=1000, T=64),
    _case("pad_in_data", pad=0), _case("pad_unused", pad=4, ids="low"),
    _case("oob", ids="oob"),
    _case("misaligned", misalign=True), _case("misaligned_D64", D=64, misalign=True),
    _case("col0", col0=8, tail=4), _case("col0_odd", col0=3, tail=2),
    _case("S17_quad_tiles", S=17, D=8, kernels=("quad",)),
    _case("skew_4096", S=2, B=64, T=64, D=8, V=3, ids="skew", kernels=("diag",)),
]


def make_case(c: dict, device="cpu", integer: bool = False, seed: int = 5):
    """``(g [S, B, T, D] fp32, ids [B, T] int64, var [V*D] fp32)`` of a kernel case.  ``integer``: values in [-8, 8], for which every
    partial sum of the three kernels is exact in fp32.  ``misalign``: ``g`` is a view one float into its storage."""
    gen = torch.Generator().manual_seed(seed + sum(map(ord, c["name"])))
    S, B, T, D, V = c["S"], c["B"], c["T"], c["D"], c["V"]
    if c["ids"] == "equal":
        ids = torch.full((B, T), V // 2, dtype=torch.int64)
    elif c["ids"] == "skew":
        ids = torch.full((B, T), 1, dtype=torch.int64)
    elif c["ids"] == "distinct":
        ids = torch.stack([torch.randperm(V, generator=gen)[:T] for _ in range(B)])
    else:
        ids = torch.randint(0, V - 1 if c["ids"] == "low" and V > 1 else V, (B, T), generator=gen)
        if c["ids"] == "random" and B * T >= 2:
            ids.view(-1)[0], ids.view(-1)[-1] = 0, V - 1
        if c["ids"] == "oob":
            ids[0, 0], ids[-1, -1] = V, -1
    n = S * B * T * D
    flat = torch.randint(-8, 9, (n + 1,), generator=gen).float() if integer else torch.randn(n + 1, generator=gen)
    var = (torch.randint(1, 9, (V * D,), generator=gen).float() if integer else torch.rand(V * D, generator=gen) + 0.1)
    flat, ids, var = flat.to(device), ids.to(device), var.to(device)
    g = flat[1:].view(S, B, T, D) if c["misalign"] else flat[:n].view(S, B, T, D)
    return g, ids, var


def case_P(c: dict) -> int:
    return c["col0"] + c["V"] * c["D"] + c["tail"]


def sentinel_js(c: dict, device="cpu", value: float = 7.5):
    """``Js [B, S, P]`` filled with a sentinel; ``misalign``: a view one float into its storage (needs a contiguous tensor of
    its own, so the sample pitch stays ``S * P``)"""
    n = c["B"] * c["S"] * case_P(c)
    flat = torch.full((n + 1,), value, dtype=torch.float32, device=device)
    return (flat[1:] if c["misalign"] else flat[:n]).view(c["B"], c["S"], case_P(c))


def gamma(k):
    """``gamma_k = k u / (1 - k u)``, ``u = 2^-24`` (a tensor or a number of roundings)"""
    u = 2.0 ** -24
    return k * u / (1 - k * u)


# ---- the checks of a kernel case (their reasoning: the docstring of tests/test_gpu_embed.py) ---------------------------------
SENTINEL = 7.5
_REF_CACHE: dict = {}


def reference(c: dict, device, integer: bool):
    """inputs of a case and, computed once in float64: the run sums ``R [S, B, V, D]``, the same on ``|g|`` (``A``), which
    (sample, id) pairs are written (``hit [B, V]``) and the run lengths (``count [B, V]``)"""
    from tests.emulated_embed_kernels import run_sums

    key = (c["name"], str(device), integer)
    if key not in _REF_CACHE:
        _REF_CACHE.clear()  # (one case's tensors at a time)
        g, ids, var = make_case(c, device, integer=integer)
        R, hit = run_sums(g.double(), ids, c["V"], c["pad"])
        A, _ = run_sums(g.double().abs(), ids, c["V"], c["pad"])
        ones = torch.ones(1, c["B"], c["T"], 1, dtype=torch.float64, device=g.device)
        count = run_sums(ones, ids, c["V"], c["pad"])[0][0, :, :, 0]
        _REF_CACHE[key] = (g, ids, var, R, A, hit, count)
    return _REF_CACHE[key]


def check_jac_case(K, c: dict, device, integer: bool):
    g, ids, var, R, A, hit, count = reference(c, device, integer)
    S, B, D, V, col0 = c["S"], c["B"], c["D"], c["V"], c["col0"]
    Js = sentinel_js(c, device, SENTINEL)
    assert Js.shape[-1] == case_P(c)
    K.jac_embed(g, ids, V, c["pad"], Js, col0)
    block = Js[:, :, col0:col0 + V * D].reshape(B, S, V, D)
    mask = hit[:, None, :, None].expand(B, S, V, D)
    # sentinel: columns outside the weight, and every (sample, id) that heads no non-padding run
    assert bool((Js[:, :, :col0] == SENTINEL).all()) and bool((Js[:, :, col0 + V * D:] == SENTINEL).all())
    assert bool((block[~mask] == SENTINEL).all()), "an element that no run owns was written"
    want = R.permute(1, 0, 2, 3)
    if integer:
        assert float(A.max()) < 2 ** 24  # (every partial sum is exact)
        assert torch.equal(block[mask].double(), want[mask]), "integer-valued cotangents: not bit-equal to the float64 sums"
    else:
        k = (count - 1).clamp(min=0)[:, None, :, None].expand(B, S, V, D)
        bound = gamma(k) * A.permute(1, 0, 2, 3)
        err = (block.double() - want).abs()
        print(f"{c['name']}: worst err / bound {float((err[mask] / bound[mask].clamp(min=1e-300)).max()) if mask.any() else 0:.3f}")
        assert bool((err[mask] <= bound[mask]).all()), "outside the order-free bound of its own sum"
    Js2 = sentinel_js(c, device, SENTINEL)
    K.jac_embed(g, ids, V, c["pad"], Js2, col0)
    assert torch.equal(Js, Js2), "two launches on the same data differ"


def check_diag_case(K, c: dict, device, integer: bool):
    g, ids, var, R, A, hit, count = reference(c, device, integer)
    S, D, V = c["S"], c["D"], c["V"]
    alpha = 0.5
    want = 3.0 + alpha * (R * R).sum((0, 1)).reshape(-1)
    mag = 3.0 + alpha * (A * A).sum((0, 1)).reshape(-1)

    def fresh():  # (h += : the kernel adds to what is there; misaligned cases: one float into the storage)
        flat = torch.full((V * D + 1,), 3.0, dtype=torch.float32, device=g.device)
        return flat[1:] if c["misalign"] else flat[:V * D]

    h = fresh()
    K.diag_embed(g, ids, V, c["pad"], alpha, h)
    untouched = ~hit.any(0)[:, None].expand(V, D).reshape(-1)
    assert bool((h[untouched] == 3.0).all()), "a row of the table that no run owns was written"
    if integer:
        assert float(mag.max()) < 2 ** 24  # (every partial sum is exact)
        assert torch.equal(h.double(), want), "integer-valued cotangents: not bit-equal to the float64 result"
    else:
        L = count.max(0).values  # [V] longest run of the id
        m = S * hit.sum(0).double()  # [V] nonzero (s, b) terms
        k = (2 * (L - 1).clamp(min=0) + 1 + (m - 1).clamp(min=0) + 2)[:, None].expand(V, D).reshape(-1)
        err = (h.double() - want).abs()
        print(f"{c['name']}: worst err / bound {float((err / (gamma(k) * mag)).max()):.3f}")
        assert bool((err <= gamma(k) * mag).all()), "outside the order-free bound of its own sum"
    h2 = fresh()
    K.diag_embed(g, ids, V, c["pad"], alpha, h2)
    assert torch.equal(h2, h), "two launches on the same data differ"


def check_quad_case(K, c: dict, device, integer: bool):
    g, ids, var, R, A, hit, count = reference(c, device, integer)
    C, B, D, V = c["S"], c["B"], c["D"], c["V"]
    v64 = var.double().reshape(V, D)
    want = 1.0 + torch.einsum("cbvd,kbvd,vd->bck", R, R, v64)
    mag = 1.0 + torch.einsum("cbvd,kbvd,vd->bck", A, A, v64.abs())
    fvar = torch.ones(B, C, C, dtype=torch.float32, device=g.device)  # (fvar += )
    K.diag_quadform_embed(g, ids, V, c["pad"], var, fvar)
    if integer:
        assert float(mag.max()) < 2 ** 24  # (every partial sum is exact)
        assert torch.equal(fvar.double(), want), "integer-valued cotangents: not bit-equal to the float64 result"
    else:
        L = count.max(1).values  # [B] longest run of the row
        m = hit.sum(1).double() * D  # [B] terms
        k = (2 * (L - 1).clamp(min=0) + 2 + (m - 1).clamp(min=0) + 1)[:, None, None]
        err = (fvar.double() - want).abs()
        print(f"{c['name']}: worst err / bound {float((err / (gamma(k) * mag)).max()):.3f}")
        assert bool((err <= gamma(k) * mag).all()), "outside the order-free bound of its own sum"
    fvar2 = torch.ones(B, C, C, dtype=torch.float32, device=g.device)
    K.diag_quadform_embed(g, ids, V, c["pad"], var, fvar2)
    assert torch.equal(fvar2, fvar), "two launches on the same data differ"
