"""nn.Embedding weights and lone parameters (class token, position table) on the device route - host logic on the kernel
emulation (tests/emulated_embed_kernels.py) against the goldens of the unmodified reference (tools/make_embed_golden.py).

Tolerance: 1e-4 max-normalised, the bar of every golden test here (BASELINE.json north_star).
"""
import copy

import pytest
import torch
from torch import nn
from torch.utils.data import DataLoader, TensorDataset

from oracle.make_golden import PRIOR_PREC, SIGMA_NOISE
from tests.embed_fixtures import (EMBED_FIXTURES, LONE, N_PARAMS, VOCAB, ef_gradients_from_golden, forbid_generic_route, golden_model,
                                  load_golden, rel)

LIKS = ("classification", "regression")
CASES = [(n, l) for n in EMBED_FIXTURES for l in LIKS]
TOL = 1e-4
SHIPPED_DEFAULT = []  # what the fixture below found before it switched the route on


@pytest.fixture(autouse=True)
def _switch_on(monkeypatch):
    """the route ships opt-in: every test of this file runs with the class default switched on"""
    from laplace_amd.backend import _HipCurvatureMixin

    SHIPPED_DEFAULT.append(_HipCurvatureMixin.__dict__["use_embed_kernels"])
    monkeypatch.setattr(_HipCurvatureMixin, "use_embed_kernels", True)


def test_the_route_is_opt_in():
    from laplace_amd import HipEF, HipGGN

    assert SHIPPED_DEFAULT and all(v is False for v in SHIPPED_DEFAULT)
    assert "use_embed_kernels" not in HipGGN.__dict__ and "use_embed_kernels" not in HipEF.__dict__


@pytest.fixture
def embed_kernels():
    from laplace_amd import _lib
    from tests.emulated_embed_kernels import EmulatedEmbedKernels

    prev = _lib.set_kernels_for_testing(EmulatedEmbedKernels())
    yield
    _lib.set_kernels_for_testing(prev)


@pytest.fixture
def gconv_only_kernels():
    from laplace_amd import _lib
    from tests.emulated_gconv_kernels import EmulatedGConvKernels

    prev = _lib.set_kernels_for_testing(EmulatedGConvKernels())
    yield
    _lib.set_kernels_for_testing(prev)


def check(got, want, what):
    e = rel(got, want)
    print(f"{what}: {e:.3e}")
    assert e < TOL, f"{what}: rel err {e:.3e}"


def spy_jacrev(monkeypatch):
    used, inner = [], torch.func.jacrev

    def spy(*a, **kw):
        used.append(1)
        return inner(*a, **kw)

    monkeypatch.setattr(torch.func, "jacrev", spy)
    return used


@pytest.mark.parametrize("use_sweep", (True, False))
@pytest.mark.parametrize("name,lik", CASES)
def test_ggn_and_ef_against_reference_golden(embed_kernels, name, lik, use_sweep):
    """on the sweep both the embedding and the lone parameter are served; on the tape the embedding is and the lone parameter
    sends the model to the generic route - both must match the reference"""
    from laplace_amd import HipEF, HipGGN

    g = load_golden(name, lik)
    assert g["Js"].shape[-1] == N_PARAMS[name]
    model, X, y = golden_model(name, g)
    assert X.dtype == torch.int64
    b = HipGGN(model, lik)
    b.use_sweep = use_sweep
    tape = b._tape()
    assert [t.name for t in tape.embed_taps] == ["embed"] and [t.name for t in tape.param_taps] == [LONE[name]]
    assert b._supported() == use_sweep
    Js, f = b.jacobians(X)
    check(Js, g["Js"], "jacobians")
    check(f, g["f"], "f")
    if use_sweep:
        assert getattr(tape, "sweep_reason", None) is None
        assert [t.kind for t in b._served_taps(tape)][-2:] == ["embed", "param"]
    else:
        assert [t.kind for t in tape.active_taps(b._route(tape))][-1] == "embed"  # (served on the tape; the lone parameter is not)
    loss, H = b.full(X, y)
    check(H, g["H_ggn"], "full GGN")
    check(loss, g["loss"], "loss")
    loss, h = b.diag(X, y)
    check(h, g["h_ggn"], "diag GGN")
    check(b.diag(X[:5], y[:5])[1] + b.diag(X[5:], y[5:])[1], g["h_ggn"], "diag additivity")
    e = HipEF(model, lik)
    e.use_sweep = use_sweep
    loss, H = e.full(X, y)
    check(H, g["H_ef"], "full EF")
    check(loss, g["loss_ef"], "EF loss")
    check(e.diag(X, y)[1], g["h_ef"], "diag EF")
    Gs, loss = e.gradients(X, y)
    check(Gs, ef_gradients_from_golden(g, lik), "EF gradients")


@pytest.mark.parametrize("name,lik", CASES)
def test_embedding_alone_is_served_on_the_tape(embed_kernels, name, lik, monkeypatch):
    """with the lone parameter frozen the autograd tape serves the model: module output hook -> g, module input -> ids"""
    from laplace_amd import HipGGN

    g = load_golden(name, lik)
    model, X, y = golden_model(name, g)
    getattr(model, LONE[name]).requires_grad_(False)
    off, cols = 0, []  # the golden's columns without the lone parameter's
    for n, p in golden_model(name, g)[0].named_parameters():
        if n != LONE[name]:
            cols += list(range(off, off + p.numel()))
        off += p.numel()
    assert off == N_PARAMS[name]
    forbid_generic_route(monkeypatch)
    for use_sweep in (True, False):
        b = HipGGN(model, lik)
        b.use_sweep = use_sweep
        assert b._supported() and b._tape().param_taps == []
        check(b.jacobians(X)[0], g["Js"][:, :, cols], f"jacobians (sweep {use_sweep})")
        check(b.diag(X, y)[1], g["h_ggn"][cols], f"diag (sweep {use_sweep})")


@pytest.mark.parametrize("hs", ("diag", "full"))
@pytest.mark.parametrize("name,lik", CASES)
def test_laplace_all_against_reference_golden(embed_kernels, name, lik, hs, monkeypatch):
    """(the backend class is handed over: ``HipLaplace``'s default is bound when laplace.py is imported, and the fixture that
    re-derives the boundary classes from the reference's, ``reference_dropin``, leaves it on the classes from before its reload)"""
    from laplace_amd import HipGGN
    from laplace_amd.laplace import HipLaplace

    g = load_golden(name, lik)
    model, X, y = golden_model(name, g)
    forbid_generic_route(monkeypatch)
    la = HipLaplace(model, lik, "all", hs, backend=HipGGN, prior_precision=PRIOR_PREC,
                    sigma_noise=SIGMA_NOISE if lik == "regression" else 1.0)
    la.fit(DataLoader(TensorDataset(X, y), batch_size=5))
    assert la.backend._supported() and getattr(la.backend._tape(), "sweep_reason", None) is None
    tag = f"la.all.{hs}"
    check(la.loss, g[f"{tag}.loss"], "loss")
    check(la.H, g[f"{tag}.H"], "accumulated H")
    f_mu, f_var = la._glm_predictive_distribution(X)
    check(f_mu, g[f"{tag}.f_mu"], "f_mu")
    check(f_var, g[f"{tag}.f_var"], "f_var")
    check(la.log_marginal_likelihood(), g[f"{tag}.marglik"], "marglik")


def test_direct_paths_never_form_the_embedding_block(embed_kernels, monkeypatch):
    """``diag`` goes through ``diag_embed`` and the diagonal predictive through ``diag_quadform_embed``: ``jac_embed`` is not called"""
    from laplace_amd import HipGGN
    from laplace_amd._lib import get_kernels
    from laplace_amd.predictive import glm_variance_diag

    K = get_kernels()
    calls = []
    for fn in ("jac_embed", "diag_embed", "diag_quadform_embed"):
        def counted(*a, _fn=fn, _inner=getattr(K, fn), **kw):
            calls.append(_fn)
            return _inner(*a, **kw)
        monkeypatch.setattr(K, fn, counted, raising=False)
    g = load_golden("tok_mean", "classification")
    model, X, y = golden_model("tok_mean", g)
    b = HipGGN(model, "classification")
    b.diag(X, y)
    assert calls == ["diag_embed"]
    post_var = torch.rand(N_PARAMS["tok_mean"], generator=torch.Generator().manual_seed(2)) + 0.1
    _, fvar = glm_variance_diag(b, X, post_var)
    assert calls == ["diag_embed", "diag_quadform_embed"]
    Js = torch.as_tensor(g["Js"])
    check(fvar, torch.einsum("ncp,p,nkp->nck", Js, post_var.double(), Js), "diagonal predictive")
    b.jacobians(X)
    assert calls[-1] == "jac_embed"


# ---- refusals of capture.Tape ------------------------------------------------------------------------------------------
class _Tok(nn.Module):
    def __init__(self, embed, head_in=4):
        super().__init__()
        self.embed = embed
        self.head = nn.Linear(head_in, 3)

    def forward(self, ids):
        return self.head(self.embed(ids).mean(1))


class _Tied(nn.Module):
    def __init__(self):
        super().__init__()
        self.embed = nn.Embedding(7, 4)
        self.mid = nn.Linear(4, 4)
        self.head = nn.Linear(4, 7, bias=False)
        self.head.weight = self.embed.weight

    def forward(self, ids):
        return self.head(torch.tanh(self.mid(self.embed(ids).mean(1))))


class _Bag(nn.Module):
    def __init__(self):
        super().__init__()
        self.embed = nn.EmbeddingBag(7, 4, mode="mean")
        self.head = nn.Linear(4, 3)

    def forward(self, ids):
        return self.head(self.embed(ids))


@pytest.mark.parametrize("what,build,match", [
    ("max_norm", lambda: _Tok(nn.Embedding(7, 4, max_norm=1.0)), r"^embed: nn\.Embedding is not served \(max_norm"),
    ("scale_grad_by_freq", lambda: _Tok(nn.Embedding(7, 4, scale_grad_by_freq=True)), r"^embed: .*scale_grad_by_freq"),
    ("sparse", lambda: _Tok(nn.Embedding(7, 4, sparse=True)), r"^embed: .*sparse=True"),
    ("tied", _Tied, r"^embed: .*tied to a Linear"),
    ("bag", _Bag, r"^embed: nn\.EmbeddingBag has no device rule"),
])
def test_tape_refuses_by_name(embed_kernels, what, build, match):
    import re

    from laplace_amd import HipGGN

    torch.manual_seed(0)
    model = build().eval()
    b = HipGGN(model, "classification")
    tape = b._tape()
    assert tape.embed_taps == []
    assert re.search(match, tape.embed_refused["embed"]), tape.embed_refused
    if what == "tied":
        assert b._supported()  # (the Linear head owns the weight: it is a covered parameter, and the tape serves the model)
    else:
        assert not b._supported()
        assert any(p is model.embed.weight for p in b._unserved(tape))


# ---- refusals of the sweep's parameter rule -----------------------------------------------------------------------------
class _Lone(nn.Module):
    """Embedding(7, 4) on ids [B, 3], one lone parameter ``p`` used as ``how`` says, mean over tokens, Linear head"""

    def __init__(self, how, shape):
        super().__init__()
        self.how = how
        self.embed = nn.Embedding(7, 4)
        self.p = nn.Parameter(torch.randn(*shape))
        self.buf = nn.Buffer(torch.arange(3))
        self.postab = nn.Embedding(3, 4)
        self.head = nn.Linear(4, 3)

    def forward(self, ids):
        x = self.embed(ids)
        if self.how == "add":
            x = x + self.p
        elif self.how == "radd":
            x = self.p + x
        elif self.how == "mul":
            x = x * self.p
        elif self.how == "matmul":
            x = x @ self.p
        elif self.how == "layer_norm":
            x = nn.functional.layer_norm(x, (4,), self.p)
        elif self.how == "expand":
            x = x + self.p.expand(x.size(0), 3, -1)
        elif self.how == "postab":
            x = x + self.postab(self.buf)
        return self.head(x.mean(1))


@pytest.mark.parametrize("how,shape,match", [
    ("add", (4,), r"parameter p: add broadcasts \(4,\) along a non-batch dim.*needs a reduction"),
    ("add", (1, 1, 4), r"parameter p: add broadcasts \(1, 1, 4\) along a non-batch dim.*needs a reduction"),
    ("mul", (1, 3, 4), r"parameter p: a product with a tracked parameter \(LayerScale\) has no rule"),
    ("matmul", (4, 4), r"parameter p: matmul with a tracked parameter has no rule"),
    ("layer_norm", (4,), r"parameter p: no VJP rule for function layer_norm"),
    ("expand", (1, 1, 4), r"parameter p: expand broadcasts \(1, 1, 4\) along a non-batch dim.*needs a reduction"),
    ("postab", (1, 3, 4), r"postab: Embedding of a constant index buffer with a tracked weight has no rule"),
])
def test_sweep_refuses_and_names_the_parameter(embed_kernels, how, shape, match, monkeypatch):
    from laplace_amd import HipGGN
    from laplace_amd.sweep import SeedBatchedSweep, SweepUnsupported

    torch.manual_seed(1)
    model = _Lone(how, shape).eval()
    (model.p if how == "postab" else model.postab.weight).requires_grad_(False)  # (the one the forward does not read)
    ids = torch.randint(0, 7, (4, 3))
    with pytest.raises(SweepUnsupported, match=match):
        SeedBatchedSweep(model, {"embed": model.embed, "head": model.head, "p": None}).forward(ids)
    # the backend then leaves the parameter unserved, exactly as without the rule: the generic route computes the model
    used = spy_jacrev(monkeypatch)
    b = HipGGN(model, "classification")
    Js, _ = b.jacobians(ids)
    assert used and not b._supported()
    m64 = copy.deepcopy(model).double()
    params = [p for p in m64.parameters() if p.requires_grad]
    want = torch.stack([torch.stack([torch.cat([g.flatten() for g in torch.autograd.grad(m64(ids[n:n + 1])[0, c], params)])
                                     for c in range(3)]) for n in range(4)])
    check(Js, want, "jacobians on the generic route")


@pytest.mark.parametrize("how,shape", [("add", (1, 3, 4)), ("add", (3, 4)), ("radd", (1, 3, 4))])
def test_position_table_spellings_are_served(embed_kernels, how, shape, monkeypatch):
    from laplace_amd import HipGGN

    torch.manual_seed(2)
    model = _Lone(how, shape).eval()
    model.postab.weight.requires_grad_(False)
    ids = torch.randint(0, 7, (4, 3))
    forbid_generic_route(monkeypatch)
    b = HipGGN(model, "classification")
    assert b._supported()
    Js, _ = b.jacobians(ids)
    m64 = copy.deepcopy(model).double()
    params = [p for p in m64.parameters() if p.requires_grad]
    want = torch.stack([torch.stack([torch.cat([g.flatten() for g in torch.autograd.grad(m64(ids[n:n + 1])[0, c], params)])
                                     for c in range(3)]) for n in range(4)])
    check(Js, want, "jacobians")


def test_frozen_position_embedding_of_a_buffer_is_a_constant(embed_kernels):
    from laplace_amd.sweep import CONST, SeedBatchedSweep

    torch.manual_seed(3)
    model = _Lone("postab", (1, 3, 4)).eval()
    model.postab.weight.requires_grad_(False)
    model.p.requires_grad_(False)
    sweep = SeedBatchedSweep(model, {"embed": model.embed, "head": model.head})
    kinds = {n.target: r.kind for n, r in sweep.rule.items() if n.op == "call_module"}
    assert kinds["postab"] == CONST and kinds["embed"] == "embedding"
    ids = torch.randint(0, 7, (4, 3))
    assert torch.allclose(sweep.forward(ids), model(ids), atol=1e-6)


def test_split_sweep_names_the_nodes(embed_kernels):
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep_nhwc import SplitSweep

    g = load_golden("tok_mean", "classification")
    model, X, y = golden_model("tok_mean", g)
    sweep = SplitSweep(model, {"embed": model.embed, "fc": model.fc, "head": model.head, "pos": None}, kernels=get_kernels)
    assert not sweep.split_ok and sweep.split_reason == "embed: Embedding has no NHWC rule"

    class Img(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = nn.Conv2d(3, 32, 3, padding=1)
            self.bias = nn.Parameter(torch.zeros(1, 32, 4, 4))
            self.head = nn.Linear(32, 3)

        def forward(self, x):
            return self.head((self.conv(x) + self.bias).mean((2, 3)))

    m = Img().eval()
    sweep = SplitSweep(m, {"conv": m.conv, "head": m.head, "bias": None}, kernels=get_kernels)
    assert not sweep.split_ok and sweep.split_reason == "parameter bias has no NHWC rule"


# ---- the switch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EMBED_FIXTURES)
def test_switch_off_reproduces_the_generic_route(embed_kernels, name, monkeypatch):
    from laplace_amd import HipGGN

    g = load_golden(name, "classification")
    model, X, y = golden_model(name, g)
    used = spy_jacrev(monkeypatch)
    b = HipGGN(model, "classification")
    b.use_embed_kernels = False
    tape = b._tape()
    assert not b._supported() and len(b._unserved(tape)) == 2
    assert [t.kind for t in tape.active_taps(b._route(tape)) if t.kind in ("embed", "param")] == []
    Js, _ = b.jacobians(X)
    assert used
    check(Js, g["Js"], "jacobians")
    check(b.diag(X, y)[1], g["h_ggn"], "diag")
    assert not any(r & {"embed", "param"} for r in tape.sweeps)  # (no sweep was built for the new taps)


def test_kernel_object_without_the_entry_point_takes_the_generic_route(gconv_only_kernels, monkeypatch):
    from laplace_amd import HipGGN
    from laplace_amd._lib import get_kernels

    assert getattr(get_kernels(), "jac_embed", None) is None
    used = spy_jacrev(monkeypatch)
    g = load_golden("tok_cls", "classification")
    model, X, y = golden_model("tok_cls", g)
    b = HipGGN(model, "classification")
    assert not b._supported()
    Js, _ = b.jacobians(X)
    assert used and rel(Js, g["Js"]) < TOL


def test_switch_reaches_the_fp32_twin(embed_kernels):
    from laplace_amd import HipGGN

    g = load_golden("tok_mean", "classification")
    model, X, y = golden_model("tok_mean", g, dtype=torch.float64)
    b = HipGGN(model, "classification")
    twin, dt = b._twin()
    assert dt == torch.float64 and twin.use_embed_kernels and twin._supported()
    Js, _ = b.jacobians(X)
    assert Js.dtype == torch.float64
    check(Js, g["Js"], "jacobians of the fp64 model")
    b.use_embed_kernels = False
    twin, _ = b._twin()
    assert twin.use_embed_kernels is False and not twin._supported()


# ---- KFAC ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frozen", ("pos", "embed.weight"))
def test_kfac_refuses_tracked_embeddings_and_lone_parameters(embed_kernels, frozen):
    from laplace_amd import HipEF, HipGGN
    from laplace_amd.predictive import glm_variance_kron

    g = load_golden("tok_mean", "classification")
    model, X, y = golden_model("tok_mean", g)
    dict(model.named_parameters())[frozen].requires_grad_(False)  # (each of the two refuses on its own)
    for b in (HipGGN(model, "classification"), HipEF(model, "classification")):
        with pytest.raises(NotImplementedError, match=r"KFAC supports nn\.Linear / nn\.Conv2d parameters only"):
            b.kron(X, y, N=len(X))
        with pytest.raises(NotImplementedError, match=r"KFAC supports nn\.Linear / nn\.Conv2d parameters only"):
            b.kron_accumulator(len(X)).add_batch(X, y)
    with pytest.raises(NotImplementedError):
        glm_variance_kron(HipGGN(model, "classification"), X, None)


@pytest.mark.parametrize("name", EMBED_FIXTURES)
def test_kron_with_frozen_tokens_runs_on_the_sweep(embed_kernels, name):
    from laplace_amd import HipGGN
    from laplace_amd.sweep import SeedBatchedSweep

    g = load_golden(name, "classification")
    model, X, y = golden_model(name, g)
    model.embed.weight.requires_grad_(False)
    getattr(model, LONE[name]).requires_grad_(False)
    for m in model.modules():
        if isinstance(m, nn.LayerNorm):
            for p in m.parameters():
                p.requires_grad_(False)
    b = HipGGN(model, "classification")
    tape = b._tape()
    assert tape.embed_taps == [] and tape.param_taps == [] and b._supported()
    loss, kron = b.kron(X, y, N=len(X))
    assert getattr(tape, "sweep_reason", None) is None and isinstance(tape.sweep, SeedBatchedSweep)  # ONE reverse pass
    t = HipGGN(model, "classification")
    t.use_sweep = False
    loss_t, kron_t = t.kron(X, y, N=len(X))
    assert not getattr(t._tape(), "sweep", None)
    assert rel(loss, loss_t) < 1e-5
    for F, Ft in zip(kron.kfacs, kron_t.kfacs):
        for A, At in zip(F, Ft):
            assert rel(A, At) < 1e-5


def test_batched_grid_search_falls_back_to_the_loop(embed_kernels):
    from laplace_amd import HipGGN
    from laplace_amd.laplace import HipLaplace
    from laplace_amd.predictive import glm_variance_diag_grid

    g = load_golden("tok_mean", "classification")
    model, X, y = golden_model("tok_mean", g)
    loader = DataLoader(TensorDataset(X, y), batch_size=5)
    picks = []
    for batched in (True, False):
        la = HipLaplace(model, "classification", "all", "diag", backend=HipGGN)
        la.fit(loader)
        picks.append(float(la.gridsearch_prior_precision(loader, grid_size=5, batched=batched)))
    assert picks[0] == picks[1]
    with pytest.raises(NotImplementedError):
        glm_variance_diag_grid(la.backend, X, la.H, [0.1, 1.0])


# ---- workloads -----------------------------------------------------------------------------------------------------------
def test_vit_class_token_default_is_unchanged(embed_kernels):
    from laplace_amd import HipGGN
    from laplace_amd.nets import ViTClassToken

    torch.manual_seed(0)
    m = ViTClassToken(num_classes=3, image=8, patch=4, dim=8, depth=1, heads=1).eval()
    assert not m.cls.requires_grad and "pos" in dict(m.named_buffers()) and "pos" not in dict(m.named_parameters())
    assert sorted(k for k in m.state_dict() if "." not in k) == ["cls", "pos"]
    b = HipGGN(m, "classification")
    tape = b._tape()
    assert tape.param_taps == [] and tape.embed_taps == [] and b._supported()
    x = torch.randn(2, 3, 8, 8)
    loss, kron = b.kron(x, torch.tensor([0, 2]), N=2)
    assert getattr(tape, "sweep_reason", None) is None and tape.sweep and torch.isfinite(loss)


def test_vit_class_token_trained_tokens_are_served(embed_kernels, monkeypatch):
    from laplace_amd import HipGGN
    from laplace_amd.nets import ViTClassToken

    torch.manual_seed(0)
    m = ViTClassToken(num_classes=3, image=8, patch=4, dim=8, depth=1, heads=1, train_tokens=True, freeze_norm=False).eval()
    assert m.cls.requires_grad and m.pos.requires_grad and tuple(m.pos.shape) == (1, 5, 8)
    x = torch.randn(3, 3, 8, 8)
    forbid_generic_route(monkeypatch)
    b = HipGGN(m, "classification")
    tape = b._tape()
    assert sorted(t.name for t in tape.param_taps) == ["cls", "pos"] and b._supported()
    Js, _ = b.jacobians(x)
    assert getattr(tape, "sweep_reason", None) is None
    m64 = copy.deepcopy(m).double()
    params = [p for p in m64.parameters() if p.requires_grad]
    want = torch.stack([torch.stack([torch.cat([g.flatten() for g in torch.autograd.grad(m64(x[n:n + 1].double())[0, c], params)])
                                     for c in range(3)]) for n in range(3)])
    check(Js, want, "jacobians")
    y = torch.tensor([0, 1, 2])
    h = b.diag(x, y)[1]
    H = b.full(x, y)[1]
    check(h, torch.diagonal(H), "diag against the diagonal of full")
    with pytest.raises(NotImplementedError, match="KFAC supports"):
        b.kron(x, y, N=3)


def test_text_transformer_defaults_and_flags():
    from laplace_amd.nets import TextTransformer

    m = TextTransformer()
    assert (m.embed.num_embeddings, m.embed.embedding_dim, m.embed.padding_idx) == (1000, 192, 0)
    assert tuple(m.pos.shape) == (1, 64, 192) and len(m.blocks) == 6 and m.blocks[0].heads == 3 and m.head.out_features == 10
    assert m.embed.weight.requires_grad and m.pos.requires_grad and not m.norm.weight.requires_grad
    f = TextTransformer(vocab=20, T=4, dim=8, depth=1, heads=1, num_classes=3, freeze_embed=True, freeze_norm=False)
    assert not f.embed.weight.requires_grad and not f.pos.requires_grad and f.norm.weight.requires_grad
    assert f(torch.randint(0, 20, (2, 4))).shape == (2, 3)


def test_emulation_agrees_with_autograd(embed_kernels):
    """the emulation itself (the witness of the device tests) against per-sample autograd weight gradients"""
    from laplace_amd._lib import get_kernels

    torch.manual_seed(4)
    V, D = 6, 3
    m = nn.Embedding(V, D, padding_idx=2).double()
    ids = torch.tensor([[1, 1, 5, 2], [0, 5, 5, 5]])
    g = torch.randn(3, 2, 4, D, dtype=torch.float64)
    Js = torch.full((2, 3, V * D + 5), 7.5, dtype=torch.float64)
    K = get_kernels()
    K.jac_embed(g, ids, V, 2, Js, 2)
    want = torch.zeros(2, 3, V * D, dtype=torch.float64)
    for n in range(2):
        for s in range(3):
            (gw,) = torch.autograd.grad(m(ids[n:n + 1]), m.weight, g[s, n:n + 1])
            want[n, s] = gw.flatten()
    hit = torch.zeros(2, V, dtype=torch.bool)
    hit[0, [1, 5]] = True
    hit[1, [0, 5]] = True
    mask = hit[:, None, :, None].expand(2, 3, V, D).reshape(2, 3, V * D)
    assert torch.allclose(Js[:, :, 2:2 + V * D][mask], want[mask], atol=1e-12)
    assert bool((Js[:, :, 2:2 + V * D][~mask] == 7.5).all()) and bool((Js[:, :, :2] == 7.5).all()) and bool((Js[:, :, -3:] == 7.5).all())
    h = torch.zeros(V * D, dtype=torch.float64)
    K.diag_embed(g, ids, V, 2, 0.5, h)
    assert torch.allclose(h, 0.5 * (want ** 2).sum((0, 1)), atol=1e-12)
    var = torch.rand(V * D, dtype=torch.float64)
    fvar = K.diag_quadform_embed(g, ids, V, 2, var, torch.zeros(2, 3, 3, dtype=torch.float64))
    assert torch.allclose(fvar, torch.einsum("ncp,p,nkp->nck", want, var, want), atol=1e-12)
