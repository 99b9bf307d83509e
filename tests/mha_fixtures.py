"""Tiny models built from nn.MultiheadAttention and the stock transformer encoder, their twins written with nn.Linear, and the
curvature checks both tiers run on them (tests/test_sweep_mha.py on the emulation, tests/test_gpu_mha.py on the device).

TEST INFRASTRUCTURE.  ``E = 8``, ``H = 2`` (head dim 4, the smallest the kernels take), ``T = 6``, ``B = 9``.  A TWIN computes
the same function of the same parameter vector in the same order with the packed projection written as ``nn.Linear(E, 3 E)``,
``F.scaled_dot_product_attention`` and ``nn.Linear(E, E)``, declared in the real model's module order so that the blocks of
``oracle.kfac_ggn`` line up.  The oracle's hooks cannot see the real module's projections (its forward reads the raw weights),
so the reference's KFAC of the twin's two weight-sharing Linear layers is the definition of the module's factors;
tests/test_sweep_mha.py proves each twin equal to its model to 1e-12 in fp64."""
from __future__ import annotations

import copy

import torch
import torch.nn.functional as F
from torch import nn

from tests.attn_fixtures import _Loader, rel

E, H, T, B, FF = 8, 2, 6, 9, 16


# ---- the models ---------------------------------------------------------------------------------------------------------------------
class MhaBlock(nn.Module):
    """[B, 6, 5] -> Linear(5, 8) -> x + MultiheadAttention(x, x, x)[0] -> mean over positions -> Linear"""

    def __init__(self, C=3, need_weights=False, **mha_kw):
        super().__init__()
        self.embed = nn.Linear(5, E)
        self.attn = nn.MultiheadAttention(E, H, batch_first=True, **mha_kw)
        self.head = nn.Linear(E, C)
        self.need_weights = need_weights

    def forward(self, x):
        x = self.embed(x)
        return self.head((x + self.attn(x, x, x, need_weights=self.need_weights)[0]).mean(1))


class EncoderLayerNet(nn.Module):
    """[B, 6, 5] -> Linear(5, 8) -> one nn.TransformerEncoderLayer -> mean over positions -> Linear"""

    def __init__(self, C=3, norm_first=False, activation="relu"):
        super().__init__()
        self.embed = nn.Linear(5, E)
        self.layer = nn.TransformerEncoderLayer(E, H, FF, 0.0, activation, batch_first=True, norm_first=norm_first)
        self.head = nn.Linear(E, C)

    def forward(self, x):
        return self.head(self.layer(self.embed(x)).mean(1))


class EncoderNet(nn.Module):
    """[B, 6, 5] -> Linear(5, 8) -> nn.TransformerEncoder of 2 pre-norm GELU layers with a final LayerNorm -> mean -> Linear"""

    def __init__(self, C=3):
        super().__init__()
        self.embed = nn.Linear(5, E)
        layer = nn.TransformerEncoderLayer(E, H, FF, 0.0, "gelu", batch_first=True, norm_first=True)
        self.encoder = nn.TransformerEncoder(layer, 2, norm=nn.LayerNorm(E), enable_nested_tensor=False)
        self.head = nn.Linear(E, C)

    def forward(self, x):
        return self.head(self.encoder(self.embed(x)).mean(1))


# ---- the twins ----------------------------------------------------------------------------------------------------------------------
class TwinMha(nn.Module):
    """unmasked self-attention nn.MultiheadAttention(E, H, batch_first=True) as Linear(E, 3 E), SDPA on H heads, Linear(E, E)"""

    def __init__(self, m: nn.MultiheadAttention):
        super().__init__()
        self.H = m.num_heads
        dt = m.in_proj_weight.dtype
        self.in_proj = nn.Linear(m.embed_dim, 3 * m.embed_dim, bias=m.in_proj_bias is not None, dtype=dt)
        self.out_proj = nn.Linear(m.embed_dim, m.embed_dim, bias=m.out_proj.bias is not None, dtype=dt)
        with torch.no_grad():
            for dst, src in ((self.in_proj.weight, m.in_proj_weight), (self.in_proj.bias, m.in_proj_bias),
                             (self.out_proj.weight, m.out_proj.weight), (self.out_proj.bias, m.out_proj.bias)):
                if dst is not None:
                    dst.copy_(src)
                    dst.requires_grad_(src.requires_grad)

    def forward(self, x):
        Bn, Tn, En = x.shape
        q, k, v = self.in_proj(x).view(Bn, Tn, 3, self.H, En // self.H).permute(2, 0, 3, 1, 4).unbind(0)
        return self.out_proj(F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(Bn, Tn, En))


class TwinLayer(nn.Module):
    """nn.TransformerEncoderLayer (batch_first, dropout 0) with its attention as a `TwinMha`; the sub-modules in the layer's order"""

    def __init__(self, layer: nn.TransformerEncoderLayer):
        super().__init__()
        self.self_attn = TwinMha(layer.self_attn)
        self.linear1, self.linear2 = copy.deepcopy(layer.linear1), copy.deepcopy(layer.linear2)
        self.norm1, self.norm2 = copy.deepcopy(layer.norm1), copy.deepcopy(layer.norm2)
        self.norm_first, self.act = layer.norm_first, layer.activation

    def forward(self, x):
        ff = lambda t: self.linear2(self.act(self.linear1(t)))  # noqa: E731
        if self.norm_first:
            x = x + self.self_attn(self.norm1(x))
            return x + ff(self.norm2(x))
        x = self.norm1(x + self.self_attn(x))
        return self.norm2(x + ff(x))


class Twin(nn.Module):
    """the twin of one of the three model classes: the same attributes in the same order"""

    def __init__(self, model):
        super().__init__()
        self.embed = copy.deepcopy(model.embed)
        if isinstance(model, MhaBlock):
            self.attn = TwinMha(model.attn)
        elif isinstance(model, EncoderLayerNet):
            self.layer = TwinLayer(model.layer)
        else:
            self.layers = nn.ModuleList(TwinLayer(layer) for layer in model.encoder.layers)
            self.norm = copy.deepcopy(model.encoder.norm)
        self.head = copy.deepcopy(model.head)

    def forward(self, x):
        x = self.embed(x)
        if hasattr(self, "attn"):
            x = x + self.attn(x)
        elif hasattr(self, "layer"):
            x = self.layer(x)
        else:
            for layer in self.layers:
                x = layer(x)
            x = self.norm(x)
        return self.head(x.mean(1))


MODELS = ("mha", "post-norm", "pre-norm", "encoder")


def make_model(name, C=3, seed=3, **kw):
    """``(model fp32 in eval mode, its fp64 TWIN, inputs [9, 6, 5] fp32)``; the LayerNorm affines are moved away from the identity
    and frozen (KFAC refuses tracked ones); ``kw``: further arguments of the model class"""
    torch.manual_seed(seed)
    if name == "mha":
        model = MhaBlock(C, **kw)
    elif name == "encoder":
        model = EncoderNet(C, **kw)
    else:
        model = EncoderLayerNet(C, norm_first=name == "pre-norm", **{"activation": "gelu" if name == "pre-norm" else "relu", **kw})
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.LayerNorm):
                m.weight.add_(0.3 * torch.randn_like(m.weight))
                m.bias.add_(0.3 * torch.randn_like(m.bias))
                m.weight.requires_grad_(False), m.bias.requires_grad_(False)
            if isinstance(m, nn.MultiheadAttention):  # (torch initialises the biases of both projections to zero)
                m.in_proj_bias.add_(0.2 * torch.randn_like(m.in_proj_bias))
                m.out_proj.bias.add_(0.2 * torch.randn_like(m.out_proj.bias))
    model.eval()
    X = torch.randn(B, T, 5)
    return model, Twin(copy.deepcopy(model).double()).eval(), X


def tap_names(name):
    """the names of the 'linear' taps of a fixture model, in ``named_modules`` order"""
    layer = lambda p: [f"{p}self_attn.in_proj", f"{p}self_attn.out_proj", f"{p}linear1", f"{p}linear2"]  # noqa: E731
    mid = {"mha": ["attn.in_proj", "attn.out_proj"], "encoder": layer("encoder.layers.0.") + layer("encoder.layers.1.")}
    return ["embed"] + mid.get(name, layer("layer.")) + ["head"]


def run_curvature_checks(dev, name, lik, configure=None, expect_sweep=True, model_kw=None):
    """the body of tests/attn_fixtures.run_curvature_checks on a fixture model of this file: jacobians, diag, full, a
    two-minibatch kron fit, the Kron and the diagonal predictive against the fp64 oracle RUN ON THE TWIN at the same bars
    (1e-5 for the output, 1e-4 for everything else) - and the proof that the sweep produced them (``expect_sweep``; ``False``:
    that it did not).  ``configure(backend)`` sets switches on every backend object; returns what the routes are compared by."""
    from laplace_amd import HipGGN
    from laplace_amd.laplace import HipLaplace
    from oracle import curvature_oracle as co

    C = 3 if lik == "classification" else 2
    model, m64, X = make_model(name, C, **(model_kw or {}))
    model, X = model.to(dev), X.to(dev)
    torch.manual_seed(11)
    y = torch.randint(C, (B,)).to(dev) if lik == "classification" else torch.randn(B, C).to(dev)
    X64, y64 = X.double().cpu(), (y.cpu() if lik == "classification" else y.double().cpu())
    Js64, f64 = co.jacobians(m64, X64)
    Hl = co.functional_hessian(f64, lik)
    configure = configure or (lambda b: None)

    def swept(backend):
        tape = backend._tape()
        built = any(s not in (None, False) for s in tape.sweeps.values())
        if expect_sweep:
            assert getattr(tape, "sweep_reason", None) is None, tape.sweep_reason
            assert built, "no sweep was built"
        else:
            assert not built, "a sweep was built"
        assert tape.uncovered == [] and [t.name for t in tape.taps] == tap_names(name)

    backend = HipGGN(model, lik)
    configure(backend)
    Js, f = backend.jacobians(X)
    assert rel(f, f64) < 1e-5 and rel(Js, Js64) < 1e-4
    _, h = backend.diag(X, y)
    assert rel(h, co.ggn_diag(Js64, Hl)) < 1e-4
    _, Hf = backend.full(X, y)
    assert rel(Hf, co.ggn_full(Js64, Hl)) < 1e-4
    swept(backend)

    loader = _Loader([(X[:5], y[:5]), (X[5:], y[5:])])
    loader.dataset = range(B)
    la = HipLaplace(model, lik, "all", "kron", prior_precision=0.7)
    configure(la.backend)
    la.fit(loader)
    want = None
    for xb, yb in ((X64[:5], y64[:5]), (X64[5:], y64[5:])):
        _, kf = co.kfac_ggn(m64, xb, yb, B, lik)
        want = kf if want is None else co.kron_add(want, kf)
    assert len(la.H_facs.kfacs) == len(want)
    for F_, G_ in zip(la.H_facs.kfacs, want):
        assert len(F_) == len(G_)
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
    return dict(Js=Js, f=f, h=h, H=Hf, f_var=f_var, f_var_d=f_var_d, kfacs=[t for F_ in la.H_facs.kfacs for t in F_])
