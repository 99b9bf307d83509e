"""Three tiny models with TRACKED grouped convolutions, for the grouped-convolution goldens (tools/make_gconv_golden.py) and
their parity tests.

TEST INFRASTRUCTURE, in the style of tests/norm_fixtures.py (batch 10, seed 711, input [10, 2, 6, 6], 3 outputs; weights and
data are stored inside the golden files):
  * ``gcsep`` (P = 333): conv, depthwise with channel multiplier 2 and stride 2, 1x1, a dilated 2-group conv without bias
  * ``gcres`` (P = 267): conv, a MobileNetV2 inverted residual (1x1 expand, BN, ReLU6, depthwise 3x3, BN, ReLU6, 1x1 project,
    BN, ``+ x``) with every BatchNorm parameter tracked and stirred statistics, eval mode
  * ``gcdw7`` (P = 339): 1x1 conv, depthwise 7x7 with padding 3 on a 6x6 map (every tap partly outside), GELU
"""
from __future__ import annotations

import os

import numpy as np
import torch
from torch import nn

from tests.norm_fixtures import _stir, ef_gradients_from_golden, forbid_generic_route, rel  # noqa: F401  (re-exported)

GCONV_FIXTURES = ("gcsep", "gcres", "gcdw7")
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
#: names of the grouped-convolution modules of each fixture
GROUPED = {"gcsep": ["2", "6"], "gcres": ["1.block.3"], "gcdw7": ["1"]}


class InvertedResidual(nn.Module):
    """MobileNetV2 block, stride 1, with the identity shortcut"""

    def __init__(self, c: int, expand: int):
        super().__init__()
        h = c * expand
        self.block = nn.Sequential(
            nn.Conv2d(c, h, 1, bias=False), nn.BatchNorm2d(h), nn.ReLU6(),
            nn.Conv2d(h, h, 3, padding=1, groups=h, bias=False), nn.BatchNorm2d(h), nn.ReLU6(),
            nn.Conv2d(h, c, 1, bias=False), nn.BatchNorm2d(c))

    def forward(self, x):
        return x + self.block(x)


def build_model(name: str) -> nn.Module:
    if name == "gcsep":
        return nn.Sequential(nn.Conv2d(2, 4, 3, padding=1), nn.Tanh(),
                             nn.Conv2d(4, 8, 3, stride=2, padding=1, groups=4), nn.Tanh(),
                             nn.Conv2d(8, 6, 1), nn.Tanh(),
                             nn.Conv2d(6, 4, 3, padding=2, dilation=2, groups=2, bias=False), nn.Tanh(),
                             nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(4, 3)).eval()
    if name == "gcres":
        return _stir(nn.Sequential(nn.Conv2d(2, 4, 3, padding=1), InvertedResidual(4, 2), nn.AdaptiveAvgPool2d(1),
                                   nn.Flatten(), nn.Linear(4, 3)))
    if name == "gcdw7":
        return nn.Sequential(nn.Conv2d(2, 6, 1), nn.Conv2d(6, 6, 7, padding=3, groups=6), nn.GELU(),
                             nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(6, 3)).eval()
    raise KeyError(name)


N_PARAMS = {"gcsep": 333, "gcres": 267, "gcdw7": 339}


def make_fixture(name: str, dtype=torch.float64, batch: int = 10, seed: int = 711):
    """Fresh model + (X, y_cls, y_reg), as oracle/fixtures.py:make_fixture."""
    torch.manual_seed(seed)
    model = build_model(name).to(dtype)
    torch.manual_seed(seed)
    X = torch.randn(batch, 2, 6, 6, dtype=dtype)
    y_cls = torch.randint(3, (batch,))
    y_reg = torch.randn(batch, 3, dtype=dtype)
    return model, X, y_cls, y_reg


def load_golden(name: str, likelihood: str) -> dict:
    """the arrays of ``<name>_<likelihood>.npz`` and of its companions ``<name>_<likelihood>.<key>.npz`` (the dense
    matrices, one per file)"""
    import glob

    out = {}
    stem = os.path.join(GOLDEN_DIR, f"{name}_{likelihood}")
    for path in [stem + ".npz"] + sorted(glob.glob(glob.escape(stem) + ".*.npz")):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


def golden_model(name: str, g: dict, dtype=torch.float32, device="cpu"):
    """the fixture with the golden file's weights / buffers, ``(model, X, y)`` in ``dtype`` on ``device``"""
    model = build_model(name).to(torch.float64)
    model.load_state_dict({k[2:]: torch.as_tensor(v) for k, v in g.items() if k.startswith("w.")})
    model = model.to(dtype).to(device).eval()
    X = torch.as_tensor(g["X"], dtype=dtype, device=device)
    y = torch.as_tensor(g["y"])
    y = y.to(device) if not y.is_floating_point() else y.to(dtype).to(device)
    return model, X, y


def count_gconv_calls(monkeypatch):
    """wrap the active kernel object's ``jac_gconv``; returns the list that receives one entry per call"""
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    inner, calls = K.jac_gconv, []

    def counted(*a, **kw):
        calls.append(1)
        return inner(*a, **kw)

    monkeypatch.setattr(K, "jac_gconv", counted, raising=False)
    return calls


def route_check(monkeypatch, dev: str):
    """With the generic route forbidden, every non-KFAC entry point of the three models runs on the kernels, and the
    grouped-convolution kernel is called once per grouped tap and backend call."""
    from torch.utils.data import DataLoader, TensorDataset

    from laplace_amd import HipEF, HipGGN
    from laplace_amd.laplace import HipLaplace

    forbid_generic_route(monkeypatch)
    calls = count_gconv_calls(monkeypatch)
    for name in GCONV_FIXTURES:
        for lik in ("classification", "regression"):
            g = load_golden(name, lik)
            model, X, y = golden_model(name, g, device=dev)
            b = HipGGN(model, lik)
            tape = b._tape()
            assert [t.name for t in tape.gconv_taps] == GROUPED[name]
            assert all(t.module.groups == 1 for t in tape.taps if t.kind == "conv2d")
            n_g = len(tape.gconv_taps)
            assert b._supported()
            seen = len(calls)
            for call in (lambda: b.jacobians(X), lambda: b.diag(X, y), lambda: b.full(X, y)):
                call()
                assert len(calls) == seen + n_g, f"{name}: {len(calls) - seen} jac_gconv calls for {n_g} grouped taps"
                seen = len(calls)
            e = HipEF(model, lik)
            assert e._supported()
            for call in (lambda: e.gradients(X, y), lambda: e.diag(X, y), lambda: e.full(X, y)):
                call()
                assert len(calls) == seen + n_g
                seen = len(calls)
            la = HipLaplace(model, lik, "all", "diag", prior_precision=0.7)
            la.fit(DataLoader(TensorDataset(X, y), batch_size=5))
            assert len(calls) == seen + 2 * n_g  # (two minibatches)
            seen = len(calls)

            def no_jacobians(*a, **kw):
                raise AssertionError("the diagonal predictive fell back to backend.jacobians")

            monkeypatch.setattr(la.backend, "jacobians", no_jacobians)
            f_mu, f_var = la._glm_predictive_distribution(X)
            assert len(calls) == seen + n_g
            assert torch.isfinite(f_var).all() and f_var.shape == (len(X), f_mu.shape[1], f_mu.shape[1])
