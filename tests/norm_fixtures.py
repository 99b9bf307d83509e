"""Three tiny models whose normalisation layers carry TRACKED affine parameters, with non-trivial statistics and affine
values, for the norm-parameter goldens (tools/make_norm_golden.py) and their parity tests.

TEST INFRASTRUCTURE, in the style of oracle/fixtures.py (batch 10, seed 711; weights and data are stored inside the
golden files):
  * ``normbn``: conv, torchvision-style BatchNorm residual block (in-place add / ReLU, eval mode), pool, linear
  * ``normln``: ``Linear(5, 8)`` along a sequence of 4, ``LayerNorm(8)``, tanh, mean over positions, ``Linear(8, 2)``
  * ``normgn``: conv to 8 channels, ``GroupNorm(2, 8)``, ReLU, pool, linear
"""
from __future__ import annotations

import os

import numpy as np
import torch
from torch import nn

NORM_FIXTURES = ("normbn", "normln", "normgn")
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class _BNResBlock(nn.Module):
    """torchvision-style BasicBlock: conv-BN-ReLU(in place)-conv-BN, ``out += identity``, ReLU"""

    def __init__(self, c: int):
        super().__init__()
        self.conv1 = nn.Conv2d(c, c, 3, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(c)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(c, c, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(c)

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        out += identity
        return self.relu(out)


class _MeanOverPositions(nn.Module):
    """[B, T, D] -> [B, D]"""

    def forward(self, x):
        return x.mean(1)


def _stir(model: nn.Module) -> nn.Module:
    """non-trivial affine values (and running statistics) for every normalisation layer; all of them stay tracked"""
    for m in model.modules():
        if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d)):
            m.running_mean.normal_(0.0, 0.5)
            m.running_var.uniform_(0.5, 1.5)
        if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d, nn.LayerNorm, nn.GroupNorm)):
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0.0, 0.3)
    return model.eval()


def build_model(name: str) -> nn.Module:
    if name == "normbn":
        return _stir(nn.Sequential(nn.Conv2d(2, 4, 3, padding=1), _BNResBlock(4), nn.AdaptiveAvgPool2d(1), nn.Flatten(),
                                   nn.Linear(4, 3)))
    if name == "normln":
        return _stir(nn.Sequential(nn.Linear(5, 8), nn.LayerNorm(8), nn.Tanh(), _MeanOverPositions(), nn.Linear(8, 2)))
    if name == "normgn":
        return _stir(nn.Sequential(nn.Conv2d(2, 8, 3, padding=1), nn.GroupNorm(2, 8), nn.ReLU(), nn.AdaptiveAvgPool2d(1),
                                   nn.Flatten(), nn.Linear(8, 3)))
    raise KeyError(name)


def input_shape(name: str):
    return {"normbn": (2, 4, 4), "normln": (4, 5), "normgn": (2, 4, 4)}[name]


def n_outputs(name: str) -> int:
    return 2 if name == "normln" else 3


def make_fixture(name: str, dtype=torch.float64, batch: int = 10, seed: int = 711):
    """Fresh model + (X, y_cls, y_reg), as oracle/fixtures.py:make_fixture."""
    torch.manual_seed(seed)
    model = build_model(name).to(dtype)
    torch.manual_seed(seed)
    X = torch.randn(batch, *input_shape(name), dtype=dtype)
    C = n_outputs(name)
    y_cls = torch.randint(C, (batch,))
    y_reg = torch.randn(batch, C, dtype=dtype)
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
    sd = {k[2:]: torch.as_tensor(v) for k, v in g.items() if k.startswith("w.")}
    model.load_state_dict(sd)
    model = model.to(dtype).to(device).eval()
    X = torch.as_tensor(g["X"], dtype=dtype, device=device)
    y = torch.as_tensor(g["y"])
    y = y.to(device) if not y.is_floating_point() else y.to(dtype).to(device)
    return model, X, y


# ---- helpers shared by tests/test_norm_params.py (emulation) and tests/test_gpu_norm_params.py (device) ---------------
def rel(got, want) -> float:
    """``max|got - want| / max|want|``, the metric of tests/test_gpu_backend.py (recorded in the parity log)"""
    from tests.parity_log import record_error

    got = torch.as_tensor(got).detach().double().cpu()
    want = torch.as_tensor(want).detach().double().cpu()
    return record_error((got - want).abs().max().item() / (want.abs().max().item() + 1e-30))


def forbid_generic_route(monkeypatch):
    """``torch.func.jacrev`` / ``torch.func.grad`` raise: the two entry points through which the reference's generic route
    (laplace/curvature/curvature.py:115, 197) and laplace_amd/mirror.py (:64, :86) form Jacobians and per-sample gradients"""

    def refuse(*a, **kw):
        raise AssertionError("the generic torch.func route was taken")

    monkeypatch.setattr(torch.func, "jacrev", refuse)
    monkeypatch.setattr(torch.func, "grad", refuse)


def count_norm_calls(monkeypatch):
    """wrap the active kernel object's ``jac_norm_affine``; returns the list that receives one entry per call"""
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    inner, calls = K.jac_norm_affine, []

    def counted(*a, **kw):
        calls.append(1)
        return inner(*a, **kw)

    monkeypatch.setattr(K, "jac_norm_affine", counted, raising=False)
    return calls


def ef_gradients_from_golden(g: dict, likelihood: str):
    """per-sample gradients of the summed torch loss, ``[B, P]``, from the recorded ``Js`` and ``f`` (float64)"""
    Js, f, y = torch.as_tensor(g["Js"]), torch.as_tensor(g["f"]), torch.as_tensor(g["y"])
    if likelihood == "regression":
        df = 2.0 * (f - y)  # MSELoss(reduction="sum")
    else:
        df = torch.softmax(f, -1)
        df[torch.arange(len(y)), y] -= 1.0
    return torch.einsum("nc,ncp->np", df, Js)


def route_check(monkeypatch, dev: str):
    """With the generic route forbidden, every non-KFAC entry point of the three models runs on the kernels, and the norm
    kernel is called once per norm tap and backend call."""
    from torch.utils.data import DataLoader, TensorDataset

    from laplace_amd import HipEF, HipGGN
    from laplace_amd.laplace import HipLaplace

    forbid_generic_route(monkeypatch)
    calls = count_norm_calls(monkeypatch)
    for name in NORM_FIXTURES:
        for lik in ("classification", "regression"):
            g = load_golden(name, lik)
            model, X, y = golden_model(name, g, device=dev)
            b = HipGGN(model, lik)
            n_norm = len(b._tape().norm_taps)
            assert n_norm == {"normbn": 2, "normln": 1, "normgn": 1}[name]
            assert b._supported()
            seen = len(calls)
            for call in (lambda: b.jacobians(X), lambda: b.diag(X, y), lambda: b.full(X, y)):
                call()
                assert len(calls) == seen + n_norm, f"{name}: {len(calls) - seen} norm-kernel calls for {n_norm} taps"
                seen = len(calls)
            e = HipEF(model, lik)
            assert e._supported()
            for call in (lambda: e.gradients(X, y), lambda: e.diag(X, y), lambda: e.full(X, y)):
                call()
                assert len(calls) == seen + n_norm
                seen = len(calls)
            la = HipLaplace(model, lik, "all", "diag", prior_precision=0.7)
            la.fit(DataLoader(TensorDataset(X, y), batch_size=5))
            assert len(calls) == seen + 2 * n_norm  # (two minibatches)
            seen = len(calls)

            def no_jacobians(*a, **kw):
                raise AssertionError("the diagonal predictive fell back to backend.jacobians")

            monkeypatch.setattr(la.backend, "jacobians", no_jacobians)
            f_mu, f_var = la._glm_predictive_distribution(X)
            assert len(calls) == seen + n_norm
            assert torch.isfinite(f_var).all() and f_var.shape == (len(X), f_mu.shape[1], f_mu.shape[1])
