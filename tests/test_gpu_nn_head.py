"""The sampled-heads kernel of the `nn` predictive (csrc/lk_nnhead.hip) against plain fp64: softmax(phi W_s^T + b_s).mean(0), the
mean and unbiased variance over the draws, and the samples.  Bounds per element, from the fp64 quantities (u = 2^-24):
  logits     E[s, b] = (D + 2) u max_c (sum_d |phi| |W_s| + |b_s|)
  probs      mean_s p64[s, b, c] (2 E[s, b] + (16 + S) u) + 2^-40        (one draw's softmax: the same with S = 1)
  mean       mean_s E + (S + 2) u mean_s |f64|
  variance   4 (S + 4) u var64 + 4 max_s |f64 - mean64| mean_s E + 2 max_s E^2
The variance bound is derived: logits off by e_s, |e_s| <= E_s, move sum_s (f_s - mean)^2 / (S - 1) by at most
2 S / (S - 1) max_s |f_s - mean| mean_s E + S / (S - 1) max_s E^2 (S / (S - 1) <= 2), and accumulating the S squares in fp32 costs
a relative (S + 4) u, doubled for slack.  Inputs keep E <= 2^-10.  The CPU test holds torch's own fp32 evaluation to every bound on
every case, so each is known to be reachable.  profiles/nn_head_instances.md has every case as measured on an MI355X."""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV, U = "cuda", 2.0 ** -24
# (C, D, B, S, bias, ld - P, special row, the variant the shape must take)
CASES = [
    (1, 1, 1, 1, True, 0, None, dict(regime=0, tiles=1, rows=64, groups=1)),            # S == 1: NaN variance
    (2, 3, 63, 2, False, 0, None, dict(regime=0, tiles=1)),                              # one below a row tile, scalar loads
    (10, 64, 65, 7, True, 3, "shift", dict(regime=0, tiles=1)),                          # one above; ld > P breaks the alignment
    (33, 513, 5, 100, True, 0, None, dict(regime=0, tiles=4, restaged=True)),            # 3 -> 4 tiles, K-chunk remainder
    (64, 64, 130, 7, True, 0, "saturated", dict(regime=0, tiles=4, restaged=False)),     # 16-byte loads
    (2, 3, 32705, 7, True, 0, None, dict(regime=0, groups=4)),                           # 2 + 2 + 2 + 1 draws over four waves
    (65, 64, 17, 7, True, 0, "shift", dict(regime=1, tiles=2, rows=64)),
    (65, 1, 32768, 2, False, 0, None, dict(regime=1, groups=1)),                         # two draws in ONE group, one launch
    (257, 3, 33, 2, False, 0, None, dict(regime=1, tiles=8, rows=32)),                   # one above a 32-row tile
    (1024, 64, 17, 7, True, 0, None, dict(regime=1, tiles=16, rows=16, groups=7)),       # LK_NN_HEAD_MAX_C, one above a tile
    (1024, 3, 1377, 7, True, 0, None, dict(regime=1, groups=4)),                         # 2 + 2 + 2 + 1 draws, Chan's update
    (1024, 513, 15, 2, True, 4, None, dict(regime=1, restaged=False)),            # one below; ld > P, aligned
]


@functools.lru_cache(maxsize=None)
def make_case(C, D, B, S, bias, pad, special):
    """(phi, theta) in fp32 and the fp64 logits f [S, B, C] and E [S, B]; the padding of theta is NaN (never read)"""
    g = torch.Generator().manual_seed(131 * C + D)
    P = C * D + (C if bias else 0)
    phi, theta = torch.randn(B, D, generator=g), torch.full((S, P + pad), float("nan"))
    W = (torch.randn(C, D, generator=g) + 0.3 * torch.randn(S, C, D, generator=g)) / D ** 0.5
    if special == "shift":  # every logit of one row moves by 80: the softmax must subtract its maximum
        phi[B // 2, 0], W[:, :, 0] = 80.0, 1.0
    if special == "saturated":
        phi[B // 2] *= 25.0
    theta[:, :C * D] = W.reshape(S, -1)
    if bias:
        theta[:, C * D:P] = torch.randn(S, C, generator=g)
    return phi, theta, *reference(phi, theta, C, bias)


def reference(phi, theta, C, bias):
    D, p64, t64 = phi.shape[1], phi.double().cpu(), theta.double().cpu()
    W = t64[:, :C * D].reshape(-1, C, D)
    b = t64[:, C * D:C * D + C] if bias else torch.zeros(len(W), C, dtype=torch.float64)
    f = torch.einsum("bd,scd->sbc", p64, W) + b[:, None]
    E = (D + 2) * U * (torch.einsum("bd,scd->sbc", p64.abs(), W.abs()) + b.abs()[:, None]).amax(2)
    return f, E


def bounds(f, E):
    """kind -> (fp64 value, bound per element)"""
    S, p, Em, E3 = f.shape[0], f.softmax(-1), E.mean(0)[:, None], E[..., None]
    dev, var = (f - f.mean(0)).abs().amax(0), f.var(0) if S > 1 else f[0] * float("nan")
    return {"probs": (p.mean(0), (p * (2 * E3 + (16 + S) * U)).mean(0) + 2.0 ** -40),
            "mean": (f.mean(0), Em + (S + 2) * U * f.abs().mean(0)),
            "var": (var, 4 * (S + 4) * U * var + 4 * dev * Em + 2 * E.amax(0)[:, None] ** 2),
            "logits": (f, E3.expand_as(f)),
            "softmax": (p, p * (2 * E3 + 17 * U) + 2.0 ** -40)}


def check(got, f, E, what):
    """every kind of `got` within its bound; S == 1: the variance is NaN as torch's"""
    ref = bounds(f, E)
    for kind, x in got.items():
        want, tol = ref[kind]
        if kind == "var" and f.shape[0] == 1:
            assert torch.isnan(x).all(), f"{what}: the variance of one draw must be NaN"
            continue
        ratio = ((x.double().cpu() - want).abs() / tol).max().item()
        print(f"| {what} | {kind} | {ratio:.3f} |")
        assert ratio <= 1.0, f"{what}, {kind}: worst error {ratio:.3f} of its bound"


def run_kernel(phi, theta, C, bias):
    from laplace_amd._lib import get_kernels

    K, out, (S, B) = get_kernels(), {}, (theta.shape[0], phi.shape[0])
    p, t = phi.to(DEV), theta.to(DEV)
    bufs = {k: torch.full((n * B * C + 128,), float("nan"), device=DEV) for k, n in dict(probs=1, mean=1, var=1, logits=S, softmax=S).items()}
    bufs = {k: (buf, buf[64:-64].view((S, B, C) if k in ("logits", "softmax") else (B, C))) for k, buf in bufs.items()}  # NaN guard bands
    K.nn_head(p, t, C, bias, "probs", out=bufs["probs"][1])
    K.nn_head(p, t, C, bias, "moments", out=bufs["mean"][1], out2=bufs["var"][1])
    K.nn_head(p, t, C, bias, "samples", out=bufs["logits"][1])
    K.nn_head(p, t, C, bias, "samples", softmax=True, out=bufs["softmax"][1])
    for k, (buf, view) in bufs.items():
        assert torch.isnan(buf[:64]).all() and torch.isnan(buf[-64:]).all(), f"a write outside {k}"
        out[k] = view.clone()
    return out


@pytest.mark.parametrize("C,D,B,S,bias,pad,special,variant", CASES, ids=lambda v: str(v) if not isinstance(v, dict) else "")
def test_torch_fp32_meets_the_bounds(C, D, B, S, bias, pad, special, variant):
    phi, theta, f, E = make_case(C, D, B, S, bias, pad, special)
    assert E.max() <= 2.0 ** -10
    W = theta[:, :C * D].reshape(S, C, D)
    f32 = torch.baddbmm(theta[:, None, C * D:C * D + C] if bias else torch.zeros(S, 1, C), phi.expand(S, B, D), W.transpose(1, 2))
    p32 = f32.softmax(-1)
    check({"probs": p32.mean(0), "mean": f32.mean(0), "var": f32.var(0) if S > 1 else f32[0] * float("nan"), "logits": f32, "softmax": p32}, f, E, "torch fp32")


@pytest.mark.gpu
@pytest.mark.parametrize("C,D,B,S,bias,pad,special,variant", CASES, ids=lambda v: str(v) if not isinstance(v, dict) else "")
def test_nn_head_against_fp64(C, D, B, S, bias, pad, special, variant):
    from laplace_amd._lib import get_kernels

    got = get_kernels().nn_head_variant(B, C, D, S)
    assert {k: got[k] for k in variant} == variant, got
    phi, theta, f, E = make_case(C, D, B, S, bias, pad, special)
    out = run_kernel(phi, theta, C, bias)
    check(out, f, E, f"{C} {D} {B} {S} {int(bias)} {pad} {special}")
    again = run_kernel(phi, theta, C, bias)
    assert all(torch.equal(out[k].view(torch.int32), again[k].view(torch.int32)) for k in out), "two equal calls differ"


def small_model(likelihood):
    from torch import nn

    torch.manual_seed(7)
    C = 5 if likelihood == "classification" else 2
    model = nn.Sequential(nn.Conv2d(2, 3, 3), nn.Tanh(), nn.Flatten(), nn.Linear(3 * 4 * 4, C)).to(DEV).eval()
    X = torch.randn(9, 2, 6, 6, device=DEV)
    return model, X, torch.randint(C, (9,), device=DEV) if likelihood == "classification" else torch.randn(9, C, device=DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("likelihood", ["classification", "regression"])
@pytest.mark.parametrize("structure", ["kron", "diag", "full"])
def test_the_predictive_with_the_kernel_on_and_off(structure, likelihood):
    """switch on and off (the cached-feature loop) on the same seeded generator: both within the bounds of the fp64 value of the
    same draws, and no parameter of the model changes"""
    from torch.utils.data import DataLoader, TensorDataset

    from laplace_amd.laplace import HipLaplace

    model, X, y = small_model(likelihood)
    la = HipLaplace(model, likelihood, "last_layer", structure, prior_precision=2.0)
    la.fit(DataLoader(TensorDataset(X, y), batch_size=9))
    before = [p.detach().clone() for p in model.parameters()]
    gen = lambda: torch.Generator(DEV).manual_seed(11)  # noqa: E731
    f, E = reference(la.backend.cache_features(X).phi, la.sample(13, gen()), la.n_outputs, True)
    for on in (True, False):
        la.use_nn_head_kernels = on
        out = la(X, pred_type="nn", link_approx="mc", n_samples=13, generator=gen())
        got = {"mean": out[0], "var": out[1]} if likelihood == "regression" else {"probs": out}
        got["logits" if likelihood == "regression" else "softmax"] = la.predictive_samples(X, pred_type="nn", n_samples=13, generator=gen())
        got["logits"] = la.functional_samples(X, pred_type="nn", n_samples=13, generator=gen())
        check(got, f, E, f"{structure} {likelihood} kernel {on}")
        assert all(torch.equal(a, b) for a, b in zip(before, model.parameters())), "a parameter of the model changed"
