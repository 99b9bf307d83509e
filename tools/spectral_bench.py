#!/usr/bin/env python
"""What the spectral route of ``HipFullLaplace`` costs and saves, measured (device events, alternating rounds, medians and
spreads) at the last-layer shapes of BASELINE c3 (D = 512, C = 10, P = 5 130, B = 512) and c5 (D = 768, C = 2, B = 32):

  (a) the predictive per batch: ``lk_spectral_quadform_ll_f32`` against ``lk_dense_quadform_ll_f32``
  (b) one change of the prior precision: nothing (the O(P) weights) against ``cholesky`` + ``cholesky_inverse``
  (c) a 100-point grid search over 10 validation batches: one batched pass against the per-point loop
  (d) 100 marginal-likelihood Adam steps on either route
  (e) the one-off ``lk_syevj_f32``

Writes ``profiles/spectral_bench.json`` with the gates (a) not slower beyond the spread of the rounds, (c) and (d) faster than the
Cholesky route.  The switch stays opt-in whatever the gates say.

    python tools/spectral_bench.py [--shapes c3,c5] [--rounds 5] [--out profiles/spectral_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn
from torch.utils.data import DataLoader, TensorDataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {"c3": dict(D=512, C=10, B=512, d_in=64), "c5": dict(D=768, C=2, B=32, d_in=64)}


def timed(fn, inner=1):
    """milliseconds of ``inner`` calls between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def alternate(a, b, rounds, inner=1):
    """``rounds`` alternating measurements of the two callables after one warm-up each -> summary dict"""
    a(), b()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(a, inner))
        tb.append(timed(b, inner))
    out = {}
    for tag, t in (("spectral", ta), ("cholesky", tb)):
        out[tag] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}
    out["ratio_cholesky_over_spectral"] = out["cholesky"]["median_ms"] / max(out["spectral"]["median_ms"], 1e-9)
    return out


def build(shape, spectral):
    from laplace_amd.laplace import HipLaplace

    torch.manual_seed(0)
    D, C, B, d_in = shape["D"], shape["C"], shape["B"], shape["d_in"]
    model = nn.Sequential(nn.Linear(d_in, D), nn.ReLU(), nn.Linear(D, C)).cuda()
    X = torch.randn(4 * B, d_in, device="cuda")
    y = torch.randint(C, (4 * B,), device="cuda")
    la = HipLaplace(model, "classification", "last_layer", "full", last_layer_name="2", spectral=spectral)
    la.fit(DataLoader(TensorDataset(X, y), batch_size=B))
    Xv, yv = torch.randn(10 * B, d_in, device="cuda"), torch.randint(C, (10 * B,), device="cuda")
    return la, X[:B], DataLoader(TensorDataset(Xv, yv), batch_size=B)  # ten validation batches


def bench_shape(name, shape, rounds):
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    res = {"shape": {k: v for k, v in shape.items() if k != "d_in"}}
    ls, Xb, val = build(shape, True)
    lc, _, _ = build(shape, False)
    P = ls.n_params
    res["shape"]["P"] = P
    print(f"[{name}] P = {P}", flush=True)
    # (e) the one-off decomposition
    H = ls.H.detach().contiguous()
    res["e_syevj_ms"] = [timed(lambda: K.syevj(H, clamp=True)) for _ in range(2)]
    print(f"[{name}] (e) syevj {res['e_syevj_ms']}", flush=True)
    lam, Q = ls.spectrum
    # (a) the predictive kernels on one batch of features
    phi = torch.randn(shape["B"], shape["D"], device="cuda")
    delta = torch.ones(1, device="cuda")
    Sigma = lc.posterior_covariance.contiguous()
    res["a_predictive"] = alternate(lambda: K.spectral_quadform_ll(phi, Q, lam, 1.0, delta, shape["C"], True),
                                    lambda: K.dense_quadform_ll(phi, Sigma, shape["C"], True), rounds, inner=5)
    print(f"[{name}] (a) {res['a_predictive']}", flush=True)

    # (b) one change of the prior precision
    def prior_spectral():
        ls.prior_precision = 0.5
        ls._mu()

    def prior_cholesky():
        lc.prior_precision = 0.5
        lc.posterior_covariance

    res["b_prior_change"] = alternate(prior_spectral, prior_cholesky, rounds)
    print(f"[{name}] (b) {res['b_prior_change']}", flush=True)
    # (c) the 100-point grid search over 10 validation batches
    res["c_grid_100"] = alternate(lambda: ls.gridsearch_prior_precision(val, grid_size=100, batched=True),
                                  lambda: lc.gridsearch_prior_precision(val, grid_size=100), rounds)
    print(f"[{name}] (c) {res['c_grid_100']}", flush=True)
    # (d) 100 marginal-likelihood Adam steps
    res["d_marglik_100"] = alternate(lambda: ls.optimize_prior_precision(method="marglik", n_steps=100, prior_structure="scalar"),
                                     lambda: lc.optimize_prior_precision(method="marglik", n_steps=100, prior_structure="scalar"),
                                     rounds)
    print(f"[{name}] (d) {res['d_marglik_100']}", flush=True)
    a = res["a_predictive"]
    res["gates"] = {
        "a_not_slower_beyond_spread": a["spectral"]["median_ms"] <= a["cholesky"]["median_ms"]
        + (a["cholesky"]["max_ms"] - a["cholesky"]["min_ms"]) + (a["spectral"]["max_ms"] - a["spectral"]["min_ms"]),
        "c_faster_than_loop": res["c_grid_100"]["ratio_cholesky_over_spectral"] > 1.0,
        "d_faster_than_cholesky_route": res["d_marglik_100"]["ratio_cholesky_over_spectral"] > 1.0,
    }
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c3,c5")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "spectral_bench needs a ROCm device"
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "method": "device events, alternating rounds, medians"}
    if os.path.exists(args.out):
        try:
            out.update({k: v for k, v in json.load(open(args.out)).items() if k in SHAPES})
        except ValueError:
            pass
    for name in args.shapes.split(","):
        out[name] = bench_shape(name, SHAPES[name], args.rounds)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
            fh.write("\n")
    print(json.dumps({k: out[k]["gates"] for k in SHAPES if k in out}))


if __name__ == "__main__":
    main()
