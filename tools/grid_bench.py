"""Prior-precision grid search on one MI355X: the per-point loop (``gridsearch_prior_precision``) against the batched route
(``batched=True`` -> ``validation_loss_grid``, csrc/lk_grid.hip) in one process, on two shapes:

* c4: full-network Kron, ResNet-18 (CIFAR shape), validation 10 x 128, G = 100;
* c5: BERT-base (``BertConfig()``, random init, sequence 128) last-layer Kron, 512 validation points in batches of 32,
  G = 100; the backbone (one feature pass per batch) and the grid are timed apart.

Each leg: one warm-up of both routes, then wall clock up to a device synchronise.  Output check: both routes must install
the same prior precision, and the batched losses must equal the loop's at three grid points to 1e-5 relative.  Writes
``profiles/grid_bench.json`` (``--out``)."""
import argparse
import json
import os
import sys
import time

import torch
from torch.utils.data import DataLoader, TensorDataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from laplace_amd.laplace import HipLaplace  # noqa: E402
from laplace_amd.nets import ResNet18  # noqa: E402
from tests.test_prior_grid import loop_losses  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="c4,c5")
ap.add_argument("--grid", type=int, default=100)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_bench.json"))
ap.add_argument("--batched-only", action="store_true", help="one batched search per leg, no loop (for a kernel trace)")
args = ap.parse_args()
dev = "cuda"
G = args.grid


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def compare(la, val, res):
    """the installed prior precisions, and the losses of both routes at three grid points"""
    interval = torch.logspace(-4, 4, G)
    res["same_prior_precision"] = bool(res.pop("_pp_loop") == res.pop("_pp_batched"))
    pick = interval[[0, G // 2, G - 1]]
    got = la.validation_loss_grid(val, pick).cpu()
    want = loop_losses(la, val, pick)
    res["loss_rel_err_3pts"] = float(((got - want).abs() / want.abs()).max())
    res["outputs_equal"] = res["same_prior_precision"] and res["loss_rel_err_3pts"] < 1e-5


def run(la, val, res, n_batches):
    if args.batched_only:
        la.gridsearch_prior_precision(val, grid_size=G, batched=True)
        _, t_b = timed(lambda: la.gridsearch_prior_precision(val, grid_size=G, batched=True))
        res.update(batched_ms=t_b * 1e3, batched_ms_per_batch=t_b * 1e3 / n_batches)
        return
    la.gridsearch_prior_precision(val, grid_size=2)  # warm-up of both routes
    la.gridsearch_prior_precision(val, grid_size=2, batched=True)
    pp, t_loop = timed(lambda: la.gridsearch_prior_precision(val, grid_size=G).clone())
    res["_pp_loop"] = float(pp)
    pp, t_b = timed(lambda: la.gridsearch_prior_precision(val, grid_size=G, batched=True).clone())
    res["_pp_batched"] = float(pp)
    res.update(loop_ms=t_loop * 1e3, batched_ms=t_b * 1e3, speedup=t_loop / t_b,
               loop_ms_per_point_and_batch=t_loop * 1e3 / (G * n_batches), batched_ms_per_batch=t_b * 1e3 / n_batches)
    compare(la, val, res)


out = {"grid_points": G}
if "c4" in args.legs:
    torch.manual_seed(0)
    model = ResNet18(10).to(dev).eval()
    X, y = torch.randn(1280, 3, 32, 32, device=dev), torch.randint(10, (1280,), device=dev)
    val = DataLoader(TensorDataset(X, y), batch_size=128)
    la = HipLaplace(model, "classification", "all", "kron", prior_precision=1.0)
    la.fit(val)
    res = {"shape": "ResNet-18 full-network Kron, validation 10 x 128"}
    from laplace_amd import predictive as P

    post = la.posterior_precision
    P.glm_variance_kron(la.backend, X[:128], post)
    _, t1 = timed(lambda: [P.glm_variance_kron(la.backend, X[i:i + 128], post) for i in range(0, 1280, 128)])
    res["single_delta_predictive_ms_per_batch"] = t1 * 1e3 / 10
    run(la, val, res, 10)
    res["batched_over_single_pass"] = res["batched_ms_per_batch"] / res["single_delta_predictive_ms_per_batch"]
    if "loop_ms_per_point_and_batch" in res:
        res["loop_over_single_pass"] = res["loop_ms_per_point_and_batch"] / res["single_delta_predictive_ms_per_batch"]
    out["c4"] = res
    print(json.dumps({"c4": res}), flush=True)
    del la, model, X, y, val
    torch.cuda.empty_cache()

if "c5" in args.legs:
    from torch import nn
    from transformers import BertConfig, BertForSequenceClassification

    class BertHead(nn.Module):
        def __init__(self, cfg):
            super().__init__()
            self.hf = BertForSequenceClassification(cfg)

        def forward(self, data):
            return self.hf(input_ids=data["input_ids"], attention_mask=data["attention_mask"]).logits

    torch.manual_seed(711)
    cfg = BertConfig(num_labels=2)
    T, bs, n = 128, 32, 512
    model = BertHead(cfg).to(dev).eval()
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(cfg.vocab_size, (n, T), generator=g)
    mask = torch.ones(n, T, dtype=torch.long)
    lens = torch.randint(T // 2, T + 1, (n,), generator=g)
    mask[torch.arange(T)[None, :] >= lens[:, None]] = 0
    yv = torch.randint(2, (n,), generator=g)

    class Loader(list):
        dataset = range(n)

    val = Loader({"input_ids": ids[i:i + bs].to(dev), "attention_mask": mask[i:i + bs].to(dev),
                  "labels": yv[i:i + bs].to(dev)} for i in range(0, n, bs))
    la = HipLaplace(model, "classification", "last_layer", "kron", last_layer_name="hf.classifier", prior_precision=1.0)
    la.fit(val)
    res = {"shape": "BERT-base last-layer Kron, 512 validation points (16 x 32)"}
    run(la, val, res, len(val))
    _, t_bb = timed(lambda: [la.backend.cache_features(b) for b in val])
    res["backbone_ms"] = t_bb * 1e3
    res["batched_grid_ms"] = res["batched_ms"] - res["backbone_ms"]
    out["c5"] = res
    print(json.dumps({"c5": res}), flush=True)

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print(json.dumps(out))
