"""Diagonal-output predictive (csrc/lk_quaddiag.hip) against the routes it replaces, at C = 100 outputs — writes
profiles/diag_output_bench.json.

Kernel lines (B = 128): `lk_kron_quaddiag_shared_f32` against what `predictive._shared_quadform` does on the same operands
(190 launches of the pair-sum kernel on gathered 10-output blocks, scattered into [B, C, C]) at ResNet-18's 64 x 576 layer
(L = 1024) and its 512 x 4608 layer (L = 16).  Model line: `la(X, diagonal_output=True)` of a Kron Laplace on
nets.ResNet18(num_classes=100) with `predictive.use_diag_output_kernels` on and off.

Method: every line is warmed up, then timed in alternating rounds (on, off, on, off, ...) between device synchronisations,
the operands rotating through two buffers so that a round does not find the previous round's tensors in cache; reported are
the median and the spread (max - min) of the rounds.  Gate: `on` is slower than `off` on no line beyond the larger spread."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from laplace_amd import nets, predictive as P  # noqa: E402
from laplace_amd._lib import get_kernels  # noqa: E402
from laplace_amd.laplace import HipLaplace  # noqa: E402

DEV = "cuda"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def alternate(on, off, rounds):
    """ms of `on(r)` and `off(r)` in alternating rounds after one warm-up of each per buffer; r is the round (the buffer)"""
    for r in range(2):
        on(r), off(r)
    t_on, t_off = [], []
    for r in range(rounds):
        t_on.append(timed(lambda: on(r))[0])
        t_off.append(timed(lambda: off(r))[0])
    line = {w: {"median_ms": statistics.median(t), "spread_ms": max(t) - min(t), "rounds_ms": t}
            for w, t in (("on", t_on), ("off", t_off))}
    spread = max(line["on"]["spread_ms"], line["off"]["spread_ms"])
    line["speedup"] = line["off"]["median_ms"] / line["on"]["median_ms"]
    line["on_not_slower"] = line["on"]["median_ms"] <= line["off"]["median_ms"] + spread
    return line


def agreement(a, b):
    """worst |a - b| / (1e-4 |b| + 1e-6 max_sample |b|): the project's element criterion"""
    a, b = a.double(), b.double()
    return ((a - b).abs() / (1e-4 * b.abs() + 1e-6 * b.abs().amax(-1, keepdim=True)).clamp_min(1e-300)).max().item()


def kernel_line(K, name, B, C, Do, Dk, L, rounds):
    g = torch.Generator(device=DEV).manual_seed(Do + L)
    us = [torch.randn(B, C, Do, L, device=DEV, generator=g) * 1e-2 for _ in range(2)]
    vs = [torch.randn(B, Dk, L, device=DEV, generator=g).relu_() for _ in range(2)]
    l1, l2 = torch.rand(Do, device=DEV, generator=g) + 0.1, torch.rand(Dk, device=DEV, generator=g) + 0.1
    d = torch.full((1,), 0.7, device=DEV)

    def on(r):
        return K.kron_quaddiag_shared(us[r % 2], vs[r % 2], l1, l2, d, torch.zeros(B, C, device=DEV))

    def off(r):
        fvar = torch.zeros(B, C, C, device=DEV)
        P._shared_quadform(K, lambda uu, vv, out: K.kron_quadform_shared(uu, vv, l1, l2, d, out), us[r % 2], vs[r % 2], fvar,
                           weight_sharing_only=True)
        return torch.diagonal(fvar, dim1=1, dim2=2)

    line = alternate(on, off, rounds)
    line.update(name=name, B=B, C=C, Do=Do, Dk=Dk, L=L, variant=K.quaddiag_variant(K.QD_KRON, B, C, Do, Dk, L),
                on_tflops=2.0 * B * C * Do * Dk * L / line["on"]["median_ms"] / 1e9, agreement=agreement(on(0), off(0)))
    return line


def model_line(B, rounds):
    torch.manual_seed(0)
    model = nets.ResNet18(num_classes=100).to(DEV).eval()
    Xf, yf = torch.randn(128, 3, 32, 32, device=DEV), torch.randint(100, (128,), device=DEV)

    class Loader(list):
        dataset = list(range(128))

    la = HipLaplace(model, "classification", "all", "kron", prior_precision=1.0)
    la.fit(Loader([(Xf[:64], yf[:64]), (Xf[64:], yf[64:])]))
    Xs = [torch.randn(B, 3, 32, 32, device=DEV) for _ in range(2)]

    def call(r, switch):
        P.use_diag_output_kernels = switch
        try:
            return la(Xs[r % 2], diagonal_output=True)
        finally:
            P.use_diag_output_kernels = True

    line = alternate(lambda r: call(r, True), lambda r: call(r, False), rounds)
    P.use_diag_output_kernels = True
    var_on = la._glm_predictive_distribution(Xs[0], diagonal_output=True)[1]
    P.use_diag_output_kernels = False
    var_off = la._glm_predictive_distribution(Xs[0], diagonal_output=True)[1]
    P.use_diag_output_kernels = True
    line.update(name="la(X, diagonal_output=True), ResNet18(num_classes=100), kron", B=B, C=100,
                agreement=agreement(var_on, var_off))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--model-batch", type=int, default=32,
                    help="predictive batch of the model line (the off route materialises [B, C, Do*Dk] blocks: 120 GB at 128)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_output_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the device: a timing taken elsewhere says nothing"
    K = get_kernels()
    lines = [kernel_line(K, "ResNet-18 layer1 conv (64 x 576, L = 1024)", 128, 100, 64, 576, 1024, a.rounds),
             kernel_line(K, "ResNet-18 layer4 conv (512 x 4608, L = 16)", 128, 100, 512, 4608, 16, a.rounds)]
    off_out_of_memory = []  # predictive batches at which the off route's [B, C, Do*Dk] blocks did not fit the device
    for mb in (a.model_batch, a.model_batch // 4, a.model_batch // 16):
        try:
            lines.append(model_line(mb, a.rounds))
            break
        except torch.OutOfMemoryError:
            off_out_of_memory.append(mb)
            P.use_diag_output_kernels = True
            torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "lines": lines,
           "model_line_off_route_out_of_memory_at_batch": off_out_of_memory,
           "gate_on_slower_on_no_line": all(ln["on_not_slower"] for ln in lines)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    for ln in lines:
        print(f"{ln['name']}: on {ln['on']['median_ms']:.3f} ms (spread {ln['on']['spread_ms']:.3f}), off "
              f"{ln['off']['median_ms']:.3f} ms (spread {ln['off']['spread_ms']:.3f}), x{ln['speedup']:.1f}, "
              f"agreement {ln['agreement']:.3g}", flush=True)
    print("gate:", res["gate_on_slower_on_no_line"])


if __name__ == "__main__":
    main()
