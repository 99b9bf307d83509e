"""Cost of KFAC-reduce on the device (dev tool; writes profiles/kfac_reduce_bench.json).

  python tools/kfac_reduce_bench.py [--out profiles/kfac_reduce_bench.json]

Two records, after tools/conv1d_bench.py:
  * kernel (no gate): `lk_possum_f16x2` / `lk_possum_f32` and `lk_patch_mean_f32` beside the torch sequences they replace, with
    the achieved TB/s of their minimal bytes (the input once plus the rows written): the G rows of the first stage of
    `nets.ResNet18()` (S = 9 seeds, B = 128: 1152 split NHWC maps of 32 x 32 x 64 against `g.float().sum((1, 2))`), the sequence
    rows of `nets.ViTSmall()` (128 x 64 rows of 192 against `.mean(1)`), and the A rows of its 3x3 stride-1 and stride-2
    convolutions on [128, 64, 32, 32] maps in both memory orders (against `F.unfold(...).mean(2)`).  The buffers rotate so that
    the last-level cache cannot hold them from one launch to the next.
  * end to end (gate): `HipGGN.kron(..., kfac_approx="reduce")` per minibatch of 128 on `nets.ResNet18()` and `nets.ViTSmall()`
    with `use_kfac_reduce_kernels` on and off (off is the torch arithmetic the fit ran before these kernels), and `expand` beside
    both; medians of alternating rounds of synchronised wall-clock time, the spread (max - min of the rounds) reported.
    GATE: with the switch on no network is slower than with it off beyond the spread; the switch's default follows it.

One child process per leg, each under its own time limit; a failing leg ends the run.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.norm_bench import _Timer  # noqa: E402  (device events around the enclosed work)

LEGS = ("kernel", "resnet18", "vit")
LEG_TIMEOUT = {"kernel": 240, "resnet18": 300, "vit": 300}
ROUTES = ("reduce_kernels_on", "reduce_kernels_off", "expand")


def _torch():
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("kfac_reduce_bench: no ROCm device (a measurement does not fall back to the CPU)")
    return torch


def _median(v):
    return sorted(v)[len(v) // 2]


def _race(torch, what, legs, nbuf, moved, extra):
    """medians of five alternating rounds of `ours` and `stock` over rotated buffers"""
    timer = _Timer(torch, "cuda")
    iters = max(2 * nbuf, 20)
    for fn in legs.values():
        for i in range(nbuf):
            fn(i)
    t = {n: [] for n in legs}
    for _ in range(5):
        for name, fn in legs.items():
            t[name].append(timer(fn, iters))
    med = {n: _median(v) for n, v in t.items()}
    row = {"what": what, "buffers_rotated": nbuf, "min_bytes": moved, "kernel_ms": med["ours"], "kernel_ms_rounds": t["ours"],
           "kernel_TBps_of_min_bytes": moved / (med["ours"] * 1e-3) / 1e12, "torch_ms": med["stock"], "torch_ms_rounds": t["stock"],
           "torch_over_kernel": med["stock"] / med["ours"], **extra}
    print(f"{what}: kernel {med['ours']:8.4f} ms ({row['kernel_TBps_of_min_bytes']:.2f} TB/s of its minimal bytes)   "
          f"torch {med['stock']:8.4f} ms", flush=True)
    return row


def leg_kernel(args):
    torch = _torch()
    import torch.nn.functional as F

    from laplace_amd._lib import SplitTensor, get_kernels

    K, rows = get_kernels(), []
    # ---- position sums -----------------------------------------------------------------------------------------------------
    R, H, D = 9 * 128, 32, 64
    moved = 4 * R * H * H * D + 4 * R * D  # (two fp16 planes: four bytes an element)
    nbuf = max(2, min(8, -(-(1 << 30) // moved)))
    sexp = torch.tensor([3], dtype=torch.int32, device="cuda")
    gs = []
    for _ in range(nbuf):
        g = torch.randn(R, H, H, D, device="cuda") * 8
        hi = g.half()
        gs.append(SplitTensor(torch.stack([hi, (g - hi.float()).half()]), sexp))
        del g, hi
    a, b = K.possum(gs[0], R, H * H, D, 0), gs[0].float().sum((1, 2))
    assert torch.allclose(a, b, rtol=1e-4, atol=1e-3), "possum (planes) differs from torch"
    rows.append(_race(torch, "G rows, ResNet18 stage 1: 1152 split NHWC maps of 32 x 32 x 64", {
        "ours": lambda i: K.possum(gs[i % nbuf], R, H * H, D, 0), "stock": lambda i: gs[i % nbuf].float().sum((1, 2))}, nbuf, moved,
        {"variant": K.possum_variant(R, H * H, D, 0), "torch": "g.float().sum((1, 2))"}))
    del gs
    R, L, D = 128, 64, 192
    moved = 4 * R * L * D + 4 * R * D
    nbuf = 8
    xs = [torch.randn(R, L, D, device="cuda") for _ in range(nbuf)]
    assert torch.allclose(K.possum(xs[0], R, L, D, 0, 1.0 / L), xs[0].mean(1), rtol=1e-4, atol=1e-5)
    rows.append(_race(torch, "A rows, ViTSmall: 128 sequences of 64 x 192", {
        "ours": lambda i: K.possum(xs[i % nbuf], R, L, D, 0, 1.0 / L), "stock": lambda i: xs[i % nbuf].mean(1).contiguous()}, nbuf, moved,
        {"variant": K.possum_variant(R, L, D, 0), "torch": "a.mean(1).contiguous()"}))
    del xs
    # ---- patch means -------------------------------------------------------------------------------------------------------
    B, C, H = 128, 64, 32
    for stride in (1, 2):
        for cl in (True, False):
            geo = ((3, 3), (stride, stride), (1, 1), (1, 1))
            moved = 4 * B * C * H * H + 4 * B * 9 * C
            nbuf = 8
            xs = [torch.randn(B, C, H, H, device="cuda") for _ in range(nbuf)]
            if cl:
                xs = [x.contiguous(memory_format=torch.channels_last) for x in xs]

            def stock(i, geo=geo, xs=xs):
                cols = F.unfold(xs[i % nbuf], geo[0], dilation=geo[3], padding=geo[2], stride=geo[1])
                cols = cols.reshape(B, C, 9, -1).transpose(1, 2).reshape(cols.shape)  # (the accumulator's native column order)
                return cols.mean(2).contiguous()

            assert torch.allclose(K.patch_mean(xs[0], *geo), stock(0), rtol=1e-4, atol=1e-5), "patch_mean differs from torch"
            rows.append(_race(torch, f"A rows, 3x3 stride {stride} on [128, 64, 32, 32] {'NHWC' if cl else 'NCHW'}", {
                "ours": lambda i, geo=geo, xs=xs: K.patch_mean(xs[i % nbuf], *geo), "stock": stock}, nbuf, moved,
                {"variant": K.patch_mean_variant((B, C, H, H), cl, *geo), "torch": "F.unfold(a, ...) [native order] .mean(2)"}))
            del xs
    return {"shapes": rows}


def leg_kron(args, net):
    """`HipGGN.kron` per minibatch of 128 on the routes of `net`, alternating rounds in this process"""
    torch = _torch()
    from laplace_amd import HipGGN
    from laplace_amd import nets

    torch.manual_seed(0)
    B = 128
    model, name = (nets.ResNet18(), "ResNet18()") if net == "resnet18" else (nets.ViTSmall(), "ViTSmall()")
    model = model.to("cuda").eval()
    X, y = torch.randn(B, 3, 32, 32, device="cuda"), torch.randint(10, (B,), device="cuda")
    backends = {}
    for route in ROUTES:
        b = backends[route] = HipGGN(model, "classification")
        b.use_kfac_reduce_kernels = route != "reduce_kernels_off"
        b.bench_kwargs = {} if route == "expand" else {"kfac_approx": "reduce"}
        for _ in range(3):
            b.kron(X, y, N=B, **b.bench_kwargs)[1].kfacs

    def timed(b, iters=4):  # (wall clock around synchronised work: the factor kernels run on side streams)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            b.kron(X, y, N=B, **b.bench_kwargs)[1].kfacs
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    rounds = {route: [] for route in backends}
    for _ in range(5):  # alternating rounds
        for route, b in backends.items():
            rounds[route].append(timed(b))
    out = {"network": name, "batch": B}
    for route, b in backends.items():
        kinds = sorted(set(getattr(b, "reduce_route", {}).values()))
        out[route] = {"kron_ms": _median(rounds[route]), "kron_ms_rounds": rounds[route],
                      "kron_ms_spread": max(rounds[route]) - min(rounds[route]), "sweep": type(b._tape().sweep).__name__,
                      "reduce_route_values": kinds, "reduce_route_taps": len(getattr(b, "reduce_route", {}))}
    assert out["reduce_kernels_on"]["reduce_route_values"] == ["kernel"], out
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kfac_reduce_bench.json"))
    ap.add_argument("--leg", choices=LEGS)
    args = ap.parse_args()
    if args.leg:  # child: one leg, result as the last line of stdout
        res = leg_kernel(args) if args.leg == "kernel" else leg_kron(args, args.leg)
        print("KFAC_REDUCE_BENCH_RESULT " + json.dumps(res), flush=True)
        return
    result = {"tool": "tools/kfac_reduce_bench.py"}
    for leg in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg]
        t0 = time.time()
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT[leg], cwd=ROOT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"kfac_reduce_bench: leg {leg} exceeded {LEG_TIMEOUT[leg]} s; stopping")
        sys.stdout.write(proc.stdout)
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr[-4000:])
            raise SystemExit(f"kfac_reduce_bench: leg {leg} ended with status {proc.returncode}; stopping")
        line = [l for l in proc.stdout.splitlines() if l.startswith("KFAC_REDUCE_BENCH_RESULT ")][-1]
        result[leg] = json.loads(line[len("KFAC_REDUCE_BENCH_RESULT "):])
        result[leg]["leg_wall_s"] = round(time.time() - t0, 1)
    nets = LEGS[1:]
    ms = {net: {route: result[net][route]["kron_ms"] for route in ROUTES} for net in nets}
    spread = {net: max(result[net][route]["kron_ms_spread"] for route in ROUTES[:2]) for net in nets}
    summary = {"kron_ms_per_minibatch_128": ms, "kron_ms_spread_of_the_reduce_routes": spread,
               **{f"{net}_kernels_off_over_on": ms[net]["reduce_kernels_off"] / ms[net]["reduce_kernels_on"] for net in nets},
               **{f"{net}_expand_over_reduce_kernels_on": ms[net]["expand"] / ms[net]["reduce_kernels_on"] for net in nets},
               "gate_kernels_on_not_slower_than_off_beyond_the_spread": bool(all(
                   ms[net]["reduce_kernels_on"] <= ms[net]["reduce_kernels_off"] + spread[net] for net in nets))}
    result["summary"] = summary
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(summary))
    if not summary["gate_kernels_on_not_slower_than_off_beyond_the_spread"]:
        raise SystemExit("kfac_reduce_bench: GATE FAILED: use_kfac_reduce_kernels = True is slower than False (the switch belongs off by default)")


if __name__ == "__main__":
    main()
