"""Cost of max pooling on the NHWC split-fp16 sweep (dev tool; writes profiles/pool_bench.json).

  python tools/pool_bench.py [--out profiles/pool_bench.json]

Two records:
  * kernel (no gate): the stem pool of `ResNet18(stem="imagenet")` on 64 x 64 inputs - MaxPool2d(3, 2, 1) on a 32 x 32 x 64 map -
    and the five MaxPool2d(2) stages of a VGG-11 on 32 x 32 inputs, S = 9 seeds, B = 128: the time of `lk_pool_vjp_nhwc_f32`, its
    minimal bytes 4 S B C (OH OW + H W) + B C OH OW and bytes/s, the path `lk_pool_variant` names, and the forward
    `lk_pool_fwd_nhwc_f32` (once per minibatch) - beside the stock pair the NCHW sweep runs on the same data:
    `F.max_pool2d(return_indices=True)` and `SeedBatchedSweep._maxpool_vjp` (a scatter_add_ through int64 indices expanded over
    the seeds), alternating in one process.  The cotangents rotate through enough buffers (>= 1 GiB in all) that the last-level
    cache cannot hold them from one launch to the next.
  * end to end (gate): `HipGGN.kron` per minibatch of 128 on `ResNet18(stem="imagenet")`, the default route against
    `SplitSweep.nhwc_pool = False` (the NCHW sweep: the route of this model before lk_pool.hip), medians of alternating rounds
    in one process.  GATE: the default is never slower.

One child process per leg, each under its own time limit; a failing leg ends the run.  Times are device events around
synchronised work after a warm-up; no profiler.  `--rehearse` runs tiny shapes on the CPU emulation to check the host logic and
writes no times worth reading (the file says so).
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

# (what, channels, height = width of the pool's input, window, stride, padding)
POOL_SHAPES = [("resnet18 imagenet stem", 64, 32, 3, 2, 1), ("vgg-11 stage 1", 64, 32, 2, 2, 0), ("vgg-11 stage 2", 128, 16, 2, 2, 0),
               ("vgg-11 stage 3", 256, 8, 2, 2, 0), ("vgg-11 stage 4", 512, 4, 2, 2, 0), ("vgg-11 stage 5", 512, 2, 2, 2, 0)]
LEGS = ("kernel", "resnet18_imagenet_stem")
LEG_TIMEOUT = {"kernel": 240, "resnet18_imagenet_stem": 240}


def _setup(rehearse: bool):
    import torch

    if rehearse:
        from laplace_amd import _lib
        from tests.emulated_pool_kernels import EmulatedPoolKernels

        _lib.set_kernels_for_testing(EmulatedPoolKernels())
        return torch, "cpu"
    if not torch.cuda.is_available():
        raise SystemExit("pool_bench: no ROCm device (a measurement does not fall back to the CPU)")
    return torch, "cuda"


def _median(v):
    return sorted(v)[len(v) // 2]


def leg_kernel(args):
    torch, dev = _setup(args.rehearse)
    import torch.nn.functional as F

    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep import SeedBatchedSweep

    K = get_kernels()
    timer = _Timer(torch, dev)
    S, B = (2, 2) if args.rehearse else (9, 128)
    rows = []
    for what, C, hw, k, s, p in POOL_SHAPES:
        ohw = (hw + 2 * p - k) // s + 1
        g_bytes, dx_bytes, arg_bytes = 4 * S * B * C * ohw * ohw, 4 * S * B * C * hw * hw, B * C * ohw * ohw
        nbuf = 1 if args.rehearse else max(2, min(32, -(-(1 << 30) // (g_bytes + dx_bytes))))
        xs = [torch.relu(torch.randn(B, hw, hw, C, device=dev)) for _ in range(nbuf)]  # (post-ReLU, as in both networks)
        gs = [torch.randn(S * B, ohw, ohw, C, device=dev) for _ in range(nbuf)]
        args_ = [K.pool_forward(x, K.POOL_MAX, k, s, p)[1] for x in xs]
        # the NCHW sweep's operands: the same values, channels first
        xs_c = [x.permute(0, 3, 1, 2).contiguous() for x in xs]
        gs_c = [g.permute(0, 3, 1, 2).contiguous() for g in gs]
        idx = [F.max_pool2d(x, k, s, p, return_indices=True)[1] for x in xs_c]
        in_shape = (B, C, hw, hw)

        def ours(i):
            K.pool_vjp(gs[i % nbuf], args_[i % nbuf], S, (hw, hw), K.POOL_MAX, k, s, p)

        def stock(i):
            SeedBatchedSweep._maxpool_vjp(gs_c[i % nbuf], idx[i % nbuf], in_shape, S, B)

        def fwd(i):
            K.pool_forward(xs[i % nbuf], K.POOL_MAX, k, s, p)

        def stock_fwd(i):
            F.max_pool2d(xs_c[i % nbuf], k, s, p, return_indices=True)

        if not args.rehearse:  # the two VJPs agree on this data (a selection or a short sum: 1e-6 of the largest element)
            a = K.pool_vjp(gs[0], args_[0], S, (hw, hw), K.POOL_MAX, k, s, p).permute(0, 3, 1, 2)
            b_ = SeedBatchedSweep._maxpool_vjp(gs_c[0], idx[0], in_shape, S, B)
            assert float((a - b_).abs().max()) <= 1e-6 * float(b_.abs().max()), what
            del a, b_
        iters = 2 if args.rehearse else max(2 * nbuf, 20)
        for fn in (ours, stock, fwd, stock_fwd):
            for i in range(nbuf):
                fn(i)
        t = {"ours": [], "stock": [], "fwd": [], "stock_fwd": []}
        for _ in range(1 if args.rehearse else 5):  # alternating rounds
            for name, fn in (("ours", ours), ("stock", stock), ("fwd", fwd), ("stock_fwd", stock_fwd)):
                t[name].append(timer(fn, iters))
        moved = g_bytes + dx_bytes + arg_bytes
        fwd_bytes = 4 * B * C * (hw * hw + ohw * ohw) + arg_bytes
        med = {n: _median(v) for n, v in t.items()}
        rows.append({
            "what": what, "channels": C, "hw": hw, "window": k, "stride": s, "padding": p, "S": S, "B": B,
            "buffers_rotated": nbuf, "variant": K.pool_variant(K.POOL_MAX, S, B, hw, hw, C, k, s, p, True),
            "pool_vjp_ms": med["ours"], "pool_vjp_ms_rounds": t["ours"], "pool_vjp_min_bytes": moved,
            "pool_vjp_TBps": moved / (med["ours"] * 1e-3) / 1e12,
            "stock_maxpool_vjp_ms": med["stock"], "stock_maxpool_vjp_ms_rounds": t["stock"],
            "pool_fwd_ms": med["fwd"], "pool_fwd_ms_rounds": t["fwd"], "pool_fwd_min_bytes": fwd_bytes,
            "pool_fwd_TBps": fwd_bytes / (med["fwd"] * 1e-3) / 1e12,
            "stock_max_pool2d_indices_ms": med["stock_fwd"], "stock_max_pool2d_indices_ms_rounds": t["stock_fwd"],
        })
        print(f"{what:24s} C={C:3d} {hw:2d}x{hw:<2d}: pool_vjp {med['ours']:8.4f} ms ({rows[-1]['pool_vjp_TBps']:.2f} TB/s of its "
              f"minimal bytes)   stock scatter {med['stock']:8.4f} ms   pool_fwd {med['fwd']:8.4f} ms "
              f"({rows[-1]['pool_fwd_TBps']:.2f} TB/s)   stock forward {med['stock_fwd']:8.4f} ms", flush=True)
        del xs, gs, args_, xs_c, gs_c, idx
    return {"shapes": rows}


def leg_kron(args, net):
    """`HipGGN.kron` per minibatch of 128: the default route and `nhwc_pool = False`, alternating rounds in this process"""
    torch, dev = _setup(args.rehearse)
    from laplace_amd import HipGGN
    from laplace_amd.nets import ResNet18
    from laplace_amd.sweep_nhwc import SplitSweep

    torch.manual_seed(0)
    B = 2 if args.rehearse else 128
    hw = 64
    model = ResNet18(stem="imagenet").to(dev).eval()
    X, y = torch.randn(B, 3, hw, hw, device=dev), torch.randint(10, (B,), device=dev)
    backends = {}
    for route, flag in (("default", True), ("nhwc_pool_false", False)):  # (the switch is read when a backend builds its sweep)
        SplitSweep.nhwc_pool = flag
        try:
            b = backends[route] = HipGGN(model, "classification")
            for _ in range(1 if args.rehearse else 3):
                b.kron(X, y, N=B)
        finally:
            SplitSweep.nhwc_pool = True
    timer = _Timer(torch, dev)
    rounds = {route: [] for route in backends}
    for _ in range(1 if args.rehearse else 5):  # alternating rounds
        for route, b in backends.items():
            rounds[route].append(timer(lambda i, b=b: b.kron(X, y, N=B), 1 if args.rehearse else 5))
    out = {"network": net, "input_hw": hw, "batch": B}
    for route, b in backends.items():
        sweep = getattr(b._tape(), "sweep", None)
        assert sweep not in (None, False), getattr(b._tape(), "sweep_reason", None)
        out[route] = {"kron_ms": _median(rounds[route]), "kron_ms_rounds": rounds[route], "sweep": type(sweep).__name__,
                      "split_ok": bool(getattr(sweep, "split_ok", False)), "split_reason": getattr(sweep, "split_reason", None)}
    if not args.rehearse:
        assert out["default"]["split_ok"] and not out["nhwc_pool_false"]["split_ok"], out
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_bench.json"))
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg:  # child: one leg, result as the last line of stdout
        res = leg_kernel(args) if args.leg == "kernel" else leg_kron(args, args.leg)
        print("POOL_BENCH_RESULT " + json.dumps(res), flush=True)
        return
    result = {"tool": "tools/pool_bench.py", "rehearsal_on_cpu_emulation_times_meaningless": bool(args.rehearse)}
    for leg in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg] + (["--rehearse"] if args.rehearse else [])
        t0 = time.time()
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT[leg], cwd=ROOT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"pool_bench: leg {leg} exceeded {LEG_TIMEOUT[leg]} s; stopping")
        sys.stdout.write(proc.stdout)
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr[-4000:])
            raise SystemExit(f"pool_bench: leg {leg} ended with status {proc.returncode}; stopping")
        line = [l for l in proc.stdout.splitlines() if l.startswith("POOL_BENCH_RESULT ")][-1]
        result[leg] = json.loads(line[len("POOL_BENCH_RESULT "):])
        result[leg]["leg_wall_s"] = round(time.time() - t0, 1)
    summary = {}
    for net in LEGS[1:]:
        d, n = result[net]["default"]["kron_ms"], result[net]["nhwc_pool_false"]["kron_ms"]
        summary[net] = {"kron_ms_per_minibatch_128_default": d, "kron_ms_per_minibatch_128_nhwc_pool_false": n, "gain": n / d,
                        "default_not_slower": bool(d <= n)}
    summary["gate_default_never_slower"] = all(summary[net]["default_not_slower"] for net in LEGS[1:])
    result["summary"] = summary
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(summary))
    if not args.rehearse and not summary["gate_default_never_slower"]:
        raise SystemExit("pool_bench: GATE FAILED: the NHWC pooling route is slower than the NCHW sweep")


if __name__ == "__main__":
    main()
