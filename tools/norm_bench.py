"""Cost of serving normalisation parameters on the device (dev tool; writes profiles/norm_bench.json).

  python tools/norm_bench.py [--out profiles/norm_bench.json]

Two records, no gates:
  * kernel: per distinct BatchNorm shape of the c4 network (ResNet-18 on 32 x 32, S = 9 seeds, B = 128) the time of
    `lk_jac_norm_affine_f32`, the bytes it must move (g once + xhat once + the block) and bytes/s, beside the time of the
    existing `lk_vjp_scale_mask_f32` pass over the SAME cotangent (it reads and writes it: twice the bytes), alternating in
    one process.  The cotangents rotate through enough buffers (>= 1 GiB in all) that the 256 MiB last-level cache cannot
    hold them from one launch to the next.
  * end to end: `HipGGN.diag` per minibatch of 128 on `ResNet18(freeze_bn=False)` against (a) `freeze_bn=True` on the same
    commit and (b) `use_norm_kernels = False`, the generic route, at the largest power-of-two batch that completes within
    60 s (scaled per sample).  One child process per leg, each under its own time limit; a failing leg ends the run.

Times are device events around synchronised work after a warm-up of every shape; no profiler.  `--rehearse` runs tiny shapes
on the CPU emulation to check the host logic and writes no times worth reading (the file says so).
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

C4_BN_SHAPES = [(64, 32), (128, 16), (256, 8), (512, 4)]  # (channels, height = width) of ResNet-18's BatchNorm outputs
LEG_TIMEOUT = {"kernel": 150, "unfrozen": 150, "frozen": 150, "generic": 240}


def _setup(rehearse: bool):
    import torch

    if rehearse:
        from laplace_amd import _lib
        from tests.emulated_norm_kernels import EmulatedNormKernels

        _lib.set_kernels_for_testing(EmulatedNormKernels())
        return torch, "cpu"
    if not torch.cuda.is_available():
        raise SystemExit("norm_bench: no ROCm device (a measurement does not fall back to the CPU)")
    return torch, "cuda"


class _Timer:
    """device events around the enclosed work (host clock around it on the rehearsal device)"""

    def __init__(self, torch, dev):
        self.torch, self.dev = torch, dev

    def __call__(self, fn, iters):
        torch = self.torch
        if self.dev == "cpu":
            t0 = time.perf_counter()
            for i in range(iters):
                fn(i)
            return (time.perf_counter() - t0) * 1e3 / iters
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters


def leg_kernel(args):
    torch, dev = _setup(args.rehearse)
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    timer = _Timer(torch, dev)
    S, B = (2, 2) if args.rehearse else (9, 128)
    rows = []
    for Ch, hw in C4_BN_SHAPES:
        L = hw * hw
        g_bytes = 4 * S * B * Ch * L
        nbuf = 1 if args.rehearse else max(2, min(32, -(-(1 << 30) // g_bytes)))
        gs = [torch.randn(S * B, Ch, hw, hw, device=dev) for _ in range(nbuf)]
        xs = [torch.randn(B, Ch, hw, hw, device=dev) for _ in range(nbuf)]
        scale = torch.rand(Ch, device=dev) + 0.5
        Jl = torch.zeros(B, S, 2 * Ch, device=dev)

        def norm(i):
            K.jac_norm_affine(gs[i % nbuf].view(S, B, Ch, hw, hw), xs[i % nbuf], Ch, 0, Jl, 0, Ch)

        def vjp(i):
            K.vjp_scale_mask(gs[i % nbuf], S, None, scale, L)

        iters = 2 if args.rehearse else max(2 * nbuf, 20)
        for fn in (norm, vjp):  # warm-up of both at this shape
            for i in range(nbuf):
                fn(i)
        t_norm, t_vjp = [], []
        for _ in range(1 if args.rehearse else 5):  # alternating rounds
            t_norm.append(timer(norm, iters))
            t_vjp.append(timer(vjp, iters))
        moved = g_bytes + 4 * B * Ch * L + 4 * B * S * 2 * Ch
        med_n, med_v = sorted(t_norm)[len(t_norm) // 2], sorted(t_vjp)[len(t_vjp) // 2]
        rows.append({
            "channels": Ch, "hw": hw, "S": S, "B": B, "cotangent_bytes": g_bytes, "buffers_rotated": nbuf,
            "norm_kernel_ms": med_n, "norm_kernel_ms_rounds": t_norm, "norm_kernel_bytes": moved,
            "norm_kernel_TBps": moved / (med_n * 1e-3) / 1e12,
            "vjp_scale_mask_ms": med_v, "vjp_scale_mask_ms_rounds": t_vjp, "vjp_scale_mask_bytes": 2 * g_bytes,
            "vjp_scale_mask_TBps": 2 * g_bytes / (med_v * 1e-3) / 1e12,
        })
        print(f"Ch={Ch:4d} {hw:2d}x{hw:<2d}: norm {med_n:8.4f} ms ({rows[-1]['norm_kernel_TBps']:.2f} TB/s)   "
              f"vjp_scale_mask {med_v:8.4f} ms ({rows[-1]['vjp_scale_mask_TBps']:.2f} TB/s)", flush=True)
        del gs, xs
    return {"shapes": rows}


def _resnet(torch, dev, freeze_bn):
    from torch import nn

    from laplace_amd.nets import ResNet18

    torch.manual_seed(0)
    model = ResNet18(freeze_bn=freeze_bn)
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0.0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    return model.to(dev).eval()


def leg_diag(args, freeze_bn):
    """`HipGGN.diag` per minibatch of 128 on the device route"""
    torch, dev = _setup(args.rehearse)
    from laplace_amd import HipGGN

    B = 2 if args.rehearse else 128
    model = _resnet(torch, dev, freeze_bn)
    b = HipGGN(model, "classification")
    X, y = torch.randn(B, 3, 32, 32, device=dev), torch.randint(10, (B,), device=dev)
    timer = _Timer(torch, dev)
    for _ in range(1 if args.rehearse else 3):
        b.diag(X, y)
    rounds = [timer(lambda i: b.diag(X, y), 1 if args.rehearse else 5) for _ in range(1 if args.rehearse else 3)]
    tape = b._tape()
    sweep = tape.sweeps.get(frozenset() if freeze_bn else frozenset({"norm"}))
    assert b._supported()
    return {"batch": B, "diag_ms": sorted(rounds)[len(rounds) // 2], "diag_ms_rounds": rounds,
            "ms_per_sample": sorted(rounds)[len(rounds) // 2] / B, "n_params": tape.n_params,
            "norm_taps": len(tape.norm_taps), "sweep": type(sweep).__name__,
            "split_ok": bool(getattr(sweep, "split_ok", False)), "split_reason": getattr(sweep, "split_reason", None)}


def leg_generic(args):
    """the route a model with tracked norm parameters took before (`use_norm_kernels = False`: the generic torch.func
    Jacobian), at growing power-of-two batches while a call stays within 60 s and its Jacobian within the free memory"""
    torch, dev = _setup(args.rehearse)
    from laplace_amd import HipGGN

    model = _resnet(torch, dev, False)
    b = HipGGN(model, "classification")
    b.use_norm_kernels = False
    assert not b._supported()
    P = sum(p.numel() for p in model.parameters() if p.requires_grad)
    runs, timer = [], _Timer(torch, dev)
    B = 1
    while B <= (2 if args.rehearse else 128):
        need = 3 * B * 10 * P * 4  # the [B, C, P] Jacobian, its per-parameter pieces before the concatenation, slack
        free = torch.cuda.mem_get_info()[0] if dev == "cuda" else 1 << 40
        if need > 0.8 * free:
            runs.append({"batch": B, "status": f"not run: about {need / 1e9:.0f} GB needed, {free / 1e9:.0f} GB free"})
            break
        X, y = torch.randn(B, 3, 32, 32, device=dev), torch.randint(10, (B,), device=dev)
        try:
            if B == 1:
                b.diag(X, y)  # warm-up (code objects, allocator) at the first size only: a call is seconds long
            ms = timer(lambda i: b.diag(X, y), 1)
        except torch.OutOfMemoryError as e:
            runs.append({"batch": B, "status": f"out of memory: {str(e)[:80]}"})
            break
        runs.append({"batch": B, "status": "ok", "diag_ms": ms, "ms_per_sample": ms / B})
        print(f"generic route, batch {B}: {ms:.1f} ms", flush=True)
        print("NORM_BENCH_PARTIAL " + json.dumps(runs[-1]), flush=True)
        if ms > 60e3:
            runs[-1]["status"] = "over 60 s"
            break
        if ms * 2 > 60e3:  # (the next size would not fit the window)
            break
        B *= 2
    ok = [r for r in runs if r["status"] == "ok"]
    return {"runs": runs, "largest_ok": ok[-1] if ok else None, "n_params": P}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "norm_bench.json"))
    ap.add_argument("--leg", choices=("kernel", "unfrozen", "frozen", "generic"))
    ap.add_argument("--legs", default="kernel,frozen,unfrozen,generic", help="legs to run (the others are kept from --base)")
    ap.add_argument("--base", help="result file of an earlier run whose other legs are kept")
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg:  # child: one leg, result as the last line of stdout
        res = {"kernel": leg_kernel, "unfrozen": lambda a: leg_diag(a, False), "frozen": lambda a: leg_diag(a, True),
               "generic": leg_generic}[args.leg](args)
        print("NORM_BENCH_RESULT " + json.dumps(res), flush=True)
        return
    result = {"tool": "tools/norm_bench.py", "rehearsal_on_cpu_emulation_times_meaningless": bool(args.rehearse),
              "hbm_copy_rate_guide_TBps": 6.29,
              "tapped_batchnorm_sweep": "NCHW seed-batched sweep (the split-fp16 NHWC sweep declares itself ineligible)"}
    if args.base:
        with open(args.base) as fh:
            result = {**json.load(fh), **result}
    failed = None
    for leg in [l for l in ("kernel", "frozen", "unfrozen", "generic") if l in args.legs.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg] + (["--rehearse"] if args.rehearse else [])
        t0 = time.time()
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT[leg], cwd=ROOT)
        except subprocess.TimeoutExpired as e:
            # what the leg had finished is kept (the generic route reports every batch size as it completes); the run ends here
            out = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
            sys.stdout.write(out)
            part = [json.loads(l[len("NORM_BENCH_PARTIAL "):]) for l in out.splitlines() if l.startswith("NORM_BENCH_PARTIAL ")]
            result[leg] = {"status": f"child process exceeded its limit of {LEG_TIMEOUT[leg]} s", "runs": part,
                           "largest_ok": part[-1] if part else None}
            failed = f"norm_bench: leg {leg} exceeded {LEG_TIMEOUT[leg]} s; stopping"
            break
        sys.stdout.write(proc.stdout)
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr[-4000:])
            raise SystemExit(f"norm_bench: leg {leg} ended with status {proc.returncode}; stopping")
        line = [l for l in proc.stdout.splitlines() if l.startswith("NORM_BENCH_RESULT ")][-1]
        result[leg] = json.loads(line[len("NORM_BENCH_RESULT "):])
        result[leg]["leg_wall_s"] = round(time.time() - t0, 1)
    fr, un, ge = result["frozen"], result["unfrozen"], result.get("generic", {}).get("largest_ok")
    result["summary"] = {
        "diag_ms_per_minibatch_128_frozen_bn": fr["diag_ms"], "diag_ms_per_minibatch_128_unfrozen_bn": un["diag_ms"],
        "norm_coverage_cost_ratio": un["diag_ms"] / fr["diag_ms"],
        "generic_route_largest_batch": ge and ge["batch"], "generic_route_ms_per_sample": ge and ge["ms_per_sample"],
        "device_route_ms_per_sample": un["ms_per_sample"],
        "gain_per_sample": ge and ge["ms_per_sample"] / un["ms_per_sample"],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result["summary"]))
    if failed:
        raise SystemExit(failed)


if __name__ == "__main__":
    main()
