"""Cost of serving grouped / depthwise convolution weights on the device (dev tool; writes profiles/gconv_bench.json).

  python tools/gconv_bench.py [--out profiles/gconv_bench.json]

  * kernel: S = 9 seeds, B = 128, depthwise 3x3 / padding 1 at the (channels, map, stride) shapes of a MobileNetV2 on 32 x 32
    inputs, and one 7x7 / padding 3 shape.  Per shape the time of `lk_jac_gconv_f32`, the bytes it must move
    (4 * (S*B*Do*L + B*Cin*H*W + B*S*Do*Dkg)) and bytes/s, beside the time of the only way the library could form the same
    block without it: `lk_jac_conv_f32` on the input viewed as [B*groups, Cig, H, W] and the cotangent as
    [S, B*groups, Do/groups, L], in chunks under its B*Cc <= 65535 limit, plus the permute into place.  Both alternate in
    one process; the buffers rotate through at least 1 GiB so that the 256 MiB last-level cache cannot hold them from one
    launch to the next.
    THE ONE GATE: at every shape the new kernel is not slower than that baseline (no margin).  The fraction of the HBM rate
    is written down, not gated.
  * end to end: `HipGGN.diag` per minibatch of 128 on `nets.MobileNetV2Small` against the generic `torch.func` route
    (`use_gconv_kernels = False`) at the largest power-of-two batch that completes within 60 s, scaled per sample.

One child process per leg, each under its own time limit; a failing leg ends the run.  Times are device events around
synchronised work after a warm-up of every shape; no profiler.  `--rehearse` runs tiny shapes on the CPU emulation to check
the host logic and writes no times worth reading (the file says so).
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

# (channels, height = width, stride, kernel, padding)
DW_SHAPES = [(32, 32, 1, 3, 1), (96, 32, 2, 3, 1), (144, 16, 1, 3, 1), (192, 16, 2, 3, 1), (384, 8, 1, 3, 1), (576, 8, 2, 3, 1),
             (960, 4, 1, 3, 1), (96, 16, 1, 7, 3)]
LEG_TIMEOUT = {"kernel": 300, "device": 150, "generic": 300}
HBM_TBPS = 6.29  # the copy rate the measuring guide gives for the device


def _setup(rehearse: bool):
    import torch

    if rehearse:
        from laplace_amd import _lib
        from tests.emulated_gconv_kernels import EmulatedGConvKernels

        _lib.set_kernels_for_testing(EmulatedGConvKernels())
        return torch, "cpu"
    if not torch.cuda.is_available():
        raise SystemExit("gconv_bench: no ROCm device (a measurement does not fall back to the CPU)")
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


def regrouped_jac_conv(K, x, g, k, stride, pad, groups, Jl):
    """the block of a grouped convolution from `lk_jac_conv_f32` alone: every (sample, group) pair becomes a sample of a
    dense convolution with Cig input and Do / groups output channels; `Jl [B, S, Do * Dkg]` (no bias columns)"""
    import torch

    B, Cin, H, W = x.shape
    S, _, Do, OH, OW = g.shape
    Cig, Dog = Cin // groups, Do // groups
    Dkg = Cig * k * k
    xv = x.view(B * groups, Cig, H, W)
    gv = g.view(S, B * groups, Dog, OH, OW)
    tmp = torch.empty(B * groups, S, Dog * Dkg, dtype=torch.float32, device=x.device)
    step = 65535 // S
    for r0 in range(0, B * groups, step):
        r1 = min(r0 + step, B * groups)
        K.jac_conv(xv[r0:r1], gv[:, r0:r1].contiguous(), (k, k), stride, pad, 1, tmp[r0:r1], 0, -1)
    Jl.copy_(tmp.view(B, groups, S, Dog * Dkg).permute(0, 2, 1, 3).reshape(B, S, Do * Dkg))


def leg_kernel(args):
    torch, dev = _setup(args.rehearse)
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    timer = _Timer(torch, dev)
    S, B = (2, 2) if args.rehearse else (9, 128)
    rows = []
    for C, hw, stride, k, pad in DW_SHAPES:
        if args.rehearse:
            C = min(C, 8)
        oh = (hw + 2 * pad - k) // stride + 1
        L, Dkg = oh * oh, k * k
        g_bytes = 4 * S * B * C * L
        moved = g_bytes + 4 * B * C * hw * hw + 4 * B * S * C * Dkg
        nbuf = 1 if args.rehearse else max(2, min(32, -(-(1 << 30) // (g_bytes + 4 * B * C * hw * hw))))
        gs = [torch.randn(S, B, C, oh, oh, device=dev) for _ in range(nbuf)]
        xs = [torch.randn(B, C, hw, hw, device=dev) for _ in range(nbuf)]
        Jl = torch.zeros(B, S, C * Dkg, device=dev)
        Jb = torch.zeros(B, S, C * Dkg, device=dev)

        def new(i):
            K.jac_gconv(xs[i % nbuf], gs[i % nbuf], k, stride, pad, 1, C, Jl, 0, -1)

        def base(i):
            regrouped_jac_conv(K, xs[i % nbuf], gs[i % nbuf], k, stride, pad, C, Jb)

        new(0), base(0)
        if dev == "cuda":
            torch.cuda.synchronize()
        agree = float((Jl - Jb).abs().max() / Jb.abs().max())
        for fn in (new, base):  # warm-up of both at this shape
            for i in range(nbuf):
                fn(i)
        it_new, it_base = (2, 1) if args.rehearse else (max(2 * nbuf, 20), max(nbuf, 4))
        t_new, t_base = [], []
        for _ in range(1 if args.rehearse else 5):  # alternating rounds
            t_new.append(timer(new, it_new))
            t_base.append(timer(base, it_base))
        med_n, med_b = sorted(t_new)[len(t_new) // 2], sorted(t_base)[len(t_base) // 2]
        rows.append({
            "channels": C, "hw": hw, "stride": stride, "kernel": k, "padding": pad, "S": S, "B": B, "L": L,
            "cotangent_bytes": g_bytes, "buffers_rotated": nbuf, "bytes_that_must_move": moved,
            "gconv_ms": med_n, "gconv_ms_rounds": t_new, "gconv_TBps": moved / (med_n * 1e-3) / 1e12,
            "gconv_fraction_of_hbm_rate": moved / (med_n * 1e-3) / 1e12 / HBM_TBPS,
            "regrouped_jac_conv_ms": med_b, "regrouped_jac_conv_ms_rounds": t_base, "speedup": med_b / med_n,
            "max_normalised_difference": agree, "gate_not_slower": bool(med_n <= med_b),
        })
        print(f"C={C:4d} {hw:2d}x{hw:<2d} s{stride} k{k}: gconv {med_n:8.4f} ms ({rows[-1]['gconv_TBps']:.2f} TB/s, "
              f"{100 * rows[-1]['gconv_fraction_of_hbm_rate']:.0f} % of HBM)   regrouped jac_conv {med_b:9.4f} ms   "
              f"x{med_b / med_n:.1f}   diff {agree:.1e}", flush=True)
        del gs, xs
    return {"shapes": rows, "gate_met_at_every_shape": all(r["gate_not_slower"] for r in rows)}


def _mobilenet(torch, dev, rehearse):
    from torch import nn

    from laplace_amd.nets import MobileNetV2Small

    torch.manual_seed(0)
    model = MobileNetV2Small(width=0.25 if rehearse else 1.0)
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0.0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    return model.to(dev).eval()


def leg_device(args):
    """`HipGGN.diag` per minibatch of 128 on the device route"""
    torch, dev = _setup(args.rehearse)
    from laplace_amd import HipGGN

    B = 2 if args.rehearse else 128
    hw = 16 if args.rehearse else 32
    b = HipGGN(_mobilenet(torch, dev, args.rehearse), "classification")
    X, y = torch.randn(B, 3, hw, hw, device=dev), torch.randint(10, (B,), device=dev)
    timer = _Timer(torch, dev)
    assert b._supported()
    for _ in range(1 if args.rehearse else 3):
        b.diag(X, y)
    rounds = [timer(lambda i: b.diag(X, y), 1 if args.rehearse else 5) for _ in range(1 if args.rehearse else 3)]
    tape = b._tape()
    sweep = tape.sweeps.get(frozenset({"gconv", "norm"}))
    return {"batch": B, "diag_ms": sorted(rounds)[len(rounds) // 2], "diag_ms_rounds": rounds,
            "ms_per_sample": sorted(rounds)[len(rounds) // 2] / B, "n_params": tape.n_params,
            "grouped_taps": len(tape.gconv_taps), "norm_taps": len(tape.norm_taps), "sweep": type(sweep).__name__,
            "sweep_reason": getattr(tape, "sweep_reason", None)}


def leg_generic(args):
    """the route such a model takes without the kernel (`use_gconv_kernels = False`: the generic torch.func Jacobian), at
    growing power-of-two batches while a call stays within 60 s and its Jacobian within the free memory"""
    torch, dev = _setup(args.rehearse)
    from laplace_amd import HipGGN

    model = _mobilenet(torch, dev, args.rehearse)
    b = HipGGN(model, "classification")
    b.use_gconv_kernels = False
    assert not b._supported()
    P = sum(p.numel() for p in model.parameters() if p.requires_grad)
    hw = 16 if args.rehearse else 32
    runs, timer = [], _Timer(torch, dev)
    B = 1
    while B <= (2 if args.rehearse else 128):
        need = 3 * B * 10 * P * 4  # the [B, C, P] Jacobian, its per-parameter pieces before the concatenation, slack
        free = torch.cuda.mem_get_info()[0] if dev == "cuda" else 1 << 40
        if need > 0.8 * free:
            runs.append({"batch": B, "status": f"not run: about {need / 1e9:.0f} GB needed, {free / 1e9:.0f} GB free"})
            break
        X, y = torch.randn(B, 3, hw, hw, device=dev), torch.randint(10, (B,), device=dev)
        try:
            if B == 1:
                b.diag(X, y)  # warm-up (code objects, allocator) at the first size only: a call is seconds long
            ms = timer(lambda i: b.diag(X, y), 1)
        except torch.OutOfMemoryError as e:
            runs.append({"batch": B, "status": f"out of memory: {str(e)[:80]}"})
            break
        runs.append({"batch": B, "status": "ok", "diag_ms": ms, "ms_per_sample": ms / B})
        print(f"generic route, batch {B}: {ms:.1f} ms", flush=True)
        print("GCONV_BENCH_PARTIAL " + json.dumps(runs[-1]), flush=True)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gconv_bench.json"))
    ap.add_argument("--leg", choices=("kernel", "device", "generic"))
    ap.add_argument("--legs", default="kernel,device,generic", help="legs to run (the others are kept from --base)")
    ap.add_argument("--base", help="result file of an earlier run whose other legs are kept")
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg:  # child: one leg, result as the last line of stdout
        res = {"kernel": leg_kernel, "device": leg_device, "generic": leg_generic}[args.leg](args)
        print("GCONV_BENCH_RESULT " + json.dumps(res), flush=True)
        return
    result = {"tool": "tools/gconv_bench.py", "rehearsal_on_cpu_emulation_times_meaningless": bool(args.rehearse),
              "hbm_copy_rate_guide_TBps": HBM_TBPS}
    if args.base:
        with open(args.base) as fh:
            result = {**json.load(fh), **result}
    failed = None
    for leg in [l for l in ("kernel", "device", "generic") if l in args.legs.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg] + (["--rehearse"] if args.rehearse else [])
        t0 = time.time()
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT[leg], cwd=ROOT)
        except subprocess.TimeoutExpired as e:
            # what the leg had finished is kept (the generic route reports every batch size as it completes); the run ends here
            out = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
            sys.stdout.write(out)
            part = [json.loads(l[len("GCONV_BENCH_PARTIAL "):]) for l in out.splitlines() if l.startswith("GCONV_BENCH_PARTIAL ")]
            result[leg] = {"status": f"child process exceeded its limit of {LEG_TIMEOUT[leg]} s", "runs": part,
                           "largest_ok": part[-1] if part else None}
            failed = f"gconv_bench: leg {leg} exceeded {LEG_TIMEOUT[leg]} s; stopping"
            break
        sys.stdout.write(proc.stdout)
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr[-4000:])
            raise SystemExit(f"gconv_bench: leg {leg} ended with status {proc.returncode}; stopping")
        line = [l for l in proc.stdout.splitlines() if l.startswith("GCONV_BENCH_RESULT ")][-1]
        result[leg] = json.loads(line[len("GCONV_BENCH_RESULT "):])
        result[leg]["leg_wall_s"] = round(time.time() - t0, 1)
    de, ge = result.get("device"), (result.get("generic") or {}).get("largest_ok")
    kern = result.get("kernel", {})
    result["summary"] = {
        "gate_kernel_not_slower_than_regrouped_jac_conv_at_every_shape": kern.get("gate_met_at_every_shape"),
        "smallest_speedup": min((r["speedup"] for r in kern.get("shapes", [])), default=None),
        "best_fraction_of_hbm_rate": max((r["gconv_fraction_of_hbm_rate"] for r in kern.get("shapes", [])), default=None),
        "device_route_diag_ms_per_minibatch_128": de and de["diag_ms"],
        "device_route_ms_per_sample": de and de["ms_per_sample"],
        "generic_route_largest_batch": ge and ge["batch"], "generic_route_ms_per_sample": ge and ge["ms_per_sample"],
        "gain_per_sample": de and ge and ge["ms_per_sample"] / de["ms_per_sample"],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result["summary"]))
    if failed:
        raise SystemExit(failed)
    if kern and not kern.get("gate_met_at_every_shape") and not args.rehearse:
        raise SystemExit("gconv_bench: the kernel is slower than the regrouped lk_jac_conv_f32 at some shape (see the file)")


if __name__ == "__main__":
    main()
