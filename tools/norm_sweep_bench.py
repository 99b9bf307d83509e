"""Cost of sweeping GroupNorm models in one seed-batched pass (dev tool; writes profiles/norm_sweep_bench.json).

  python tools/norm_sweep_bench.py [--out profiles/norm_sweep_bench.json]

Two records:
  * kernel (no gate): per GroupNorm shape of `ResNet18(norm="gn")` on 32 x 32 - (C, H) in {(64, 32), (128, 16), (256, 8),
    (512, 4)}, GroupNorm(32, C), S = 9 seeds, B = 128 - and per layout the time of `lk_norm_vjp_f32`, its minimal bytes (g read
    once, dx written once, xhat once) and bytes/s, beside `lk_vjp_scale_mask_f32` on the SAME cotangent (it reads and writes
    it), and the forward `lk_norm_fwd_f32` (once per minibatch; x read once, y and xhat written), alternating in one process.  The cotangents rotate through enough buffers (>= 1 GiB in all) that the last-level cache
    cannot hold them from one launch to the next.  `lk_norm_sweep_variant` names the path each shape takes.
  * end to end: `HipGGN.kron` per minibatch of 128 on `ResNet18(norm="gn")` on the split sweep (the default), on the NCHW
    sweep (`use_split_sweep = False`) and on the autograd tape (`use_sweep = False`: one stock reverse pass per seed, the route
    this model took before the sweeps had a rule for GroupNorm).  GATE: the default is never slower than the tape.

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

GN_SHAPES = [(64, 32), (128, 16), (256, 8), (512, 4)]  # (channels, height = width) of the GroupNorm outputs of ResNet18(norm="gn")
GROUPS = 32
LEGS = ("kernel", "split", "nchw", "tape")
LEG_TIMEOUT = {"kernel": 200, "split": 150, "nchw": 150, "tape": 200}


def _setup(rehearse: bool):
    import torch

    if rehearse:
        from laplace_amd import _lib
        from tests.emulated_normvjp_kernels import EmulatedNormVjpKernels

        _lib.set_kernels_for_testing(EmulatedNormVjpKernels())
        return torch, "cpu"
    if not torch.cuda.is_available():
        raise SystemExit("norm_sweep_bench: no ROCm device (a measurement does not fall back to the CPU)")
    return torch, "cuda"


def leg_kernel(args):
    torch, dev = _setup(args.rehearse)
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    timer = _Timer(torch, dev)
    S, B = (2, 2) if args.rehearse else (9, 128)
    rows = []
    for Ch, hw in GN_SHAPES:
        L = hw * hw
        g_bytes = 4 * S * B * Ch * L
        nbuf = 1 if args.rehearse else max(2, min(32, -(-(1 << 30) // g_bytes)))
        w = torch.rand(Ch, device=dev) + 0.5
        for layout in (0, 1):
            shape = (Ch, hw, hw) if layout == 0 else (hw, hw, Ch)
            gs = [torch.randn(S * B, *shape, device=dev) for _ in range(nbuf)]
            ins = [torch.randn(B, *shape, device=dev) for _ in range(nbuf)]
            xs = [K.norm_forward(x, w, None, GROUPS, layout, 1e-5)[1:] for x in ins]

            def norm(i):
                xhat, rstd = xs[i % nbuf]
                K.norm_vjp(gs[i % nbuf], xhat, rstd, w, S, GROUPS, layout)

            def vjp(i):  # (the per-channel scale of an eval-mode BatchNorm; on the NHWC copy the channel index is only nominal)
                K.vjp_scale_mask(gs[i % nbuf], S, None, w, L)

            def fwd(i):  # (once per minibatch, not per seed; a lane group per row in both layouts - see DESIGN.md)
                K.norm_forward(ins[i % nbuf], w, None, GROUPS, layout, 1e-5)

            iters = 2 if args.rehearse else max(2 * nbuf, 20)
            for fn in (norm, vjp, fwd):  # warm-up of all three at this shape
                for i in range(nbuf):
                    fn(i)
            t_norm, t_vjp, t_fwd = [], [], []
            for _ in range(1 if args.rehearse else 5):  # alternating rounds
                t_norm.append(timer(norm, iters))
                t_vjp.append(timer(vjp, iters))
                t_fwd.append(timer(fwd, iters))
            moved = 2 * g_bytes + 4 * B * Ch * L
            med_n, med_v = sorted(t_norm)[len(t_norm) // 2], sorted(t_vjp)[len(t_vjp) // 2]
            med_f, fwd_bytes = sorted(t_fwd)[len(t_fwd) // 2], 3 * 4 * B * Ch * L  # (x read once; y and xhat written)
            rows.append({
                "channels": Ch, "hw": hw, "groups": GROUPS, "layout": layout, "S": S, "B": B, "cotangent_bytes": g_bytes,
                "buffers_rotated": nbuf, "variant": K.norm_sweep_variant(S, B, L, Ch, GROUPS, layout, True),
                "norm_vjp_ms": med_n, "norm_vjp_ms_rounds": t_norm, "norm_vjp_min_bytes": moved,
                "norm_vjp_TBps": moved / (med_n * 1e-3) / 1e12,
                "vjp_scale_mask_ms": med_v, "vjp_scale_mask_ms_rounds": t_vjp, "vjp_scale_mask_bytes": 2 * g_bytes,
                "vjp_scale_mask_TBps": 2 * g_bytes / (med_v * 1e-3) / 1e12,
                "norm_fwd_ms": med_f, "norm_fwd_ms_rounds": t_fwd, "norm_fwd_min_bytes": fwd_bytes,
                "norm_fwd_TBps": fwd_bytes / (med_f * 1e-3) / 1e12,
            })
            print(f"Ch={Ch:4d} {hw:2d}x{hw:<2d} layout {layout}: norm_vjp {med_n:8.4f} ms ({rows[-1]['norm_vjp_TBps']:.2f} TB/s)   "
                  f"vjp_scale_mask {med_v:8.4f} ms ({rows[-1]['vjp_scale_mask_TBps']:.2f} TB/s)   "
                  f"norm_fwd {med_f:8.4f} ms ({rows[-1]['norm_fwd_TBps']:.2f} TB/s)", flush=True)
            del gs, xs, ins
    return {"shapes": rows}


def leg_kron(args, route):
    """`HipGGN.kron` per minibatch of 128 on ResNet18(norm="gn"), frozen affine"""
    torch, dev = _setup(args.rehearse)
    from laplace_amd import HipGGN
    from laplace_amd.nets import ResNet18

    torch.manual_seed(0)
    B = 2 if args.rehearse else 128
    model = ResNet18(norm="gn").to(dev).eval()
    b = HipGGN(model, "classification")
    if route == "tape":
        b.use_sweep = False
    elif route == "nchw":
        b.use_split_sweep = False
    X, y = torch.randn(B, 3, 32, 32, device=dev), torch.randint(10, (B,), device=dev)
    timer = _Timer(torch, dev)
    for _ in range(1 if args.rehearse else 3):
        b.kron(X, y, N=B)
    rounds = [timer(lambda i: b.kron(X, y, N=B), 1 if args.rehearse else 5) for _ in range(1 if args.rehearse else 3)]
    sweep = getattr(b._tape(), "sweep", None)
    if route != "tape":
        assert sweep not in (None, False), getattr(b._tape(), "sweep_reason", None)
    return {"route": route, "batch": B, "kron_ms": sorted(rounds)[len(rounds) // 2], "kron_ms_rounds": rounds,
            "sweep": type(sweep).__name__ if sweep not in (None, False) else None,
            "split_ok": bool(getattr(sweep, "split_ok", False)), "split_reason": getattr(sweep, "split_reason", None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "norm_sweep_bench.json"))
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg:  # child: one leg, result as the last line of stdout
        res = leg_kernel(args) if args.leg == "kernel" else leg_kron(args, args.leg)
        print("NORM_SWEEP_BENCH_RESULT " + json.dumps(res), flush=True)
        return
    result = {"tool": "tools/norm_sweep_bench.py", "rehearsal_on_cpu_emulation_times_meaningless": bool(args.rehearse)}
    for leg in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg] + (["--rehearse"] if args.rehearse else [])
        t0 = time.time()
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT[leg], cwd=ROOT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"norm_sweep_bench: leg {leg} exceeded {LEG_TIMEOUT[leg]} s; stopping")
        sys.stdout.write(proc.stdout)
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr[-4000:])
            raise SystemExit(f"norm_sweep_bench: leg {leg} ended with status {proc.returncode}; stopping")
        line = [l for l in proc.stdout.splitlines() if l.startswith("NORM_SWEEP_BENCH_RESULT ")][-1]
        result[leg] = json.loads(line[len("NORM_SWEEP_BENCH_RESULT "):])
        result[leg]["leg_wall_s"] = round(time.time() - t0, 1)
    sp, nc, tp = result["split"]["kron_ms"], result["nchw"]["kron_ms"], result["tape"]["kron_ms"]
    result["summary"] = {"kron_ms_per_minibatch_128_split_sweep": sp, "kron_ms_per_minibatch_128_nchw_sweep": nc,
                         "kron_ms_per_minibatch_128_autograd_tape": tp, "gain_over_tape": tp / sp,
                         "gate_default_not_slower_than_tape": bool(sp <= tp)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result["summary"]))
    if not args.rehearse and not result["summary"]["gate_default_not_slower_than_tape"]:
        raise SystemExit("norm_sweep_bench: GATE FAILED: the swept route is slower than the autograd tape")


if __name__ == "__main__":
    main()
