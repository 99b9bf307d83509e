"""Cost of crossing scaled dot-product attention in the seed-batched reverse sweep (dev tool; writes profiles/attn_bench.json).

  python tools/attn_bench.py [--out profiles/attn_bench.json]

Two records:
  * kernel: `lk_attn_vjp_f32` (one call for all seeds) at S = 9, B = 128, H = 3, T = 64, D = 64 (`nets.ViTSmall()`) and at S = 1,
    B = 32, H = 12, T = 128, D = 64 (the attention shape of the c5 encoder), operands in layout 1 as the sweep hands them over,
    beside (a) the torch-math rule `sweep.attn_vjp_math` on the same tensors and (b) S stock backward passes of
    `F.scaled_dot_product_attention`, alternating in one process; achieved bytes/s against the minimal traffic of
    include/laplace_hip.h.  The cotangents rotate through enough buffers (>= 1 GiB in all) that the last-level cache cannot hold
    them from one launch to the next.  The forward `lk_attn_fwd_f32` beside `sweep.attn_forward_math` is recorded too.
  * end to end: `HipGGN.kron` per minibatch of 128 on `nets.ViTSmall()` with the kernels, with `use_attn_kernels = False` (the
    torch math inside the sweep) and with `use_sweep = False` (the autograd tape: one stock reverse pass per seed, the route this
    model took before the sweep had a rule for attention).
GATE: with the kernels on, no line is slower than the torch-math route, and the sweep is not slower than the tape.

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

SHAPES = [dict(name="vit-small", S=9, B=128, H=3, T=64, D=64), dict(name="c5-encoder", S=1, B=32, H=12, T=128, D=64)]
LEGS = ("kernel", "kernels_on", "math", "tape")
LEG_TIMEOUT = {"kernel": 240, "kernels_on": 150, "math": 150, "tape": 200}


def _setup(rehearse: bool):
    import torch

    if rehearse:
        from laplace_amd import _lib
        from tests.emulated_attn_kernels import EmulatedAttnKernels

        _lib.set_kernels_for_testing(EmulatedAttnKernels())
        return torch, "cpu"
    if not torch.cuda.is_available():
        raise SystemExit("attn_bench: no ROCm device (a measurement does not fall back to the CPU)")
    return torch, "cuda"


def _median(v):
    return sorted(v)[len(v) // 2]


def leg_kernel(args):
    torch, dev = _setup(args.rehearse)
    import torch.nn.functional as F

    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep import attn_forward_math, attn_vjp_math

    K = get_kernels()
    timer = _Timer(torch, dev)
    rows = []
    for shp in SHAPES:
        S, B, H, T, D = (2, 2, 2, 5, 4) if args.rehearse else (shp["S"], shp["B"], shp["H"], shp["T"], shp["D"])
        scale = D ** -0.5
        lay1 = lambda *s: torch.randn(s[0], s[2], s[1], s[3], device=dev).transpose(1, 2)  # noqa: E731  ([N][T][H][D] memory)
        go_bytes = 4 * S * B * H * T * D
        nbuf = 1 if args.rehearse else max(2, min(32, -(-(1 << 30) // go_bytes)))
        q, k, v = lay1(B, H, T, D), lay1(B, H, T, D), lay1(B, H, T, D)
        gos = [lay1(S * B, H, T, D) for _ in range(nbuf)]
        o, lse = K.attn_forward(q, k, v, scale, False)
        o_m, p_m = attn_forward_math(q, k, v, scale, False)
        qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        out = F.scaled_dot_product_attention(qr, kr, vr)

        def kern(i):
            K.attn_vjp(gos[i % nbuf], q, k, v, o, lse, S, scale, False)

        def math(i):
            attn_vjp_math(gos[i % nbuf], q, k, v, o_m, p_m, S, scale)

        def stock(i):
            g = gos[i % nbuf].reshape(S, B, H, T, D)
            for s in range(S):
                torch.autograd.grad(out, (qr, kr, vr), g[s], retain_graph=True)

        def fwd_kern(i):
            K.attn_forward(q, k, v, scale, False)

        def fwd_math(i):
            attn_forward_math(q, k, v, scale, False)

        iters = 2 if args.rehearse else max(nbuf, 10)
        fns = (kern, math, stock, fwd_kern, fwd_math)
        for fn in fns:  # warm-up of all at this shape
            for i in range(min(nbuf, 3)):
                fn(i)
        times = [[] for _ in fns]
        for _ in range(1 if args.rehearse else 5):  # alternating rounds
            for t, fn in zip(times, fns):
                t.append(timer(fn, iters))
        med = [_median(t) for t in times]
        moved = 5 * go_bytes + 8 * S * B * H * T + 24 * B * H * T * D + 8 * B * H * T
        rows.append({
            "shape": shp["name"], "S": S, "B": B, "H": H, "T": T, "D": D, "layout": 1, "cotangent_bytes": go_bytes,
            "buffers_rotated": nbuf, "variant": K.attn_variant(S, B, H, T, D, 1, False),
            "attn_vjp_ms": med[0], "attn_vjp_ms_rounds": times[0], "attn_vjp_min_bytes": moved,
            "attn_vjp_TBps": moved / (med[0] * 1e-3) / 1e12,
            "attn_vjp_tflops": 2.0 * 5 * S * B * H * T * T * D / (med[0] * 1e-3) / 1e12,  # (P rebuilt once per owner pass not counted)
            "torch_math_vjp_ms": med[1], "torch_math_vjp_ms_rounds": times[1],
            "stock_backward_x_S_ms": med[2], "stock_backward_x_S_ms_rounds": times[2],
            "attn_fwd_ms": med[3], "attn_fwd_ms_rounds": times[3], "torch_math_fwd_ms": med[4], "torch_math_fwd_ms_rounds": times[4],
        })
        print(f"{shp['name']:10s} S={S} B={B} H={H} T={T} D={D}: attn_vjp {med[0]:8.4f} ms ({rows[-1]['attn_vjp_TBps']:.3f} TB/s)   "
              f"torch math {med[1]:8.4f} ms   {S} stock backward passes {med[2]:8.4f} ms   fwd {med[3]:.4f} ms vs math {med[4]:.4f} ms",
              flush=True)
        del gos
    return {"shapes": rows}


def leg_kron(args, route):
    """`HipGGN.kron` per minibatch of 128 on nets.ViTSmall() (LayerNorm affines frozen)"""
    torch, dev = _setup(args.rehearse)
    from laplace_amd import HipGGN
    from laplace_amd.nets import ViTSmall

    torch.manual_seed(0)
    B = 2 if args.rehearse else 128
    model = (ViTSmall(dim=16, depth=1, heads=2, image=8) if args.rehearse else ViTSmall()).to(dev).eval()
    b = HipGGN(model, "classification")
    if route == "tape":
        b.use_sweep = False
    elif route == "math":
        b.use_attn_kernels = False
    X = torch.randn(B, 3, 8 if args.rehearse else 32, 8 if args.rehearse else 32, device=dev)
    y = torch.randint(10, (B,), device=dev)
    timer = _Timer(torch, dev)
    for _ in range(1 if args.rehearse else 3):
        b.kron(X, y, N=B)
    rounds = [timer(lambda i: b.kron(X, y, N=B), 1 if args.rehearse else 5) for _ in range(1 if args.rehearse else 3)]
    sweep = getattr(b._tape(), "sweep", None)
    served = None
    if route != "tape":
        assert sweep not in (None, False), getattr(b._tape(), "sweep_reason", None)
        from laplace_amd.sweep import ATTN

        b._forward(X)  # (what the attention nodes kept tells which branch of the rule served them)
        served = sorted({"kernels" if sweep.saved[n][0] is not None else "math" for n, r in sweep.rule.items() if r.kind == ATTN})
        sweep.release()
    return {"route": route, "batch": B, "kron_ms": _median(rounds), "kron_ms_rounds": rounds,
            "sweep": type(sweep).__name__ if sweep not in (None, False) else None, "attention_served_by": served,
            "split_reason": getattr(sweep, "split_reason", None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_bench.json"))
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg:  # child: one leg, result as the last line of stdout
        res = leg_kernel(args) if args.leg == "kernel" else leg_kron(args, args.leg)
        print("ATTN_BENCH_RESULT " + json.dumps(res), flush=True)
        return
    result = {"tool": "tools/attn_bench.py", "rehearsal_on_cpu_emulation_times_meaningless": bool(args.rehearse)}
    for leg in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg] + (["--rehearse"] if args.rehearse else [])
        t0 = time.time()
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT[leg], cwd=ROOT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"attn_bench: leg {leg} exceeded {LEG_TIMEOUT[leg]} s; stopping")
        sys.stdout.write(proc.stdout)
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr[-4000:])
            raise SystemExit(f"attn_bench: leg {leg} ended with status {proc.returncode}; stopping")
        line = [l for l in proc.stdout.splitlines() if l.startswith("ATTN_BENCH_RESULT ")][-1]
        result[leg] = json.loads(line[len("ATTN_BENCH_RESULT "):])
        result[leg]["leg_wall_s"] = round(time.time() - t0, 1)
    on, ma, tp = result["kernels_on"]["kron_ms"], result["math"]["kron_ms"], result["tape"]["kron_ms"]
    lines = {r["shape"]: {"attn_vjp_ms": r["attn_vjp_ms"], "torch_math_vjp_ms": r["torch_math_vjp_ms"],
                          "stock_backward_x_S_ms": r["stock_backward_x_S_ms"], "attn_fwd_ms": r["attn_fwd_ms"],
                          "torch_math_fwd_ms": r["torch_math_fwd_ms"]} for r in result["kernel"]["shapes"]}
    kernel_ok = all(v["attn_vjp_ms"] <= v["torch_math_vjp_ms"] and v["attn_fwd_ms"] <= v["torch_math_fwd_ms"] for v in lines.values())
    result["summary"] = {"kernel_lines": lines, "kron_ms_per_minibatch_128_kernels": on, "kron_ms_per_minibatch_128_torch_math": ma,
                         "kron_ms_per_minibatch_128_autograd_tape": tp, "gain_over_tape": tp / on, "gain_over_torch_math": ma / on,
                         "gate_kernel_lines_not_slower_than_torch_math": bool(kernel_ok),
                         "gate_kron_with_kernels_not_slower_than_torch_math": bool(on <= ma),
                         "gate_sweep_not_slower_than_tape": bool(min(on, ma) <= tp),
                         "gate": bool(kernel_ok and on <= ma and on <= tp)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result["summary"]))
    if not args.rehearse and not result["summary"]["gate"]:
        raise SystemExit("attn_bench: GATE FAILED (see the summary): the kernels ship switched off unless every line holds")


if __name__ == "__main__":
    main()
