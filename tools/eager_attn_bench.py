"""Cost of hand-written attention (matmul, / sqrt(d), softmax) on the seed-batched reverse sweep (dev tool; writes
profiles/eager_attn_bench.json).

  python tools/eager_attn_bench.py [--out profiles/eager_attn_bench.json]

Three records:
  * kernel (no gate): `lk_softmax_vjp_f32` and `lk_matmul_vjp_f32` beside the torch math of their rules on the same data
    (`sweep.softmax_vjp_math`, `sweep.matmul_vjp_math`) at the shapes of `nets.ViTEager()`, S = 9 seeds, B = 128: the softmax over
    [128 x 3 x 64] rows of 64 keys, `q @ k^T` ([64, 64] @ [64, 64] per head) and `p @ v`.  Time, the minimal bytes (g read once, the
    per-sample operands once, the outputs written once) and bytes/s of them, and the path the `*_variant` query names.  The buffers
    rotate so that the last-level cache cannot hold them from one launch to the next.
  * end to end (gates): `HipGGN.kron` per minibatch of 128 on `nets.ViTEager()` in one process, medians of alternating rounds,
    five ways: both kernel switches on, `use_matmul_kernels` alone, `use_softmax_kernels` alone, both off (the torch math of the
    rules), and `use_sweep = False` (the autograd tape: the route of this model before the rules).
    GATE 1: the sweep (any way) is never slower than the tape.  GATE 2: both switches on is not slower than both off beyond the
    spread of the rounds (the larger interquartile range of the two routes' rounds, measured here); the same comparison is recorded
    for each switch alone - a switch whose comparison fails ships `False`.
  * `nets.ViTSmall()` (the fused `F.scaled_dot_product_attention`, csrc/lk_attn.hip) on the sweep and on the tape beside it: what
    the `T x T` scores in device memory cost against keeping them on chip.

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

LEGS = ("kernel", "vit_eager", "vit_small")
LEG_TIMEOUT = {"kernel": 240, "vit_eager": 420, "vit_small": 300}
ROUTES = {"vit_eager": ("kernels_on", "matmul_only", "softmax_only", "kernels_off", "tape"), "vit_small": ("sweep", "tape")}
SWITCHES = {"kernels_on": (True, True), "matmul_only": (True, False), "softmax_only": (False, True), "kernels_off": (False, False)}
ROUNDS = 7


def _setup(rehearse: bool):
    import torch

    if rehearse:
        from laplace_amd import _lib
        from tests.emulated_matmul_kernels import EmulatedEagerAttnKernels

        _lib.set_kernels_for_testing(EmulatedEagerAttnKernels())
        return torch, "cpu"
    if not torch.cuda.is_available():
        raise SystemExit("eager_attn_bench: no ROCm device (a measurement does not fall back to the CPU)")
    return torch, "cuda"


def _median(v):
    return sorted(v)[len(v) // 2]


def _iqr(v):
    s = sorted(v)
    return s[(3 * len(s)) // 4] - s[len(s) // 4]


def _race(torch, timer, ours, stock, nbuf, rehearse):
    """medians of alternating rounds of the two routes"""
    iters = 2 if rehearse else max(2 * nbuf, 20)
    for fn in (ours, stock):
        for i in range(nbuf):
            fn(i)
    t = {"ours": [], "stock": []}
    for _ in range(1 if rehearse else 5):
        for name, fn in (("ours", ours), ("stock", stock)):
            t[name].append(timer(fn, iters))
    return {n: _median(v) for n, v in t.items()}, t


def leg_kernel(args):
    torch, dev = _setup(args.rehearse)
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep import matmul_vjp_math, softmax_vjp_math

    K = get_kernels()
    timer = _Timer(torch, dev)
    S, B, H, T, D = (2, 2, 2, 8, 4) if args.rehearse else (9, 128, 3, 64, 64)
    rows = []
    # ---- the softmax over the keys ----
    R, L = B * H * T, T
    moved = 4 * (2 * S * R * L + R * L)  # g read, dx written, y once
    nbuf = 1 if args.rehearse else max(2, min(8, -(-(1 << 30) // moved)))
    bufs = [(torch.randn(S * B, H, T, T, device=dev), torch.softmax(torch.randn(B, H, T, T, device=dev), -1)) for _ in range(nbuf)]

    def ours(i):
        g, y = bufs[i % nbuf]
        return K.softmax_vjp(g, y, S)

    def stock(i):
        g, y = bufs[i % nbuf]
        return softmax_vjp_math(g, y, S, 3)

    if not args.rehearse:  # the two routes agree on this data to fp32 accuracy
        d, d0 = ours(0), stock(0)
        assert float((d - d0).abs().max()) <= 1e-5 * float(d0.abs().max()), "softmax"
    med, t = _race(torch, timer, ours, stock, nbuf, args.rehearse)
    what = f"ViTEager: softmax over [{B} x {H} x {T}] rows of {T} keys"
    rows.append({"what": what, "entry": "lk_softmax_vjp_f32", "S": S, "B": B, "R": R, "L": L, "buffers_rotated": nbuf,
                 "variant": K.softmax_vjp_variant(S, R, L), "kernel_ms": med["ours"], "kernel_ms_rounds": t["ours"], "min_bytes": moved,
                 "kernel_TBps": moved / (med["ours"] * 1e-3) / 1e12, "torch_math_ms": med["stock"], "torch_math_ms_rounds": t["stock"],
                 "torch_math_TBps_of_the_same_bytes": moved / (med["stock"] * 1e-3) / 1e12})
    print(f"{what}: softmax_vjp {med['ours']:8.4f} ms ({rows[-1]['kernel_TBps']:.2f} TB/s of its minimal bytes)   "
          f"torch math {med['stock']:8.4f} ms", flush=True)
    del bufs
    # ---- the two products ----
    for what, (M, Kd, N), b_is_view in ((f"ViTEager: q [{T}, {D}] @ k^T [{D}, {T}]", (T, D, T), True),
                                        (f"ViTEager: p [{T}, {T}] @ v [{T}, {D}]", (T, T, D), False)):
        NB = B * H
        moved = 4 * (S * NB * M * N + NB * M * Kd + NB * Kd * N + S * NB * M * Kd + S * NB * Kd * N)
        nbuf = 1 if args.rehearse else max(2, min(8, -(-(1 << 30) // moved)))
        bufs = [(torch.randn(S * B, H, M, N, device=dev), torch.randn(B, H, M, Kd, device=dev),
                 torch.randn(B, H, N, Kd, device=dev).transpose(-1, -2) if b_is_view else torch.randn(B, H, Kd, N, device=dev))
                for _ in range(nbuf)]

        def ours(i):
            g, a, b = bufs[i % nbuf]
            return K.matmul_vjp(g, a, b.contiguous(), S)  # (the per-sample copy of a transposed view is part of the route)

        def stock(i):
            g, a, b = bufs[i % nbuf]
            return matmul_vjp_math(g, a, b, S)

        if not args.rehearse:
            for x, x0 in zip(ours(0), stock(0)):
                assert float((x - x0).abs().max()) <= 1e-4 * float(x0.abs().max()), what
        med, t = _race(torch, timer, ours, stock, nbuf, args.rehearse)
        rows.append({"what": what, "entry": "lk_matmul_vjp_f32", "S": S, "B": B, "NB": NB, "M": M, "K": Kd, "N": N, "buffers_rotated": nbuf,
                     "variant": K.matmul_vjp_variant(S, NB, M, Kd, N), "kernel_ms": med["ours"], "kernel_ms_rounds": t["ours"],
                     "min_bytes": moved, "kernel_TBps": moved / (med["ours"] * 1e-3) / 1e12, "torch_math_ms": med["stock"],
                     "torch_math_ms_rounds": t["stock"], "torch_math_TBps_of_the_same_bytes": moved / (med["stock"] * 1e-3) / 1e12})
        print(f"{what}: matmul_vjp {med['ours']:8.4f} ms ({rows[-1]['kernel_TBps']:.2f} TB/s of its minimal bytes)   "
              f"torch math {med['stock']:8.4f} ms", flush=True)
        del bufs
    return {"shapes": rows}


def leg_kron(args, net):
    """`HipGGN.kron` per minibatch of 128 on the routes of `net`, alternating rounds in this process"""
    torch, dev = _setup(args.rehearse)
    from laplace_amd import HipGGN
    from laplace_amd.nets import ViTEager, ViTSmall

    torch.manual_seed(0)
    B, hw = (2, 8) if args.rehearse else (128, 32)
    small = dict(image=8, dim=32, depth=1, heads=2)
    if net == "vit_eager":
        model, name = (ViTEager(**small) if args.rehearse else ViTEager()), "ViTEager()"
    else:
        model, name = (ViTSmall(**small) if args.rehearse else ViTSmall()), "ViTSmall()"
    model = model.to(dev).eval()
    X, y = torch.randn(B, 3, hw, hw, device=dev), torch.randint(10, (B,), device=dev)
    backends = {}
    for route in ROUTES[net]:  # (the switches are read in every reverse sweep: set on the sweep object of each backend)
        b = backends[route] = HipGGN(model, "classification")
        if route == "tape":
            b.use_sweep = False
        b.kron(X, y, N=B)
        sweep = getattr(b._tape(), "sweep", None)
        if sweep not in (None, False) and route in SWITCHES:
            sweep.use_matmul_kernels, sweep.use_softmax_kernels = SWITCHES[route]
        for _ in range(0 if args.rehearse else 2):
            b.kron(X, y, N=B)
    timer = _Timer(torch, dev)
    rounds = {route: [] for route in backends}
    for _ in range(1 if args.rehearse else ROUNDS):  # alternating rounds
        for route, b in backends.items():
            rounds[route].append(timer(lambda i, b=b: b.kron(X, y, N=B), 1 if args.rehearse else 4))
    out = {"network": name, "input_hw": hw, "batch": B}
    for route, b in backends.items():
        sweep = getattr(b._tape(), "sweep", None)
        out[route] = {"kron_ms": _median(rounds[route]), "kron_ms_rounds": rounds[route], "kron_ms_iqr": _iqr(rounds[route]),
                      "sweep": type(sweep).__name__ if sweep not in (None, False) else None,
                      "sweep_reason": getattr(b._tape(), "sweep_reason", None),
                      "split_ok": bool(getattr(sweep, "split_ok", False)), "split_reason": getattr(sweep, "split_reason", None),
                      "use_matmul_kernels": bool(getattr(sweep, "use_matmul_kernels", False)),
                      "use_softmax_kernels": bool(getattr(sweep, "use_softmax_kernels", False))}
    for route in ROUTES[net][:-1]:
        assert out[route]["sweep"] is not None and not out[route]["split_ok"] and not out[route]["sweep_reason"], out
    assert out["tape"]["sweep"] is None, out
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eager_attn_bench.json"))
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg:  # child: one leg, result as the last line of stdout
        res = leg_kernel(args) if args.leg == "kernel" else leg_kron(args, args.leg)
        print("EAGER_ATTN_BENCH_RESULT " + json.dumps(res), flush=True)
        return
    result = {"tool": "tools/eager_attn_bench.py", "rehearsal_on_cpu_emulation_times_meaningless": bool(args.rehearse)}
    for leg in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg] + (["--rehearse"] if args.rehearse else [])
        t0 = time.time()
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT[leg], cwd=ROOT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"eager_attn_bench: leg {leg} exceeded {LEG_TIMEOUT[leg]} s; stopping")
        sys.stdout.write(proc.stdout)
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr[-4000:])
            raise SystemExit(f"eager_attn_bench: leg {leg} ended with status {proc.returncode}; stopping")
        line = [l for l in proc.stdout.splitlines() if l.startswith("EAGER_ATTN_BENCH_RESULT ")][-1]
        result[leg] = json.loads(line[len("EAGER_ATTN_BENCH_RESULT "):])
        result[leg]["leg_wall_s"] = round(time.time() - t0, 1)
    ms = {net: {route: result[net][route]["kron_ms"] for route in ROUTES[net]} for net in LEGS[1:]}
    e, iqr = ms["vit_eager"], {route: result["vit_eager"][route]["kron_ms_iqr"] for route in SWITCHES}
    not_slower = {route: e[route] <= e["kernels_off"] + max(iqr[route], iqr["kernels_off"]) for route in ("kernels_on", "matmul_only", "softmax_only")}
    summary = {"kron_ms_per_minibatch_128": ms, "vit_eager_iqr_ms_of_the_rounds": iqr,
               "vit_eager_tape_over_kernels_on": e["tape"] / e["kernels_on"], "vit_eager_tape_over_kernels_off": e["tape"] / e["kernels_off"],
               "vit_eager_kernels_off_over_on": e["kernels_off"] / e["kernels_on"],
               "vit_eager_kernels_on_over_vit_small_sweep": e["kernels_on"] / ms["vit_small"]["sweep"],
               "gate_1_no_sweep_slower_than_the_tape": all(e[route] <= e["tape"] for route in SWITCHES),
               "gate_2_kernels_on_not_slower_than_kernels_off_beyond_the_spread": not_slower["kernels_on"],
               "each_switch_alone_not_slower_than_kernels_off_beyond_the_spread": {k: not_slower[k] for k in ("matmul_only", "softmax_only")}}
    result["summary"] = summary
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(summary))
    if not args.rehearse and not summary["gate_1_no_sweep_slower_than_the_tape"]:
        raise SystemExit("eager_attn_bench: GATE 1 FAILED: the sweep is slower than the autograd tape")
    if not args.rehearse and not summary["gate_2_kernels_on_not_slower_than_kernels_off_beyond_the_spread"]:
        raise SystemExit("eager_attn_bench: GATE 2 FAILED: the kernels are slower than the torch math (the switches belong off by default)")


if __name__ == "__main__":
    main()
