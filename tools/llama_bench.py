"""Cost of nn.RMSNorm (LLaMA / Mistral / Gemma blocks) on the seed-batched reverse sweep (dev tool; writes
profiles/llama_bench.json).

  python tools/llama_bench.py [--out profiles/llama_bench.json]

Two records:
  * kernel (no gate): `lk_rmsnorm_vjp_f32` and `lk_rmsnorm_fwd_f32` beside the torch math of the same rule on the same data
    (`sweep.rmsnorm_vjp_math` / `rmsnorm_forward_math`), S = 9 seeds: the shape of `nets.ViTLlama()` (128 x 64 rows of 192) and one
    with a long row (1024 rows of 4096, the two-pass path).  Time, the minimal bytes - the VJP reads g and writes dx for every seed
    and reads x once, `4 (2 S + 1) rows D`; the forward reads x and writes y, `8 rows D` - and bytes/s of them, and the path
    `lk_rmsnorm_variant` names.  The buffers rotate so that the last-level cache cannot hold them from one launch to the next.
  * end to end (gates): `HipGGN.kron` per minibatch of 128 on `nets.ViTLlama()` in one process, medians of alternating rounds,
    three ways: `use_rmsnorm_kernels` on, off, and `use_sweep = False` (the autograd tape: the route of this model before the
    rules).  GATE 1: the sweep (either way) is never slower than the tape.  GATE 2: `use_rmsnorm_kernels = True` is not slower
    than `False` beyond the spread of the rounds (the larger interquartile range of the two routes' rounds, measured here).

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

LEGS = ("kernel", "vit_llama")
LEG_TIMEOUT = {"kernel": 240, "vit_llama": 300}
ROUTES = ("kernels_on", "kernels_off", "tape")
ROUNDS = 7


def _setup(rehearse: bool):
    import torch

    if rehearse:
        from laplace_amd import _lib
        from tests.emulated_rmsnorm_kernels import EmulatedRmsNormKernels

        _lib.set_kernels_for_testing(EmulatedRmsNormKernels())
        return torch, "cpu"
    if not torch.cuda.is_available():
        raise SystemExit("llama_bench: no ROCm device (a measurement does not fall back to the CPU)")
    return torch, "cuda"


def _median(v):
    return sorted(v)[len(v) // 2]


def _iqr(v):
    s = sorted(v)
    return s[(3 * len(s)) // 4] - s[len(s) // 4]


def leg_kernel(args):
    torch, dev = _setup(args.rehearse)
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep import rmsnorm_forward_math, rmsnorm_vjp_math

    K = get_kernels()
    timer = _Timer(torch, dev)
    S = 2 if args.rehearse else 9
    shapes = [("ViTLlama: [128, 64, 192] rows of the pre-norms", 128 * 64, 192), ("a long row: 1024 rows of 4096 (two-pass)", 1024, 4096)]
    if args.rehearse:
        shapes = [(what, rows // 256, D // 16) for what, rows, D in shapes]
    out = []
    for what, rows, D in shapes:
        vjp_bytes, fwd_bytes = 4 * (2 * S + 1) * rows * D, 8 * rows * D
        nbuf = 1 if args.rehearse else max(2, min(8, -(-(1 << 30) // vjp_bytes)))
        bufs = []
        for _ in range(nbuf):
            x, w = torch.randn(rows, D, device=dev) + 0.5, torch.randn(D, device=dev)
            bufs.append((torch.randn(S * rows, D, device=dev), x, w, rmsnorm_forward_math(x, w, 1e-6)[1].contiguous()))

        def vjp_ours(i):
            g, x, w, rstd = bufs[i % nbuf]
            return K.rmsnorm_vjp(g, x, rstd, w, S)

        def vjp_stock(i):
            g, x, w, rstd = bufs[i % nbuf]
            return rmsnorm_vjp_math(g, x, rstd, w, S)

        def fwd_ours(i):
            _, x, w, _ = bufs[i % nbuf]
            return K.rmsnorm_forward(x, w, 1e-6)

        def fwd_stock(i):
            _, x, w, _ = bufs[i % nbuf]
            return rmsnorm_forward_math(x, w, 1e-6)

        if not args.rehearse:  # the two routes agree on this data to fp32 accuracy
            a, b = vjp_ours(0), vjp_stock(0)
            assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()), what
            (ya, ra), (yb, rb) = fwd_ours(0), fwd_stock(0)
            assert float((ya - yb).abs().max()) <= 1e-5 * float(yb.abs().max()) and float((ra - rb).abs().max()) <= 1e-5 * float(rb.abs().max())
        iters = 2 if args.rehearse else max(2 * nbuf, 20)
        fns = {"vjp_ours": vjp_ours, "vjp_stock": vjp_stock, "fwd_ours": fwd_ours, "fwd_stock": fwd_stock}
        for fn in fns.values():
            for i in range(nbuf):
                fn(i)
        t = {n: [] for n in fns}
        for _ in range(1 if args.rehearse else 5):  # alternating rounds
            for name, fn in fns.items():
                t[name].append(timer(fn, iters))
        med = {n: _median(v) for n, v in t.items()}
        tbps = lambda b, ms: b / (ms * 1e-3) / 1e12  # noqa: E731
        out.append({
            "what": what, "S": S, "rows": rows, "D": D, "buffers_rotated": nbuf, "variant": K.rmsnorm_variant(S, rows, D),
            "lk_rmsnorm_vjp_f32_ms": med["vjp_ours"], "lk_rmsnorm_vjp_f32_ms_rounds": t["vjp_ours"], "vjp_min_bytes": vjp_bytes,
            "lk_rmsnorm_vjp_f32_TBps": tbps(vjp_bytes, med["vjp_ours"]), "vjp_torch_math_ms": med["vjp_stock"],
            "vjp_torch_math_ms_rounds": t["vjp_stock"], "vjp_torch_math_TBps_of_the_same_bytes": tbps(vjp_bytes, med["vjp_stock"]),
            "lk_rmsnorm_fwd_f32_ms": med["fwd_ours"], "lk_rmsnorm_fwd_f32_ms_rounds": t["fwd_ours"], "fwd_min_bytes": fwd_bytes,
            "lk_rmsnorm_fwd_f32_TBps": tbps(fwd_bytes, med["fwd_ours"]), "fwd_torch_math_ms": med["fwd_stock"],
            "fwd_torch_math_ms_rounds": t["fwd_stock"], "fwd_torch_math_TBps_of_the_same_bytes": tbps(fwd_bytes, med["fwd_stock"]),
        })
        print(f"{what}: lk_rmsnorm_vjp_f32 {med['vjp_ours']:8.4f} ms ({out[-1]['lk_rmsnorm_vjp_f32_TBps']:.2f} TB/s of its minimal bytes), "
              f"torch math {med['vjp_stock']:8.4f} ms;   lk_rmsnorm_fwd_f32 {med['fwd_ours']:8.4f} ms "
              f"({out[-1]['lk_rmsnorm_fwd_f32_TBps']:.2f} TB/s), torch math {med['fwd_stock']:8.4f} ms", flush=True)
        del bufs
    return {"shapes": out}


def leg_kron(args):
    """`HipGGN.kron` per minibatch of 128 on the three routes of `nets.ViTLlama()`, alternating rounds in this process"""
    torch, dev = _setup(args.rehearse)
    from laplace_amd import HipGGN
    from laplace_amd.nets import ViTLlama

    torch.manual_seed(0)
    B, hw = (2, 8) if args.rehearse else (128, 32)
    model = (ViTLlama(image=8, dim=32, depth=1, heads=2) if args.rehearse else ViTLlama()).to(dev).eval()
    X, y = torch.randn(B, 3, hw, hw, device=dev), torch.randint(10, (B,), device=dev)
    backends = {}
    for route in ROUTES:  # (`use_rmsnorm_kernels` is read in every forward and reverse sweep: set on the sweep object of each backend)
        b = backends[route] = HipGGN(model, "classification")
        if route == "tape":
            b.use_sweep = False
        b.kron(X, y, N=B)
        sweep = getattr(b._tape(), "sweep", None)
        if sweep not in (None, False):
            sweep.use_rmsnorm_kernels = route == "kernels_on"
        for _ in range(0 if args.rehearse else 2):
            b.kron(X, y, N=B)
    timer = _Timer(torch, dev)
    rounds = {route: [] for route in backends}
    for _ in range(1 if args.rehearse else ROUNDS):  # alternating rounds
        for route, b in backends.items():
            rounds[route].append(timer(lambda i, b=b: b.kron(X, y, N=B), 1 if args.rehearse else 4))
    out = {"network": "ViTLlama()", "input_hw": hw, "batch": B}
    for route, b in backends.items():
        sweep = getattr(b._tape(), "sweep", None)
        out[route] = {"kron_ms": _median(rounds[route]), "kron_ms_rounds": rounds[route], "kron_ms_iqr": _iqr(rounds[route]),
                      "sweep": type(sweep).__name__ if sweep not in (None, False) else None,
                      "sweep_reason": getattr(b._tape(), "sweep_reason", None),
                      "split_ok": bool(getattr(sweep, "split_ok", False)), "split_reason": getattr(sweep, "split_reason", None),
                      "use_rmsnorm_kernels": bool(getattr(sweep, "use_rmsnorm_kernels", False))}
    for route in ("kernels_on", "kernels_off"):
        assert out[route]["sweep"] is not None and not out[route]["split_ok"] and not out[route]["sweep_reason"], out
    assert out["tape"]["sweep"] is None, out
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "llama_bench.json"))
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg:  # child: one leg, result as the last line of stdout
        res = leg_kernel(args) if args.leg == "kernel" else leg_kron(args)
        print("LLAMA_BENCH_RESULT " + json.dumps(res), flush=True)
        return
    result = {"tool": "tools/llama_bench.py", "rehearsal_on_cpu_emulation_times_meaningless": bool(args.rehearse)}
    for leg in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg] + (["--rehearse"] if args.rehearse else [])
        t0 = time.time()
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT[leg], cwd=ROOT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"llama_bench: leg {leg} exceeded {LEG_TIMEOUT[leg]} s; stopping")
        sys.stdout.write(proc.stdout)
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr[-4000:])
            raise SystemExit(f"llama_bench: leg {leg} ended with status {proc.returncode}; stopping")
        line = [l for l in proc.stdout.splitlines() if l.startswith("LLAMA_BENCH_RESULT ")][-1]
        result[leg] = json.loads(line[len("LLAMA_BENCH_RESULT "):])
        result[leg]["leg_wall_s"] = round(time.time() - t0, 1)
    r = result["vit_llama"]
    ms = {route: r[route]["kron_ms"] for route in ROUTES}
    spread = max(r[route]["kron_ms_iqr"] for route in ("kernels_on", "kernels_off"))
    summary = {"kron_ms_per_minibatch_128": ms, "spread_ms_larger_iqr_of_on_and_off_rounds": spread,
               "tape_over_kernels_on": ms["tape"] / ms["kernels_on"], "kernels_off_over_on": ms["kernels_off"] / ms["kernels_on"],
               "gate_1_no_sweep_slower_than_the_tape": max(ms["kernels_on"], ms["kernels_off"]) <= ms["tape"],
               "gate_2_kernels_on_not_slower_than_kernels_off_beyond_the_spread": ms["kernels_on"] <= ms["kernels_off"] + spread}
    result["summary"] = summary
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(summary))
    if not args.rehearse and not summary["gate_1_no_sweep_slower_than_the_tape"]:
        raise SystemExit("llama_bench: GATE 1 FAILED: the sweep is slower than the autograd tape")
    if not args.rehearse and not summary["gate_2_kernels_on_not_slower_than_kernels_off_beyond_the_spread"]:
        raise SystemExit("llama_bench: GATE 2 FAILED: use_rmsnorm_kernels = True is slower than False (the switch belongs off by default)")


if __name__ == "__main__":
    main()
