"""Cost of element-wise products (squeeze-and-excitation gates, SwiGLU) on the seed-batched reverse sweep (dev tool; writes
profiles/mul_bench.json).

  python tools/mul_bench.py [--out profiles/mul_bench.json]

Three records:
  * kernel (no gate): `lk_mul_vjp_f32` beside the torch math of the same rule on the same data (`g * b`, `g * a` and - for a gate -
    a sum over the trailing dims), S = 9 seeds, B = 128: the row form at the three gates of `nets.SEResNetSmall()` (C = 32 at
    32 x 32, C = 64 at 16 x 16, C = 128 at 8 x 8) and the full form at the gated feed-forward of `nets.ViTSwiGLU()` ([128, 64, 512]).
    Time, the minimal bytes (g read once, a and b once, both outputs written) and bytes/s of them, and the path `lk_mul_variant`
    names.  The buffers rotate so that the last-level cache cannot hold them from one launch to the next.
  * end to end (gates): `HipGGN.kron` per minibatch of 128 in one process per network, medians of alternating rounds, three ways:
    `use_mul_kernels` on, off, and `use_sweep = False` (the autograd tape: the route of these models before the rule).
    GATE 1: the sweep (either way) is never slower than the tape.  GATE 2: `use_mul_kernels = True` is not slower than `False`
    beyond the spread of the rounds (the larger interquartile range of the two routes' rounds, measured here).

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

LEGS = ("kernel", "se_resnet_small", "vit_swiglu")
LEG_TIMEOUT = {"kernel": 240, "se_resnet_small": 300, "vit_swiglu": 300}
ROUTES = ("kernels_on", "kernels_off", "tape")
ROUNDS = 7


def _setup(rehearse: bool):
    import torch

    if rehearse:
        from laplace_amd import _lib
        from tests.emulated_mul_kernels import EmulatedMulKernels

        _lib.set_kernels_for_testing(EmulatedMulKernels())
        return torch, "cpu"
    if not torch.cuda.is_available():
        raise SystemExit("mul_bench: no ROCm device (a measurement does not fall back to the CPU)")
    return torch, "cuda"


def _median(v):
    return sorted(v)[len(v) // 2]


def _iqr(v):
    s = sorted(v)
    return s[(3 * len(s)) // 4] - s[len(s) // 4]


def leg_kernel(args):
    torch, dev = _setup(args.rehearse)
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    timer = _Timer(torch, dev)
    S, B = (2, 2) if args.rehearse else (9, 128)
    sc = 4 if args.rehearse else 1  # (the rehearsal shrinks the maps)
    # (what, shape of a per sample, shape of b per sample)
    shapes = [("SEResNetSmall stage 1: map [32, 32, 32] * gate [32, 1, 1]", (32, 32 // sc, 32 // sc), (32, 1, 1)),
              ("SEResNetSmall stage 2: map [64, 16, 16] * gate [64, 1, 1]", (64, 16 // sc, 16 // sc), (64, 1, 1)),
              ("SEResNetSmall stage 3: map [128, 8, 8] * gate [128, 1, 1]", (128, 8 // sc, 8 // sc), (128, 1, 1)),
              ("ViTSwiGLU: silu(w1 x) [64, 512] * w3 x [64, 512]", (64 // sc, 512 // sc), (64 // sc, 512 // sc))]
    rows = []
    for what, sa, sb in shapes:
        row = sa != sb
        na = 1
        for d in sa:
            na *= d
        nb = sb[0] if row else na
        R, L = (B * nb, na // nb) if row else (B, na)
        moved = 4 * (S * B * na + B * na + B * nb + S * B * na + S * B * nb)  # g, a, b read once; da and db written
        nbuf = 1 if args.rehearse else max(2, min(8, -(-(1 << 30) // moved)))
        bufs = [(torch.randn(S * B, *sa, device=dev), torch.randn(B, *sa, device=dev), torch.randn(B, *sb, device=dev))
                for _ in range(nbuf)]

        def ours(i):
            g, a, b = bufs[i % nbuf]
            return K.mul_vjp(g, a, b, S, row)

        def stock(i):
            g, a, b = bufs[i % nbuf]
            gv = g.reshape(S, *a.shape)
            da = (gv * b).reshape(g.shape)
            db = gv * a
            db = db.sum(tuple(range(3, gv.dim())), keepdim=True).reshape(S * B, *sb) if row else db.reshape(g.shape)
            return da, db

        if not args.rehearse:  # the two routes agree on this data: the products bit for bit, the row sums to fp32 accuracy
            (da, db), (da0, db0) = ours(0), stock(0)
            assert torch.equal(da, da0), what
            assert torch.equal(db, db0) if not row else float((db - db0).abs().max()) <= 1e-4 * float(db0.abs().max()), what
        iters = 2 if args.rehearse else max(2 * nbuf, 20)
        for fn in (ours, stock):
            for i in range(nbuf):
                fn(i)
        t = {"ours": [], "stock": []}
        for _ in range(1 if args.rehearse else 5):  # alternating rounds
            for name, fn in (("ours", ours), ("stock", stock)):
                t[name].append(timer(fn, iters))
        med = {n: _median(v) for n, v in t.items()}
        rows.append({
            "what": what, "form": "row" if row else "full", "S": S, "B": B, "R": R, "L": L, "buffers_rotated": nbuf,
            "variant": K.mul_variant(S, R, L, row), "mul_vjp_ms": med["ours"], "mul_vjp_ms_rounds": t["ours"], "mul_vjp_min_bytes": moved,
            "mul_vjp_TBps": moved / (med["ours"] * 1e-3) / 1e12, "torch_math_ms": med["stock"], "torch_math_ms_rounds": t["stock"],
            "torch_math_TBps_of_the_same_bytes": moved / (med["stock"] * 1e-3) / 1e12,
        })
        print(f"{what}: mul_vjp {med['ours']:8.4f} ms ({rows[-1]['mul_vjp_TBps']:.2f} TB/s of its minimal bytes)   "
              f"torch math {med['stock']:8.4f} ms", flush=True)
        del bufs
    return {"shapes": rows}


def leg_kron(args, net):
    """`HipGGN.kron` per minibatch of 128 on the three routes of `net`, alternating rounds in this process"""
    torch, dev = _setup(args.rehearse)
    from laplace_amd import HipGGN
    from laplace_amd.nets import SEResNetSmall, ViTSwiGLU

    torch.manual_seed(0)
    B, hw = (2, 8) if args.rehearse else (128, 32)
    if net == "se_resnet_small":
        model, name = (SEResNetSmall(widths=(8, 16), depth=1) if args.rehearse else SEResNetSmall()), "SEResNetSmall()"
    else:
        model, name = (ViTSwiGLU(image=8, dim=32, depth=1, heads=2) if args.rehearse else ViTSwiGLU()), "ViTSwiGLU()"
    model = model.to(dev).eval()
    X, y = torch.randn(B, 3, hw, hw, device=dev), torch.randint(10, (B,), device=dev)
    backends = {}
    for route in ROUTES:  # (`use_mul_kernels` is read in every reverse sweep: set on the sweep object of each backend)
        b = backends[route] = HipGGN(model, "classification")
        if route == "tape":
            b.use_sweep = False
        b.kron(X, y, N=B)
        sweep = getattr(b._tape(), "sweep", None)
        if sweep not in (None, False):
            sweep.use_mul_kernels = route == "kernels_on"
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
                      "use_mul_kernels": bool(getattr(sweep, "use_mul_kernels", False))}
    for route in ("kernels_on", "kernels_off"):
        assert out[route]["sweep"] is not None and not out[route]["split_ok"] and not out[route]["sweep_reason"], out
    assert out["tape"]["sweep"] is None, out
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mul_bench.json"))
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg:  # child: one leg, result as the last line of stdout
        res = leg_kernel(args) if args.leg == "kernel" else leg_kron(args, args.leg)
        print("MUL_BENCH_RESULT " + json.dumps(res), flush=True)
        return
    result = {"tool": "tools/mul_bench.py", "rehearsal_on_cpu_emulation_times_meaningless": bool(args.rehearse)}
    for leg in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg] + (["--rehearse"] if args.rehearse else [])
        t0 = time.time()
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT[leg], cwd=ROOT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"mul_bench: leg {leg} exceeded {LEG_TIMEOUT[leg]} s; stopping")
        sys.stdout.write(proc.stdout)
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr[-4000:])
            raise SystemExit(f"mul_bench: leg {leg} ended with status {proc.returncode}; stopping")
        line = [l for l in proc.stdout.splitlines() if l.startswith("MUL_BENCH_RESULT ")][-1]
        result[leg] = json.loads(line[len("MUL_BENCH_RESULT "):])
        result[leg]["leg_wall_s"] = round(time.time() - t0, 1)
    nets = LEGS[1:]
    ms = {net: {route: result[net][route]["kron_ms"] for route in ROUTES} for net in nets}
    spread = {net: max(result[net][route]["kron_ms_iqr"] for route in ("kernels_on", "kernels_off")) for net in nets}
    summary = {"kron_ms_per_minibatch_128": ms, "spread_ms_larger_iqr_of_on_and_off_rounds": spread,
               **{f"{net}_tape_over_kernels_on": ms[net]["tape"] / ms[net]["kernels_on"] for net in nets},
               **{f"{net}_kernels_off_over_on": ms[net]["kernels_off"] / ms[net]["kernels_on"] for net in nets},
               "gate_1_no_sweep_slower_than_the_tape": all(max(ms[net]["kernels_on"], ms[net]["kernels_off"]) <= ms[net]["tape"] for net in nets),
               "gate_2_kernels_on_not_slower_than_kernels_off_beyond_the_spread":
                   all(ms[net]["kernels_on"] <= ms[net]["kernels_off"] + spread[net] for net in nets)}
    result["summary"] = summary
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(summary))
    if not args.rehearse and not summary["gate_1_no_sweep_slower_than_the_tape"]:
        raise SystemExit("mul_bench: GATE 1 FAILED: the sweep is slower than the autograd tape")
    if not args.rehearse and not summary["gate_2_kernels_on_not_slower_than_kernels_off_beyond_the_spread"]:
        raise SystemExit("mul_bench: GATE 2 FAILED: use_mul_kernels = True is slower than False (the switch belongs off by default)")


if __name__ == "__main__":
    main()
