"""Cost of 1-D convolutional networks on the reverse sweep (dev tool; writes profiles/conv1d_bench.json).

  python tools/conv1d_bench.py [--out profiles/conv1d_bench.json]

Two records:
  * kernel (no gate): `lk_maxred_vjp_f32` beside the torch formulation it replaces (`sweep.reduce_vjp_math`: a comparison against
    the positions or the maximum, a broadcast `where` into a fresh [S, outer, L, inner] tensor; for the first-maximum mode also the
    literal zero fill plus one scatter per seed) at the shapes of `nets.TextCNN()` - `amax(2)` of [128, 100, 128 - k + 1] maps for
    k = 3, 4, 5, S = 4 seeds, the even split - and at a PointNet-style maximum over 1024 points of [128, 1024, 64] features
    (inner = 64, S = 9, the first maximum).  Time, the minimal bytes 4 S (outer inner)(L + 1) and GB/s of them, and the path
    `lk_reduce_variant` names.  The buffers rotate so that the last-level cache cannot hold them from one launch to the next.
  * end to end (gates): `HipGGN.kron` per minibatch of 128 in one process per network, medians of alternating rounds, with the
    spread (max - min of the rounds) reported: `nets.ResNet1d()` on [128, 12, 1024] inputs and `nets.TextCNN()` on [128, 128] token
    ids, on the sweep with `use_reduce_kernels` on and off and with `use_sweep = False` (the autograd tape: the only device route
    of these models before the Conv1d rule).  GATE 1: the sweep is never slower than the tape.  GATE 2: kernels on are not slower
    than off beyond the spread.

One child process per leg, each under its own time limit; a failing leg ends the run.  Times are device events around synchronised
work after a warm-up; no profiler.  `--rehearse` runs tiny shapes on the CPU emulation to check the host logic and writes no times
worth reading (the file says so).
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

LEGS = ("kernel", "resnet1d", "textcnn")
LEG_TIMEOUT = {"kernel": 240, "resnet1d": 420, "textcnn": 300}
ROUTES = ("sweep_kernels_on", "sweep_kernels_off", "tape")


def _setup(rehearse: bool):
    import torch

    if rehearse:
        from laplace_amd import _lib
        from tests.emulated_reduce_kernels import EmulatedReduceKernels

        _lib.set_kernels_for_testing(EmulatedReduceKernels())
        return torch, "cpu"
    if not torch.cuda.is_available():
        raise SystemExit("conv1d_bench: no ROCm device (a measurement does not fall back to the CPU)")
    return torch, "cuda"


def _median(v):
    return sorted(v)[len(v) // 2]


def leg_kernel(args):
    torch, dev = _setup(args.rehearse)
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep import reduce_vjp_math

    K = get_kernels()
    timer = _Timer(torch, dev)
    small = args.rehearse
    # (what, S, outer, L, inner, even)
    shapes = [(f"TextCNN: amax(2) of [128, 100, {128 - k + 1}] (width {k})", 4, (2 if small else 128) * 100, (12 if small else 128) - k + 1, 1, True)
              for k in (3, 4, 5)]
    shapes.append(("PointNet-style: x.max(1)[0] of [128, 1024, 64]", 2 if small else 9, 2 if small else 128, 16 if small else 1024, 64, False))
    rows = []
    for what, S, outer, L, inner, even in shapes:
        moved = 4 * S * outer * inner * (L + 1)
        nbuf = 1 if small else max(2, min(8, -(-(1 << 30) // (2 * moved))))
        xs = [torch.randn(outer, L, inner, device=dev) for _ in range(nbuf)]
        gs = [torch.randn(S, outer, inner, device=dev) for _ in range(nbuf)]
        fwd = [K.maxred_forward(x, outer, L, inner) for x in xs]

        def ours(i):
            y, idx, cnt = fwd[i % nbuf]
            if even:
                return K.maxred_vjp(gs[i % nbuf], S, outer, L, inner, x=xs[i % nbuf], y=y, cnt=cnt)
            return K.maxred_vjp(gs[i % nbuf], S, outer, L, inner, idx=idx)

        def stock(i):
            y, idx, cnt = fwd[i % nbuf]
            if even:
                return reduce_vjp_math(gs[i % nbuf], L, x=xs[i % nbuf], y=y, cnt=cnt)
            return reduce_vjp_math(gs[i % nbuf], L, idx=idx)

        def scatter(i):  # (the literal torch rule of the first-maximum mode: a zero fill and a scatter per seed)
            idx = fwd[i % nbuf][1].to(torch.int64).unsqueeze(1)
            out = torch.zeros(S, outer, L, inner, device=dev)
            for s in range(S):
                out[s].scatter_(1, idx, gs[i % nbuf][s].unsqueeze(1))
            return out

        legs = {"ours": ours, "stock": stock, **({} if even else {"scatter": scatter})}
        a, b = ours(0), stock(0)
        assert torch.equal(a, b) if not even else torch.allclose(a, b, rtol=1e-6, atol=0), what
        if not even:
            assert torch.equal(a, scatter(0)), what
        iters = 2 if small else max(2 * nbuf, 20)
        for fn in legs.values():
            for i in range(nbuf):
                fn(i)
        t = {n: [] for n in legs}
        for _ in range(1 if small else 5):  # alternating rounds
            for name, fn in legs.items():
                t[name].append(timer(fn, iters))
        med = {n: _median(v) for n, v in t.items()}
        row = {"what": what, "S": S, "outer": outer, "L": L, "inner": inner, "mode": "even" if even else "first", "buffers_rotated": nbuf,
               "variant": K.reduce_variant(True, S, outer, L, inner, even, True),
               "maxred_vjp_ms": med["ours"], "maxred_vjp_ms_rounds": t["ours"], "maxred_vjp_min_bytes": moved,
               "maxred_vjp_GBps": moved / (med["ours"] * 1e-3) / 1e9,
               "torch_where_ms": med["stock"], "torch_where_ms_rounds": t["stock"]}
        if not even:
            row.update(torch_zeros_scatter_ms=med["scatter"], torch_zeros_scatter_ms_rounds=t["scatter"])
        rows.append(row)
        print(f"{what}: maxred_vjp {med['ours']:8.4f} ms ({row['maxred_vjp_GBps']:.0f} GB/s of its minimal bytes)   "
              f"torch {med['stock']:8.4f} ms", flush=True)
        del xs, gs, fwd
    return {"shapes": rows}


def leg_kron(args, net):
    """`HipGGN.kron` per minibatch of 128 on the routes of `net`, alternating rounds in this process"""
    torch, dev = _setup(args.rehearse)
    from laplace_amd import HipGGN
    from laplace_amd.nets import ResNet1d, TextCNN

    torch.manual_seed(0)
    small = args.rehearse
    B = 2 if small else 128
    if net == "resnet1d":
        model, name = (ResNet1d(widths=(8, 8, 16, 16), depth=1) if small else ResNet1d()), "ResNet1d()"
        X, shape = torch.randn(B, 12, 64 if small else 1024, device=dev), [B, 12, 64 if small else 1024]
        y = torch.randint(10, (B,), device=dev)
    else:
        model, name = (TextCNN(vocab=50, embed_dim=8, channels=6) if small else TextCNN()), "TextCNN()"
        X, shape = torch.randint(50 if small else 2000, (B, 12 if small else 128), device=dev), [B, 12 if small else 128]
        y = torch.randint(4, (B,), device=dev)
    model = model.to(dev).eval()
    backends = {}
    for route in ROUTES:
        b = backends[route] = HipGGN(model, "classification")
        if route == "tape":
            b.use_sweep = False
        b.kron(X, y, N=B)
        sweep = getattr(b._tape(), "sweep", None)
        if sweep not in (None, False):
            sweep.use_reduce_kernels = route == "sweep_kernels_on"
        for _ in range(0 if small else 2):
            b.kron(X, y, N=B)
    timer = _Timer(torch, dev)
    rounds = {route: [] for route in backends}
    for _ in range(1 if small else 5):  # alternating rounds
        for route, b in backends.items():
            rounds[route].append(timer(lambda i, b=b: b.kron(X, y, N=B), 1 if small else 4))
    out = {"network": name, "input": shape, "batch": B}
    for route, b in backends.items():
        sweep = getattr(b._tape(), "sweep", None)
        out[route] = {"kron_ms": _median(rounds[route]), "kron_ms_rounds": rounds[route],
                      "kron_ms_spread": max(rounds[route]) - min(rounds[route]),
                      "sweep": type(sweep).__name__ if sweep not in (None, False) else None,
                      "sweep_reason": getattr(b._tape(), "sweep_reason", None),
                      "split_reason": getattr(sweep, "split_reason", None),
                      "use_reduce_kernels": bool(getattr(sweep, "use_reduce_kernels", False))}
    for route in ROUTES[:2]:
        assert out[route]["sweep"] is not None and not out[route]["sweep_reason"], out
    assert out["tape"]["sweep"] is None, out
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv1d_bench.json"))
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg:  # child: one leg, result as the last line of stdout
        res = leg_kernel(args) if args.leg == "kernel" else leg_kron(args, args.leg)
        print("CONV1D_BENCH_RESULT " + json.dumps(res), flush=True)
        return
    result = {"tool": "tools/conv1d_bench.py", "rehearsal_on_cpu_emulation_times_meaningless": bool(args.rehearse)}
    for leg in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg] + (["--rehearse"] if args.rehearse else [])
        t0 = time.time()
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT[leg], cwd=ROOT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"conv1d_bench: leg {leg} exceeded {LEG_TIMEOUT[leg]} s; stopping")
        sys.stdout.write(proc.stdout)
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr[-4000:])
            raise SystemExit(f"conv1d_bench: leg {leg} ended with status {proc.returncode}; stopping")
        line = [l for l in proc.stdout.splitlines() if l.startswith("CONV1D_BENCH_RESULT ")][-1]
        result[leg] = json.loads(line[len("CONV1D_BENCH_RESULT "):])
        result[leg]["leg_wall_s"] = round(time.time() - t0, 1)
    nets = ("resnet1d", "textcnn")
    ms = {net: {route: result[net][route]["kron_ms"] for route in ROUTES} for net in nets}
    spread = {net: max(result[net][route]["kron_ms_spread"] for route in ROUTES[:2]) for net in nets}
    summary = {"kron_ms_per_minibatch_128": ms, "kron_ms_spread_of_the_sweep_routes": spread,
               **{f"{net}_tape_over_sweep_kernels_on": ms[net]["tape"] / ms[net]["sweep_kernels_on"] for net in nets},
               **{f"{net}_kernels_off_over_on": ms[net]["sweep_kernels_off"] / ms[net]["sweep_kernels_on"] for net in nets},
               "gate_1_the_sweep_is_never_slower_than_the_tape": bool(all(
                   max(ms[net]["sweep_kernels_on"], ms[net]["sweep_kernels_off"]) <= ms[net]["tape"] for net in nets)),
               "gate_2_kernels_on_not_slower_than_off_beyond_the_spread": bool(all(
                   ms[net]["sweep_kernels_on"] <= ms[net]["sweep_kernels_off"] + spread[net] for net in nets))}
    result["summary"] = summary
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(summary))
    if not args.rehearse and not summary["gate_1_the_sweep_is_never_slower_than_the_tape"]:
        raise SystemExit("conv1d_bench: GATE 1 FAILED: the sweep is slower than the autograd tape")
    if not args.rehearse and not summary["gate_2_kernels_on_not_slower_than_off_beyond_the_spread"]:
        raise SystemExit("conv1d_bench: GATE 2 FAILED: use_reduce_kernels = True is slower than False (the switch belongs off by default)")


if __name__ == "__main__":
    main()
