"""Cost of upsampling and padding on the reverse sweep (dev tool; writes profiles/resample_bench.json).

  python tools/resample_bench.py [--out profiles/resample_bench.json]

Two records:
  * kernel (no gate): `lk_resample_vjp_f32` at the shapes of the workloads - the two top-down steps of `nets.FPNSmall()` on
    [128, 3, 32, 32] inputs (8x8 -> 16x16 and 16x16 -> 32x32 maps of 64 channels, nearest and bilinear) and the causal pads of
    `nets.TCNSmall()` on [128, 8, 256] inputs (zeros, left pad 16; reflection, left pad 4), S = 10 seeds - beside two alternatives:
    the two-matmul form of the rule (`sweep.resample_vjp_math`) and stock autograd's own backward of the operation on the
    [S B, C, ...] tensor.  Time, the minimal bytes 4 P (OH OW + H W) and TB/s of them, and the path `lk_resample_variant` names.
    The buffers rotate so that the last-level cache cannot hold them from one launch to the next.
  * end to end (gates): `HipGGN.kron` per minibatch of 128 in one process per network, medians of alternating rounds, with the
    spread (max - min of the rounds) reported: `FPNSmall()` in both modes and `TCNSmall()`, on the sweep with
    `use_resample_kernels` on and off and with `use_sweep = False` (the autograd tape: the only route of these models before the
    rule).  GATE 1: the sweep is never slower than the tape.  GATE 2: kernels on are not slower than off beyond the spread.

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

LEGS = ("kernel", "fpn_nearest", "fpn_bilinear", "tcn")
LEG_TIMEOUT = {"kernel": 240, "fpn_nearest": 240, "fpn_bilinear": 240, "tcn": 240}
ROUTES = ("sweep_kernels_on", "sweep_kernels_off", "tape")
NETS = LEGS[1:]


def _setup(rehearse: bool):
    import torch

    if rehearse:
        from laplace_amd import _lib
        from tests.emulated_resample_kernels import EmulatedResampleKernels

        _lib.set_kernels_for_testing(EmulatedResampleKernels())
        return torch, "cpu"
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench: no ROCm device (a measurement does not fall back to the CPU)")
    return torch, "cuda"


def _median(v):
    return sorted(v)[len(v) // 2]


def leg_kernel(args):
    torch, dev = _setup(args.rehearse)
    import torch.nn.functional as F

    from laplace_amd import sweep as sw
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    timer = _Timer(torch, dev)
    small = args.rehearse
    S, B, C = (2, 2, 4) if small else (10, 128, 64)
    up = dict(size=None, recompute_scale_factor=None, antialias=False, scale_factor=2)
    L = 24 if small else 256
    # (what, op, keyword arguments, k, (H, W))
    shapes = []
    for h in ((4,) if small else (8, 16)):
        shapes.append((f"FPNSmall: nearest x2 of [{B}, {C}, {h}, {h}]", "interpolate", dict(up, mode="nearest", align_corners=None), 2, (h, h)))
        shapes.append((f"FPNSmall: bilinear x2 of [{B}, {C}, {h}, {h}]", "interpolate", dict(up, mode="bilinear", align_corners=False), 2, (h, h)))
    shapes.append((f"TCNSmall: F.pad(x, (16, 0)) of [{B}, {C}, {L}]", "pad", dict(pad=(16, 0), mode="constant", value=None), 1, (1, L)))
    shapes.append((f"TCNSmall: ReflectionPad1d((4, 0)) of [{B}, {C}, {L}]", "pad", dict(pad=(4, 0), mode="reflect", value=None), 1, (1, L)))
    rows = []
    for what, op, kw, k, (H, W) in shapes:
        fn = F.interpolate if op == "interpolate" else F.pad
        lead = (S * B, C) + ((H,) if k == 2 else ())
        x0 = torch.zeros(*lead, W, device=dev)
        y0 = fn(x0, **kw)
        OH, OW = (int(y0.shape[-2]) if k == 2 else 1), int(y0.shape[-1])
        t = sw.resample_tables(op, kw, (H, W), (OH, OW), k, x0)
        axes = (K.resample_pack(*t.csr_h, H, OH), K.resample_pack(*t.csr_w, W, OW))
        P = S * B * C
        moved = 4 * P * (OH * OW + H * W)
        nbuf = 1 if small else max(2, min(8, -(-(1 << 30) // (2 * moved))))
        gs = [torch.randn(P, OH, OW, device=dev) for _ in range(nbuf)]
        xs = [torch.randn(*lead, W, device=dev).requires_grad_(True) for _ in range(nbuf)]
        ys = [fn(x, **kw) for x in xs]

        def ours(i):
            return K.resample_vjp(gs[i % nbuf], *axes)

        def matmuls(i):
            return sw.resample_vjp_math(gs[i % nbuf], t.Mh, t.Mw)

        def stock(i):  # (autograd's own backward of the operation: atomics for bilinear and reflection)
            return torch.autograd.grad(ys[i % nbuf], xs[i % nbuf], gs[i % nbuf].view_as(ys[i % nbuf]), retain_graph=True)[0]

        legs = {"ours": ours, "matmuls": matmuls, "stock": stock}
        a, b, c = ours(0), matmuls(0), stock(0).reshape(P, H, W)
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-5) and torch.allclose(a, c, rtol=1e-4, atol=1e-5), what
        iters = 2 if small else max(2 * nbuf, 10)
        for f_ in legs.values():
            for i in range(nbuf):
                f_(i)
        tm = {n: [] for n in legs}
        for _ in range(1 if small else 5):  # alternating rounds
            for name, f_ in legs.items():
                tm[name].append(timer(f_, iters))
        med = {n: _median(v) for n, v in tm.items()}
        row = {"what": what, "P": P, "OH": OH, "OW": OW, "H": H, "W": W, "taps": list(t.taps), "buffers_rotated": nbuf,
               "variant": K.resample_variant(P, OH, OW, H, W, *t.taps, True),
               "resample_vjp_ms": med["ours"], "resample_vjp_ms_rounds": tm["ours"], "resample_vjp_min_bytes": moved,
               "resample_vjp_TBps": moved / (med["ours"] * 1e-3) / 1e12,
               "two_matmuls_ms": med["matmuls"], "two_matmuls_ms_rounds": tm["matmuls"],
               "autograd_backward_ms": med["stock"], "autograd_backward_ms_rounds": tm["stock"]}
        rows.append(row)
        print(f"{what}: resample_vjp {med['ours']:8.4f} ms ({row['resample_vjp_TBps']:.2f} TB/s of its minimal bytes)   "
              f"two matmuls {med['matmuls']:8.4f} ms   autograd {med['stock']:8.4f} ms", flush=True)
        del gs, xs, ys
    return {"shapes": rows}


def leg_kron(args, net):
    """`HipGGN.kron` per minibatch of 128 on the routes of `net`, alternating rounds in this process"""
    torch, dev = _setup(args.rehearse)
    from laplace_amd import HipGGN
    from laplace_amd.nets import FPNSmall, TCNSmall

    torch.manual_seed(0)
    small = args.rehearse
    B = 2 if small else 128
    if net.startswith("fpn"):
        mode = net.split("_")[1]
        model = FPNSmall(10, (32, 32, 64), 32, mode) if small else FPNSmall(mode=mode)
        name, shape = f"FPNSmall(mode={mode!r})", [B, 3, 16 if small else 32, 16 if small else 32]
    else:
        model = TCNSmall(10, 8, 8, dilations=(1, 2)) if small else TCNSmall()
        name, shape = "TCNSmall()", [B, 8, 24 if small else 256]
    X, y = torch.randn(*shape, device=dev), torch.randint(10, (B,), device=dev)
    model = model.to(dev).eval()
    backends = {}
    for route in ROUTES:
        b = backends[route] = HipGGN(model, "classification")
        if route == "tape":
            b.use_sweep = False
        b.kron(X, y, N=B)
        sweep = getattr(b._tape(), "sweep", None)
        if sweep not in (None, False):
            sweep.use_resample_kernels = route == "sweep_kernels_on"
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
                      "resample_route": sorted(set(getattr(sweep, "resample_route", {}).values()))}
    for route in ROUTES[:2]:
        assert out[route]["sweep"] is not None and not out[route]["sweep_reason"], out
    assert out["sweep_kernels_on"]["resample_route"] == ["kernel"], out
    assert out["tape"]["sweep"] is None, out
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg:  # child: one leg, result as the last line of stdout
        res = leg_kernel(args) if args.leg == "kernel" else leg_kron(args, args.leg)
        print("RESAMPLE_BENCH_RESULT " + json.dumps(res), flush=True)
        return
    result = {"tool": "tools/resample_bench.py", "rehearsal_on_cpu_emulation_times_meaningless": bool(args.rehearse)}
    for leg in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg] + (["--rehearse"] if args.rehearse else [])
        t0 = time.time()
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT[leg], cwd=ROOT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"resample_bench: leg {leg} exceeded {LEG_TIMEOUT[leg]} s; stopping")
        sys.stdout.write(proc.stdout)
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr[-4000:])
            raise SystemExit(f"resample_bench: leg {leg} ended with status {proc.returncode}; stopping")
        line = [l for l in proc.stdout.splitlines() if l.startswith("RESAMPLE_BENCH_RESULT ")][-1]
        result[leg] = json.loads(line[len("RESAMPLE_BENCH_RESULT "):])
        result[leg]["leg_wall_s"] = round(time.time() - t0, 1)
    ms = {net: {route: result[net][route]["kron_ms"] for route in ROUTES} for net in NETS}
    spread = {net: max(result[net][route]["kron_ms_spread"] for route in ROUTES[:2]) for net in NETS}
    summary = {"kron_ms_per_minibatch_128": ms, "kron_ms_spread_of_the_sweep_routes": spread,
               **{f"{net}_tape_over_sweep_kernels_on": ms[net]["tape"] / ms[net]["sweep_kernels_on"] for net in NETS},
               **{f"{net}_kernels_off_over_on": ms[net]["sweep_kernels_off"] / ms[net]["sweep_kernels_on"] for net in NETS},
               "gate_1_the_sweep_is_never_slower_than_the_tape": bool(all(
                   max(ms[net]["sweep_kernels_on"], ms[net]["sweep_kernels_off"]) <= ms[net]["tape"] for net in NETS)),
               "gate_2_kernels_on_not_slower_than_off_beyond_the_spread": bool(all(
                   ms[net]["sweep_kernels_on"] <= ms[net]["sweep_kernels_off"] + spread[net] for net in NETS))}
    result["summary"] = summary
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(summary))
    if not args.rehearse and not summary["gate_1_the_sweep_is_never_slower_than_the_tape"]:
        raise SystemExit("resample_bench: GATE 1 FAILED: the sweep is slower than the autograd tape")
    if not args.rehearse and not summary["gate_2_kernels_on_not_slower_than_off_beyond_the_spread"]:
        raise SystemExit("resample_bench: GATE 2 FAILED: use_resample_kernels = True is slower than False (the switch belongs off by default)")


if __name__ == "__main__":
    main()
