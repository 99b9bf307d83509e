"""Cost of tracked BatchNorm / GroupNorm parameters on the NHWC split-fp16 sweep (dev tool; writes profiles/norm_tap_bench.json).

  python tools/norm_tap_bench.py [--out profiles/norm_tap_bench.json]

Two records, both gated:
  * kernel: the four ResNet-18 stage shapes (64 ch 32 x 32, 128 ch 16 x 16, 256 ch 8 x 8, 512 ch 4 x 4), S = 9 seeds, B = 128: the
    time of `lk_jac_norm_affine_nhwc_f16x2`, its byte floor 4 S B L Ch + 4 B L Ch + 8 B S Ch and bytes/s, the path
    `lk_normtap_variant` names - beside the route it replaces on the same values: `SplitTensor.float()`, the permute to NCHW,
    forming `xhat` from the tapped input and the running statistics, and `lk_jac_norm_affine_f32` in layout 0 (priced against ITS
    floor, 4 S B L Ch + 4 B L Ch + 8 B S Ch of fp32 operands).  Alternating in one process; the cotangents rotate through enough
    buffers (>= 1 GiB in all) that the last-level cache cannot hold them from one launch to the next.
  * end to end: `HipGGN.diag` (minibatch 128) and `HipGGN.jacobians` (minibatch 32: the dense Jacobian of 128 samples is 57 GB) on
    `nets.ResNet18(freeze_bn=False)`, and `HipGGN.diag` (minibatch 128) on `ResNet18(norm="gn")` with the affine parameters tracked -
    `nhwc_norm_taps = True` against `False` (the NCHW sweep: the route of these models before lk_normtap.hip), medians of
    alternating rounds in one process.
GATE: the switch on is slower on none of these lines.  The file records the verdict and the class default it ran beside.

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

STAGES = [(64, 32), (128, 16), (256, 8), (512, 4)]  # (channels, height = width) of the ResNet-18 stages on 32 x 32 inputs
E2E = {"diag_bn": ("bn", "diag", 128), "jacobians_bn": ("bn", "jacobians", 32), "diag_gn": ("gn", "diag", 128)}
LEGS = ("kernel",) + tuple(E2E)
LEG_TIMEOUT = 300


def _setup(rehearse: bool):
    import torch

    if rehearse:
        from laplace_amd import _lib
        from tests.emulated_normtap_kernels import EmulatedNormtapKernels

        _lib.set_kernels_for_testing(EmulatedNormtapKernels())
        return torch, "cpu"
    if not torch.cuda.is_available():
        raise SystemExit("norm_tap_bench: no ROCm device (a measurement does not fall back to the CPU)")
    return torch, "cuda"


def _median(v):
    return sorted(v)[len(v) // 2]


def leg_kernel(args):
    torch, dev = _setup(args.rehearse)
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    timer = _Timer(torch, dev)
    S, B = (2, 2) if args.rehearse else (9, 128)
    rows = []
    for Ch, hw in STAGES:
        L = hw * hw
        floor = 4 * S * B * L * Ch + 4 * B * L * Ch + 8 * B * S * Ch
        nbuf = 1 if args.rehearse else max(2, min(32, -(-(1 << 30) // (4 * S * B * L * Ch))))
        x = torch.randn(B, hw, hw, Ch, device=dev) * 2.0 + 0.5
        mu, var = torch.randn(Ch, device=dev) * 0.5, torch.rand(Ch, device=dev) + 0.5
        eps = 1e-5
        gs = [K.split_f16x2(torch.randn(S * B, hw, hw, Ch, device=dev)) for _ in range(nbuf)]
        Js = torch.zeros(B, S, 2 * Ch, dtype=torch.float32, device=dev)
        a_nchw = x.permute(0, 3, 1, 2)  # the tap's input as the forward leaves it: NCHW-logical over NHWC memory

        def ours(i):
            K.jac_norm_affine_nhwc(gs[i % nbuf], x, mu, torch.rsqrt(var + eps), S, Js, 0, Ch)

        def replaced(i):
            g = gs[i % nbuf].float().reshape(S, B, hw, hw, Ch).permute(0, 1, 4, 2, 3).contiguous()
            xhat = ((a_nchw - mu.reshape(1, -1, 1, 1)) * torch.rsqrt(var + eps).reshape(1, -1, 1, 1)).contiguous()
            K.jac_norm_affine(g, xhat, Ch, 0, Js, 0, Ch)

        with torch.no_grad():
            ours(0)
            a = Js.clone()
            replaced(0)
            assert float((a - Js).abs().max()) <= 1e-4 * float(Js.abs().max()), (Ch, hw)  # (the two routes agree on this data)
            iters = 2 if args.rehearse else max(2 * nbuf, 20)
            for fn in (ours, replaced):
                for i in range(nbuf):
                    fn(i)
            t = {"ours": [], "replaced": []}
            for _ in range(1 if args.rehearse else 5):  # alternating rounds
                for name, fn in (("ours", ours), ("replaced", replaced)):
                    t[name].append(timer(fn, iters))
        med = {n: _median(v) for n, v in t.items()}
        rows.append({
            "channels": Ch, "hw": hw, "S": S, "B": B, "buffers_rotated": nbuf, "byte_floor": floor,
            "variant": K.normtap_variant(S, B, L, Ch, True, True),
            "normtap_ms": med["ours"], "normtap_ms_rounds": t["ours"], "normtap_TBps": floor / (med["ours"] * 1e-3) / 1e12,
            "replaced_route_ms": med["replaced"], "replaced_route_ms_rounds": t["replaced"],
            "replaced_route_TBps": floor / (med["replaced"] * 1e-3) / 1e12,
            "not_slower": bool(med["ours"] <= med["replaced"]),
        })
        print(f"Ch={Ch:4d} {hw:2d}x{hw:<2d}: normtap {med['ours']:8.4f} ms ({rows[-1]['normtap_TBps']:.2f} TB/s of its byte floor)   "
              f"float + permute + xhat + layout 0 {med['replaced']:8.4f} ms ({rows[-1]['replaced_route_TBps']:.2f} TB/s)", flush=True)
        del gs
    return {"shapes": rows}


def leg_e2e(args, leg):
    """one entry point per minibatch on ResNet-18 with tracked norm parameters: `nhwc_norm_taps = True` and `False`, alternating
    rounds in this process"""
    torch, dev = _setup(args.rehearse)
    from laplace_amd import HipGGN
    from laplace_amd.nets import ResNet18

    norm, what, B = E2E[leg]
    torch.manual_seed(0)
    B, hw = (2, 8) if args.rehearse else (B, 32)
    model = ResNet18(freeze_bn=False, norm=norm).to(dev).eval()
    X, y = torch.randn(B, 3, hw, hw, device=dev), torch.randint(10, (B,), device=dev)

    def step(b):
        return b.diag(X, y) if what == "diag" else b.jacobians(X)

    backends = {}
    for route, flag in (("nhwc_norm_taps_true", True), ("nhwc_norm_taps_false", False)):
        b = backends[route] = HipGGN(model, "classification")
        b.nhwc_norm_taps = flag  # (read when the backend builds its sweep)
        for _ in range(1 if args.rehearse else 3):
            step(b)
    timer = _Timer(torch, dev)
    rounds = {route: [] for route in backends}
    for _ in range(1 if args.rehearse else 5):  # alternating rounds
        for route, b in backends.items():
            rounds[route].append(timer(lambda i, b=b: step(b), 1 if args.rehearse else 3))
    out = {"network": f"ResNet18(freeze_bn=False, norm={norm!r})", "entry_point": f"HipGGN.{what}", "input_hw": hw, "batch": B,
           "class_default": HipGGN.nhwc_norm_taps}
    for route, b in backends.items():
        tape = b._tape()
        sweep = tape.sweeps.get(frozenset({"norm"}))
        assert sweep not in (None, False), getattr(tape, "sweep_reason", None)
        out[route] = {"ms": _median(rounds[route]), "ms_rounds": rounds[route], "sweep": type(sweep).__name__,
                      "split_ok": bool(getattr(sweep, "split_ok", False)), "split_reason": getattr(sweep, "split_reason", None)}
    assert out["nhwc_norm_taps_true"]["split_ok"] and not out["nhwc_norm_taps_false"]["split_ok"], out
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "norm_tap_bench.json"))
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg:  # child: one leg, result as the last line of stdout
        res = leg_kernel(args) if args.leg == "kernel" else leg_e2e(args, args.leg)
        print("NORM_TAP_BENCH_RESULT " + json.dumps(res), flush=True)
        return
    result = {"tool": "tools/norm_tap_bench.py", "rehearsal_on_cpu_emulation_times_meaningless": bool(args.rehearse)}
    for leg in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg] + (["--rehearse"] if args.rehearse else [])
        t0 = time.time()
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT, cwd=ROOT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"norm_tap_bench: leg {leg} exceeded {LEG_TIMEOUT} s; stopping")
        sys.stdout.write(proc.stdout)
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr[-4000:])
            raise SystemExit(f"norm_tap_bench: leg {leg} ended with status {proc.returncode}; stopping")
        line = [l for l in proc.stdout.splitlines() if l.startswith("NORM_TAP_BENCH_RESULT ")][-1]
        result[leg] = json.loads(line[len("NORM_TAP_BENCH_RESULT "):])
        result[leg]["leg_wall_s"] = round(time.time() - t0, 1)
    summary = {"kernel_not_slower_on_every_shape": all(r["not_slower"] for r in result["kernel"]["shapes"])}
    for leg in E2E:
        on, off = result[leg]["nhwc_norm_taps_true"]["ms"], result[leg]["nhwc_norm_taps_false"]["ms"]
        summary[leg] = {"ms_per_minibatch_nhwc_norm_taps_true": on, "ms_per_minibatch_nhwc_norm_taps_false": off,
                        "batch": result[leg]["batch"], "gain": off / on, "switch_on_not_slower": bool(on <= off)}
    summary["gate_switch_on_never_slower"] = bool(summary["kernel_not_slower_on_every_shape"]
                                                  and all(summary[leg]["switch_on_not_slower"] for leg in E2E))
    summary["class_default_nhwc_norm_taps"] = result["diag_bn"]["class_default"]
    result["summary"] = summary
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(summary))
    if not args.rehearse and not summary["gate_switch_on_never_slower"]:
        print("norm_tap_bench: GATE FAILED: the switch on is slower than the NCHW sweep on a line; nhwc_norm_taps must default to False")
        if summary["class_default_nhwc_norm_taps"]:
            raise SystemExit(1)


if __name__ == "__main__":
    main()
