"""Cost of depthwise convolutions on the NHWC split-fp16 sweep (dev tool; writes profiles/dwconv_bench.json).

  python tools/dwconv_bench.py [--out profiles/dwconv_bench.json]

Two records:
  * kernel (no gate): the nine depthwise 3 x 3 layers of distinct shape of `MobileNetV1()` on 32 x 32 inputs, S = 9 seeds,
    B = 128: the time of `lk_dwconv_bwd_nhwc_f16x2`, its minimal bytes 4 S B C (OH OW + H W) + 4 kh kw C and bytes/s, the path
    `lk_dwconv_variant` names, and the forward `lk_dwconv_fwd_nhwc_f32` (once per minibatch) - beside the library pair the NCHW
    sweep runs on the same values: `SeedBatchedSweep._conv_input_grad` (convolution_backward with `groups`) and
    `F.conv2d(groups=C)`, alternating in one process.  The cotangents rotate through enough buffers (>= 1 GiB in all) that the
    last-level cache cannot hold them from one launch to the next.
  * end to end (gate): `MobileNetV1()` at minibatch 128 - `HipGGN.diag` with everything but BatchNorm tracked, and `HipGGN.kron`
    with `freeze_depthwise=True` - `SplitSweep.nhwc_depthwise = True` against `False` (the NCHW sweep: the route of this model
    before lk_dwconv.hip), medians of alternating rounds in one process.  GATE: the depthwise route is never slower on either
    line; the class default may be `True` only while the gate passes (the file records the default it ran beside).

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

# (channels, height = width of the layer's input, stride): the depthwise 3 x 3 / padding 1 layers of MobileNetV1 on 32 x 32 inputs
DW_SHAPES = [(32, 32, 1), (64, 32, 2), (128, 16, 1), (128, 16, 2), (256, 8, 1), (256, 8, 2), (512, 4, 1), (512, 4, 2), (1024, 2, 1)]
LEGS = ("kernel", "diag", "kron")
LEG_TIMEOUT = {"kernel": 300, "diag": 300, "kron": 300}


def _setup(rehearse: bool):
    import torch

    if rehearse:
        from laplace_amd import _lib
        from tests.emulated_dwconv_kernels import EmulatedDwconvKernels

        _lib.set_kernels_for_testing(EmulatedDwconvKernels())
        return torch, "cpu"
    if not torch.cuda.is_available():
        raise SystemExit("dwconv_bench: no ROCm device (a measurement does not fall back to the CPU)")
    return torch, "cuda"


def _median(v):
    return sorted(v)[len(v) // 2]


def leg_kernel(args):
    torch, dev = _setup(args.rehearse)
    import torch.nn.functional as F

    from laplace_amd import conv as cv
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep import SeedBatchedSweep

    K = get_kernels()
    timer = _Timer(torch, dev)
    S, B = (2, 2) if args.rehearse else (9, 128)
    k, p, rows = 3, 1, []
    for C, hw, s in DW_SHAPES:
        ohw = (hw + 2 * p - k) // s + 1
        g_bytes, dx_bytes, w_bytes = 4 * S * B * C * ohw * ohw, 4 * S * B * C * hw * hw, 4 * k * k * C
        nbuf = 1 if args.rehearse else max(2, min(32, -(-(1 << 30) // (g_bytes + dx_bytes))))
        m = torch.nn.Conv2d(C, C, k, s, p, groups=C, bias=False).to(dev)
        w_tap = cv.PreparedDepthwise(m).w_tap
        xs = [torch.randn(B, hw, hw, C, device=dev) for _ in range(nbuf)]
        g32 = [torch.randn(S * B, ohw, ohw, C, device=dev) for _ in range(nbuf)]
        gs = [K.split_f16x2(g) for g in g32]  # (one scale: what every producer of the NHWC sweep hands over)
        # the NCHW sweep's operands: the same values, channels first
        xs_c = [x.permute(0, 3, 1, 2).contiguous() for x in xs]
        gs_c = [g.float().permute(0, 3, 1, 2).contiguous() for g in gs]
        del g32
        in_shape = (S * B, C, hw, hw)

        def ours(i):
            K.dwconv_backward(gs[i % nbuf], w_tap, S, (hw, hw), k, s, p)

        def stock(i):
            SeedBatchedSweep._conv_input_grad(in_shape, m, gs_c[i % nbuf])

        def fwd(i):
            K.dwconv_forward(xs[i % nbuf], w_tap, None, k, s, p)

        def stock_fwd(i):
            F.conv2d(xs_c[i % nbuf], m.weight, None, s, p, 1, C)

        with torch.no_grad():
            # the two backward passes agree on this data (nine-term fp32 sums: 1e-5 of the largest element)
            a = K.dwconv_backward(gs[0], w_tap, S, (hw, hw), k, s, p).permute(0, 3, 1, 2)
            b_ = SeedBatchedSweep._conv_input_grad(in_shape, m, gs_c[0])
            assert float((a - b_).abs().max()) <= 1e-5 * float(b_.abs().max()), (C, hw, s)
            del a, b_
            iters = 2 if args.rehearse else max(2 * nbuf, 20)
            for fn in (ours, stock, fwd, stock_fwd):
                for i in range(nbuf):
                    fn(i)
            t = {"ours": [], "stock": [], "fwd": [], "stock_fwd": []}
            for _ in range(1 if args.rehearse else 5):  # alternating rounds
                for name, fn in (("ours", ours), ("stock", stock), ("fwd", fwd), ("stock_fwd", stock_fwd)):
                    t[name].append(timer(fn, iters))
        moved = g_bytes + dx_bytes + w_bytes
        fwd_bytes = 4 * B * C * (hw * hw + ohw * ohw) + w_bytes
        med = {n: _median(v) for n, v in t.items()}
        rows.append({
            "channels": C, "hw": hw, "window": k, "stride": s, "padding": p, "S": S, "B": B, "buffers_rotated": nbuf,
            "variant": K.dwconv_variant(S, B, hw, hw, C, k, s, p, True),
            "dwconv_bwd_ms": med["ours"], "dwconv_bwd_ms_rounds": t["ours"], "dwconv_bwd_min_bytes": moved,
            "dwconv_bwd_TBps": moved / (med["ours"] * 1e-3) / 1e12,
            "stock_conv_input_grad_ms": med["stock"], "stock_conv_input_grad_ms_rounds": t["stock"],
            "dwconv_fwd_ms": med["fwd"], "dwconv_fwd_ms_rounds": t["fwd"], "dwconv_fwd_min_bytes": fwd_bytes,
            "dwconv_fwd_TBps": fwd_bytes / (med["fwd"] * 1e-3) / 1e12,
            "stock_conv2d_groups_ms": med["stock_fwd"], "stock_conv2d_groups_ms_rounds": t["stock_fwd"],
        })
        print(f"C={C:4d} {hw:2d}x{hw:<2d} stride {s}: dwconv_bwd {med['ours']:8.4f} ms ({rows[-1]['dwconv_bwd_TBps']:.2f} TB/s of its "
              f"minimal bytes)   stock input-grad {med['stock']:8.4f} ms   dwconv_fwd {med['fwd']:8.4f} ms "
              f"({rows[-1]['dwconv_fwd_TBps']:.2f} TB/s)   stock forward {med['stock_fwd']:8.4f} ms", flush=True)
        del xs, gs, xs_c, gs_c
    return {"shapes": rows}


def leg_e2e(args, what):
    """`HipGGN.diag` / `HipGGN.kron` per minibatch of 128 on MobileNetV1: `nhwc_depthwise = True` and `False`, alternating rounds
    in this process"""
    torch, dev = _setup(args.rehearse)
    from laplace_amd import HipGGN
    from laplace_amd.nets import MobileNetV1
    from laplace_amd.sweep_nhwc import SplitSweep

    torch.manual_seed(0)
    B, hw = (2, 32) if args.rehearse else (128, 32)
    model = MobileNetV1(width=0.25 if args.rehearse else 1.0, freeze_depthwise=what == "kron").to(dev).eval()
    X, y = torch.randn(B, 3, hw, hw, device=dev), torch.randint(10, (B,), device=dev)

    def step(b):
        return b.kron(X, y, N=B) if what == "kron" else b.diag(X, y)

    backends, class_default = {}, SplitSweep.nhwc_depthwise
    for route, flag in (("nhwc_depthwise_true", True), ("nhwc_depthwise_false", False)):  # (read when a backend builds its sweep)
        SplitSweep.nhwc_depthwise = flag
        try:
            b = backends[route] = HipGGN(model, "classification")
            for _ in range(1 if args.rehearse else 3):
                step(b)
        finally:
            SplitSweep.nhwc_depthwise = class_default
    timer = _Timer(torch, dev)
    rounds = {route: [] for route in backends}
    for _ in range(1 if args.rehearse else 5):  # alternating rounds
        for route, b in backends.items():
            rounds[route].append(timer(lambda i, b=b: step(b), 1 if args.rehearse else 5))
    out = {"network": "MobileNetV1", "entry_point": f"HipGGN.{what}", "input_hw": hw, "batch": B, "class_default": class_default,
           "tracked": "all but BatchNorm and the depthwise weights" if what == "kron" else "all but BatchNorm"}
    for route, b in backends.items():
        tape = b._tape()
        sweep = tape.sweeps.get(frozenset() if what == "kron" else frozenset({"gconv"}))
        assert sweep not in (None, False), getattr(tape, "sweep_reason", None)
        out[route] = {"ms": _median(rounds[route]), "ms_rounds": rounds[route], "sweep": type(sweep).__name__,
                      "split_ok": bool(getattr(sweep, "split_ok", False)), "split_reason": getattr(sweep, "split_reason", None)}
    assert out["nhwc_depthwise_true"]["split_ok"] and not out["nhwc_depthwise_false"]["split_ok"], out
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dwconv_bench.json"))
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg:  # child: one leg, result as the last line of stdout
        res = leg_kernel(args) if args.leg == "kernel" else leg_e2e(args, args.leg)
        print("DWCONV_BENCH_RESULT " + json.dumps(res), flush=True)
        return
    result = {"tool": "tools/dwconv_bench.py", "rehearsal_on_cpu_emulation_times_meaningless": bool(args.rehearse)}
    for leg in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg] + (["--rehearse"] if args.rehearse else [])
        t0 = time.time()
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT[leg], cwd=ROOT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"dwconv_bench: leg {leg} exceeded {LEG_TIMEOUT[leg]} s; stopping")
        sys.stdout.write(proc.stdout)
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr[-4000:])
            raise SystemExit(f"dwconv_bench: leg {leg} ended with status {proc.returncode}; stopping")
        line = [l for l in proc.stdout.splitlines() if l.startswith("DWCONV_BENCH_RESULT ")][-1]
        result[leg] = json.loads(line[len("DWCONV_BENCH_RESULT "):])
        result[leg]["leg_wall_s"] = round(time.time() - t0, 1)
    summary = {}
    for leg in LEGS[1:]:
        d, n = result[leg]["nhwc_depthwise_true"]["ms"], result[leg]["nhwc_depthwise_false"]["ms"]
        summary[leg] = {"ms_per_minibatch_128_nhwc_depthwise_true": d, "ms_per_minibatch_128_nhwc_depthwise_false": n, "gain": n / d,
                        "depthwise_route_not_slower": bool(d <= n)}
    summary["gate_depthwise_route_never_slower"] = all(summary[leg]["depthwise_route_not_slower"] for leg in LEGS[1:])
    summary["class_default_nhwc_depthwise"] = result[LEGS[1]]["class_default"]
    result["summary"] = summary
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(summary))
    if not args.rehearse and not summary["gate_depthwise_route_never_slower"]:
        print("dwconv_bench: GATE FAILED: the NHWC depthwise route is slower than the NCHW sweep on a line; "
              "SplitSweep.nhwc_depthwise must default to False")
        if summary["class_default_nhwc_depthwise"]:
            raise SystemExit(1)


if __name__ == "__main__":
    main()
