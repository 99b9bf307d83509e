"""Cost of squeeze-and-excitation gates on the NHWC split-fp16 sweep (dev tool; writes profiles/se_nhwc_bench.json).

  python tools/se_nhwc_bench.py [--out profiles/se_nhwc_bench.json]

Two records:
  * kernel (no gate): `lk_gate_reduce_nhwc_f32` and `lk_gate_vjp_nhwc_f32` at the three gates of `nets.SEResNetSmall()` (C = 32 at
    32 x 32, C = 64 at 16 x 16, C = 128 at 8 x 8), S = 9 seeds, B = 128, each with the cotangent as an fp32 map and as a split tensor.
    Time, the minimal bytes (g once, x / gate and r once per sample, the outputs once) and TB/s of them (the VJP with its max|dx|
    word, as the sweep calls it), and the path
    `lk_gate_variant` names.  Beside it what the NCHW route spends on the same data: `lk_mul_vjp_f32` (both outputs), the pooling
    cotangent expanded to the map, and the add of the two.  The buffers rotate so that the last-level cache cannot hold them from
    one launch to the next.
  * end to end (gates): `HipGGN.kron` per minibatch of 128 on `SEResNetSmall()` in one process, medians of alternating rounds,
    three ways: `SplitSweep.nhwc_mul = True` (the split walk), the default (the NCHW sweep) and `use_sweep = False` (the autograd
    tape).  GATE 1: no sweep is slower than the tape.  GATE 2: `nhwc_mul = True` is not slower than the default beyond the spread
    of the rounds (the larger interquartile range of the two routes' rounds, measured here).

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

LEGS = ("kernel", "se_resnet_small")
LEG_TIMEOUT = {"kernel": 240, "se_resnet_small": 360}
ROUTES = ("nhwc_mul", "default", "tape")
ROUNDS = 7


def _setup(rehearse: bool):
    import torch

    if rehearse:
        from laplace_amd import _lib
        from tests.emulated_gate_kernels import EmulatedGateKernels

        _lib.set_kernels_for_testing(EmulatedGateKernels())
        return torch, "cpu"
    if not torch.cuda.is_available():
        raise SystemExit("se_nhwc_bench: no ROCm device (a measurement does not fall back to the CPU)")
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
    shapes = [("SEResNetSmall stage 1: map [32, 32, 32]", 32, 32 // sc), ("SEResNetSmall stage 2: map [64, 16, 16]", 64, 16 // sc),
              ("SEResNetSmall stage 3: map [128, 8, 8]", 128, 8 // sc)]
    rows = []
    for what, C, hw in shapes:
        P, N = hw * hw, S * B
        g_bytes = 4 * N * P * C  # (an fp32 map and the two fp16 planes of a split tensor weigh the same)
        red_bytes = g_bytes + 4 * B * P * C + 4 * N * C
        vjp_bytes = g_bytes + 4 * B * C + 4 * N * C + 4 * N * P * C
        nbuf = 1 if args.rehearse else max(2, min(8, -(-(1 << 30) // vjp_bytes)))
        bufs = []
        for _ in range(nbuf):
            g = torch.randn(N, hw, hw, C, device=dev)
            bufs.append(dict(g=g, gs=K.split_f16x2(g), x=torch.randn(B, hw, hw, C, device=dev), gate=torch.rand(B, C, device=dev),
                             r=torch.randn(N, C, device=dev) / P, g_nchw=g.permute(0, 3, 1, 2).contiguous()))
        for b in bufs:
            b["x_nchw"] = b["x"].permute(0, 3, 1, 2).contiguous()

        def reduce_(i, form):
            b = bufs[i % nbuf]
            return K.gate_reduce(b[form], b["x"], S)

        words, word_i = torch.zeros(4096, device=dev), [0]  # (a fresh zeroed max|dx| word per launch, as the sweep hands one out)

        def vjp(i, form):
            b = bufs[i % nbuf]
            word_i[0] += 1
            assert word_i[0] < words.numel()
            return K.gate_vjp(b[form], b["gate"], b["r"], S, amax=words[word_i[0]:word_i[0] + 1])

        def nchw(i):
            b = bufs[i % nbuf]
            da, db = K.mul_vjp(b["g_nchw"], b["x_nchw"], b["gate"].reshape(B, C, 1, 1), S, True)
            return da + b["r"].reshape(N, C, 1, 1).expand(N, C, hw, hw).contiguous(), db

        if not args.rehearse:  # the routes agree on this data to fp32 accuracy
            dx, ds = vjp(0, "g"), reduce_(0, "g")
            dx0, ds0 = nchw(0)
            assert float((dx.permute(0, 3, 1, 2) - dx0).abs().max()) <= 1e-5 * float(dx0.abs().max()), what
            assert float((ds - ds0.reshape(N, C)).abs().max()) <= 1e-4 * float(ds0.abs().max()), what
        legs = {"reduce_f32": lambda i: reduce_(i, "g"), "reduce_split": lambda i: reduce_(i, "gs"), "vjp_f32": lambda i: vjp(i, "g"),
                "vjp_split": lambda i: vjp(i, "gs"), "nchw_route": nchw}
        iters = 2 if args.rehearse else max(2 * nbuf, 20)
        for fn in legs.values():
            for i in range(nbuf):
                fn(i)
        t = {name: [] for name in legs}
        for _ in range(1 if args.rehearse else 5):  # alternating rounds
            for name, fn in legs.items():
                t[name].append(timer(fn, iters))
        med = {n: _median(v) for n, v in t.items()}
        row = {"what": what, "S": S, "B": B, "P": P, "C": C, "buffers_rotated": nbuf,
               "reduce_variant": K.gate_variant(False, S, B, P, C), "vjp_variant": K.gate_variant(True, S, B, P, C),
               "reduce_min_bytes": red_bytes, "vjp_min_bytes": vjp_bytes}
        for name in legs:
            row[name + "_ms"], row[name + "_ms_rounds"] = med[name], t[name]
        for name, nbytes in (("reduce_f32", red_bytes), ("reduce_split", red_bytes), ("vjp_f32", vjp_bytes), ("vjp_split", vjp_bytes)):
            row[name + "_TBps"] = nbytes / (med[name] * 1e-3) / 1e12
        row["gate_kernels_f32_ms"] = med["reduce_f32"] + med["vjp_f32"]
        row["gate_kernels_split_ms"] = med["reduce_split"] + med["vjp_split"]
        row["nchw_route_is"] = "lk_mul_vjp_f32 (both outputs) + the expanded pooling cotangent + the add, on NCHW copies of the same data"
        rows.append(row)
        print(f"{what}: reduce {med['reduce_f32']:.4f} / {med['reduce_split']:.4f} ms ({row['reduce_f32_TBps']:.2f} / "
              f"{row['reduce_split_TBps']:.2f} TB/s)   vjp {med['vjp_f32']:.4f} / {med['vjp_split']:.4f} ms ({row['vjp_f32_TBps']:.2f} / "
              f"{row['vjp_split_TBps']:.2f} TB/s)   NCHW route {med['nchw_route']:.4f} ms", flush=True)
        del bufs
    return {"shapes": rows}


def leg_kron(args):
    """`HipGGN.kron` per minibatch of 128 on the three routes of `SEResNetSmall()`, alternating rounds in this process"""
    torch, dev = _setup(args.rehearse)
    from laplace_amd import HipGGN
    from laplace_amd.nets import SEResNetSmall
    from laplace_amd.sweep_nhwc import SplitSweep

    torch.manual_seed(0)
    B, hw = (2, 8) if args.rehearse else (128, 32)
    model = (SEResNetSmall(widths=(32, 64), depth=1) if args.rehearse else SEResNetSmall()).to(dev).eval()
    X, y = torch.randn(B, 3, hw, hw, device=dev), torch.randint(10, (B,), device=dev)
    backends = {}
    for route in ROUTES:  # (`nhwc_mul` is read when the sweep is built: in the first call of each backend)
        b = backends[route] = HipGGN(model, "classification")
        if route == "tape":
            b.use_sweep = False
        SplitSweep.nhwc_mul = route == "nhwc_mul"
        try:
            b.kron(X, y, N=B)
        finally:
            SplitSweep.nhwc_mul = False
        for _ in range(0 if args.rehearse else 2):
            b.kron(X, y, N=B)
    timer = _Timer(torch, dev)
    rounds = {route: [] for route in backends}
    for _ in range(1 if args.rehearse else ROUNDS):  # alternating rounds
        for route, b in backends.items():
            rounds[route].append(timer(lambda i, b=b: b.kron(X, y, N=B), 1 if args.rehearse else 4))
    out = {"network": "SEResNetSmall()", "input_hw": hw, "batch": B}
    for route, b in backends.items():
        sweep = getattr(b._tape(), "sweep", None)
        out[route] = {"kron_ms": _median(rounds[route]), "kron_ms_rounds": rounds[route], "kron_ms_iqr": _iqr(rounds[route]),
                      "sweep": type(sweep).__name__ if sweep not in (None, False) else None,
                      "sweep_reason": getattr(b._tape(), "sweep_reason", None),
                      "split_ok": bool(getattr(sweep, "split_ok", False)), "split_reason": getattr(sweep, "split_reason", None)}
    assert out["nhwc_mul"]["split_ok"] and not out["nhwc_mul"]["sweep_reason"], out
    assert out["default"]["sweep"] is not None and not out["default"]["split_ok"] and not out["default"]["sweep_reason"], out
    assert out["default"]["split_reason"] == "mul has no NHWC rule" and out["tape"]["sweep"] is None, out
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "se_nhwc_bench.json"))
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg:  # child: one leg, result as the last line of stdout
        res = leg_kernel(args) if args.leg == "kernel" else leg_kron(args)
        print("SE_NHWC_BENCH_RESULT " + json.dumps(res), flush=True)
        return
    result = {"tool": "tools/se_nhwc_bench.py", "rehearsal_on_cpu_emulation_times_meaningless": bool(args.rehearse)}
    for leg in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg] + (["--rehearse"] if args.rehearse else [])
        t0 = time.time()
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT[leg], cwd=ROOT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"se_nhwc_bench: leg {leg} exceeded {LEG_TIMEOUT[leg]} s; stopping")
        sys.stdout.write(proc.stdout)
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr[-4000:])
            raise SystemExit(f"se_nhwc_bench: leg {leg} ended with status {proc.returncode}; stopping")
        line = [l for l in proc.stdout.splitlines() if l.startswith("SE_NHWC_BENCH_RESULT ")][-1]
        result[leg] = json.loads(line[len("SE_NHWC_BENCH_RESULT "):])
        result[leg]["leg_wall_s"] = round(time.time() - t0, 1)
    e2e = result["se_resnet_small"]
    ms = {route: e2e[route]["kron_ms"] for route in ROUTES}
    spread = max(e2e[route]["kron_ms_iqr"] for route in ("nhwc_mul", "default"))
    summary = {"kron_ms_per_minibatch_128": ms, "spread_ms_larger_iqr_of_nhwc_mul_and_default_rounds": spread,
               "tape_over_nhwc_mul": ms["tape"] / ms["nhwc_mul"], "default_over_nhwc_mul": ms["default"] / ms["nhwc_mul"],
               "gate_1_no_sweep_slower_than_the_tape": max(ms["nhwc_mul"], ms["default"]) <= ms["tape"],
               "gate_2_nhwc_mul_not_slower_than_the_default_beyond_the_spread": ms["nhwc_mul"] <= ms["default"] + spread}
    result["summary"] = summary
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(summary))
    if not args.rehearse and not summary["gate_1_no_sweep_slower_than_the_tape"]:
        raise SystemExit("se_nhwc_bench: GATE 1 FAILED: a sweep is slower than the autograd tape")
    if not args.rehearse and not summary["gate_2_nhwc_mul_not_slower_than_the_default_beyond_the_spread"]:
        raise SystemExit("se_nhwc_bench: GATE 2 FAILED: nhwc_mul = True is slower than the default (the switch stays opt-in)")


if __name__ == "__main__":
    main()
