"""Cost of channel concatenation on the two reverse sweeps (dev tool; writes profiles/cat_bench.json).

  python tools/cat_bench.py [--out profiles/cat_bench.json]

Two records:
  * kernel (no gate): the last concatenation of each dense block of `nets.DenseNetSmall()` - [x, new] with 32 new channels into
    192 channels at 32 x 32, 224 at 16 x 16 and 224 at 8 x 8 -, S = 9 seeds, B = 128.  `lk_cat_vjp_nhwc_f32` for both sources
    (two launches) on the parts the walk hands it - an fp32 map and a split tensor - beside the torch sequence it replaces: a
    `.float()` of the split part, the sum, a `narrow().contiguous()` per source and a max|.| pass per source; and
    `lk_cat_fwd_nhwc_f32` (one launch per source, once per minibatch) beside `torch.cat`.  Time, the minimal bytes
    R Cs (4 + 4 n_f32 + 4 n_split) summed over the sources (forward: 8 R Ct) and bytes/s of them, and the path `lk_cat_variant`
    names.  The buffers rotate so that the last-level cache cannot hold them from one launch to the next.
  * end to end (gates): `HipGGN.kron` on `nets.DenseNetSmall()` per minibatch of 128 on three routes in one process, medians of
    alternating rounds: the split sweep (`nhwc_cat = True`), `nhwc_cat = False` (the NCHW sweep with its CAT rule) and
    `use_sweep = False` (the autograd tape: the route of this model before the rule).  GATE 1: neither sweep is slower than the
    tape.  GATE 2: the split sweep is not slower than `nhwc_cat = False`.

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

# (what, channels of the concatenation, new channels, height = width)
CAT_SHAPES = [("block 1, layer 4", 192, 32, 32), ("block 2, layer 4", 224, 32, 16), ("block 3, layer 4", 224, 32, 8)]
LEGS = ("kernel", "densenet_small")
LEG_TIMEOUT = {"kernel": 240, "densenet_small": 420}
ROUTES = ("split_sweep", "nhwc_cat_false", "tape")


def _setup(rehearse: bool):
    import torch

    if rehearse:
        from laplace_amd import _lib
        from tests.emulated_cat_kernels import EmulatedCatKernels

        _lib.set_kernels_for_testing(EmulatedCatKernels())
        return torch, "cpu"
    if not torch.cuda.is_available():
        raise SystemExit("cat_bench: no ROCm device (a measurement does not fall back to the CPU)")
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
    for what, Ct, new, hw in CAT_SHAPES:
        if args.rehearse:
            hw = 4
        N, R, widths = S * B, S * B * hw * hw, (Ct - new, new)
        part_bytes = 4 * R * Ct  # (an fp32 map; the two planes of a split tensor take as much)
        nbuf = 1 if args.rehearse else max(2, min(8, -(-(1 << 30) // (2 * part_bytes))))
        f32s = [torch.randn(N, hw, hw, Ct, device=dev) for _ in range(nbuf)]
        splits = [K.split_f16x2(torch.randn(N, hw, hw, Ct, device=dev)) for _ in range(nbuf)]
        xs = [[torch.randn(B, hw, hw, w, device=dev) for w in widths] for _ in range(nbuf)]
        words = torch.zeros(2, device=dev)

        def ours(i):
            at = 0
            for j, w in enumerate(widths):
                K.cat_vjp([f32s[i % nbuf], splits[i % nbuf]], at, w, amax=words[j:j + 1])
                at += w

        def stock(i):
            g, at = f32s[i % nbuf] + splits[i % nbuf].float(), 0
            for w in widths:
                K.absmax(g.narrow(3, at, w).contiguous())
                at += w

        def fwd(i):
            K.cat_forward(xs[i % nbuf])

        def stock_fwd(i):
            torch.cat(xs[i % nbuf], 3)

        if not args.rehearse:  # the two routes agree on this data bit for bit (the same sum in the same order)
            a = K.cat_vjp([f32s[0], splits[0]], 0, widths[0])
            assert torch.equal(a, (f32s[0] + splits[0].float()).narrow(3, 0, widths[0])), what
            assert torch.equal(K.cat_forward(xs[0]), torch.cat(xs[0], 3)), what
            del a
        iters = 2 if args.rehearse else max(2 * nbuf, 20)
        for fn in (ours, stock, fwd, stock_fwd):
            for i in range(nbuf):
                fn(i)
        t = {"ours": [], "stock": [], "fwd": [], "stock_fwd": []}
        for _ in range(1 if args.rehearse else 5):  # alternating rounds
            for name, fn in (("ours", ours), ("stock", stock), ("fwd", fwd), ("stock_fwd", stock_fwd)):
                t[name].append(timer(fn, iters))
        moved = R * Ct * (4 + 4 + 4)  # both sources: every dst element once, the slice of an fp32 and of a split part
        fwd_bytes = 8 * B * hw * hw * Ct
        med = {n: _median(v) for n, v in t.items()}
        rows.append({
            "what": what, "Ct": Ct, "new_channels": new, "hw": hw, "S": S, "B": B, "parts": ["f32", "split"], "buffers_rotated": nbuf,
            "variant": [K.cat_variant(2, 2, R, Ct, c0, w, True) for c0, w in ((0, widths[0]), (widths[0], widths[1]))],
            "cat_vjp_ms": med["ours"], "cat_vjp_ms_rounds": t["ours"], "cat_vjp_min_bytes": moved,
            "cat_vjp_TBps": moved / (med["ours"] * 1e-3) / 1e12,
            "torch_float_sum_narrow_absmax_ms": med["stock"], "torch_float_sum_narrow_absmax_ms_rounds": t["stock"],
            "cat_fwd_ms": med["fwd"], "cat_fwd_ms_rounds": t["fwd"], "cat_fwd_min_bytes": fwd_bytes,
            "cat_fwd_TBps": fwd_bytes / (med["fwd"] * 1e-3) / 1e12,
            "torch_cat_ms": med["stock_fwd"], "torch_cat_ms_rounds": t["stock_fwd"],
        })
        print(f"{what:18s} Ct={Ct:3d} {hw:2d}x{hw:<2d}: cat_vjp {med['ours']:8.4f} ms ({rows[-1]['cat_vjp_TBps']:.2f} TB/s of its "
              f"minimal bytes)   torch sequence {med['stock']:8.4f} ms   cat_fwd {med['fwd']:8.4f} ms "
              f"({rows[-1]['cat_fwd_TBps']:.2f} TB/s)   torch.cat {med['stock_fwd']:8.4f} ms", flush=True)
        del f32s, splits, xs
    return {"shapes": rows}


def leg_kron(args, net):
    """`HipGGN.kron` per minibatch of 128 on the three routes, alternating rounds in this process"""
    torch, dev = _setup(args.rehearse)
    from laplace_amd import HipGGN
    from laplace_amd.nets import DenseNetSmall
    from laplace_amd.sweep_nhwc import SplitSweep

    torch.manual_seed(0)
    B, hw = (2, 8) if args.rehearse else (128, 32)
    model = (DenseNetSmall(blocks=(1, 1)) if args.rehearse else DenseNetSmall()).to(dev).eval()
    X, y = torch.randn(B, 3, hw, hw, device=dev), torch.randint(10, (B,), device=dev)
    backends, default = {}, SplitSweep.nhwc_cat
    for route in ROUTES:  # (the switch is read when a backend builds its sweep)
        SplitSweep.nhwc_cat = route == "split_sweep"
        try:
            b = backends[route] = HipGGN(model, "classification")
            if route == "tape":
                b.use_sweep = False
            for _ in range(1 if args.rehearse else 3):
                b.kron(X, y, N=B)
        finally:
            SplitSweep.nhwc_cat = default
    timer = _Timer(torch, dev)
    rounds = {route: [] for route in backends}
    for _ in range(1 if args.rehearse else 5):  # alternating rounds
        for route, b in backends.items():
            rounds[route].append(timer(lambda i, b=b: b.kron(X, y, N=B), 1 if args.rehearse else 4))
    out = {"network": "DenseNetSmall()", "input_hw": hw, "batch": B, "nhwc_cat_default_of_this_build": bool(default)}
    for route, b in backends.items():
        sweep = getattr(b._tape(), "sweep", None)
        out[route] = {"kron_ms": _median(rounds[route]), "kron_ms_rounds": rounds[route],
                      "sweep": type(sweep).__name__ if sweep not in (None, False) else None,
                      "sweep_reason": getattr(b._tape(), "sweep_reason", None),
                      "split_ok": bool(getattr(sweep, "split_ok", False)), "split_reason": getattr(sweep, "split_reason", None)}
    assert out["split_sweep"]["split_ok"] and not out["split_sweep"]["sweep_reason"], out
    assert out["nhwc_cat_false"]["sweep"] is not None and not out["nhwc_cat_false"]["split_ok"], out
    assert out["tape"]["sweep"] is None, out
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cat_bench.json"))
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg:  # child: one leg, result as the last line of stdout
        res = leg_kernel(args) if args.leg == "kernel" else leg_kron(args, args.leg)
        print("CAT_BENCH_RESULT " + json.dumps(res), flush=True)
        return
    result = {"tool": "tools/cat_bench.py", "rehearsal_on_cpu_emulation_times_meaningless": bool(args.rehearse)}
    for leg in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg] + (["--rehearse"] if args.rehearse else [])
        t0 = time.time()
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT[leg], cwd=ROOT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"cat_bench: leg {leg} exceeded {LEG_TIMEOUT[leg]} s; stopping")
        sys.stdout.write(proc.stdout)
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr[-4000:])
            raise SystemExit(f"cat_bench: leg {leg} ended with status {proc.returncode}; stopping")
        line = [l for l in proc.stdout.splitlines() if l.startswith("CAT_BENCH_RESULT ")][-1]
        result[leg] = json.loads(line[len("CAT_BENCH_RESULT "):])
        result[leg]["leg_wall_s"] = round(time.time() - t0, 1)
    ms = {route: result["densenet_small"][route]["kron_ms"] for route in ROUTES}
    summary = {"kron_ms_per_minibatch_128": ms,
               "tape_over_split_sweep": ms["tape"] / ms["split_sweep"], "tape_over_nhwc_cat_false": ms["tape"] / ms["nhwc_cat_false"],
               "nhwc_cat_false_over_split_sweep": ms["nhwc_cat_false"] / ms["split_sweep"],
               "gate_1_neither_sweep_slower_than_the_tape": bool(ms["split_sweep"] <= ms["tape"] and ms["nhwc_cat_false"] <= ms["tape"]),
               "gate_2_split_sweep_not_slower_than_nhwc_cat_false": bool(ms["split_sweep"] <= ms["nhwc_cat_false"])}
    result["summary"] = summary
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(summary))
    if not args.rehearse and not summary["gate_1_neither_sweep_slower_than_the_tape"]:
        raise SystemExit("cat_bench: GATE 1 FAILED: a sweep is slower than the autograd tape")
    if not args.rehearse and not summary["gate_2_split_sweep_not_slower_than_nhwc_cat_false"]:
        raise SystemExit("cat_bench: GATE 2 FAILED: the split sweep is slower than nhwc_cat = False (the switch belongs off by default)")


if __name__ == "__main__":
    main()
