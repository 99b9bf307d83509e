"""Cost of static slicing (chunk / split / indexing) on the two reverse sweeps (dev tool; writes profiles/slice_bench.json).

  python tools/slice_bench.py [--out profiles/slice_bench.json]

Three records:
  * kernel (no gate): `lk_slice_vjp_f32` beside the torch sequence it replaces (a zero fill of the full-width tensor, a
    `narrow(...).add_` per piece, and - on the NHWC walk - a `.float()` per split piece and a max|.| pass), S = 9 seeds, B = 128, at
    the largest chunk of `nets.CSPNetSmall()` (64 channels at 32 x 32 in two halves: the pieces the walk hands over - a split
    tensor and an fp32 map over one half, an fp32 map over the other) and at the packed-qkv shape of `nets.ViTClassToken()` (rows of
    3 x 192 columns in three fp32 pieces, T = 65).  Time, the minimal bytes (4 R Ct written plus every piece read once) and
    bytes/s of them, and the path `lk_slice_variant` names.  The buffers rotate so that the last-level cache cannot hold them
    from one launch to the next.
  * end to end (gates): `HipGGN.kron` per minibatch of 128 in one process per network, medians of alternating rounds.
    `nets.CSPNetSmall()`: the split sweep (`nhwc_slice = True`), the NCHW sweep (`nhwc_slice = False`) with
    `use_slice_kernels` on and off, and `use_sweep = False` (the autograd tape: the route of this model before the rules).
    `nets.ViTClassToken()`: the NCHW walk (its attention node keeps it there) with `use_slice_kernels` on and off, and the tape.
    GATE 1: no sweep is slower than the tape.  GATE 2: `use_slice_kernels = True` is not slower than `False`.

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

LEGS = ("kernel", "cspnet_small", "vit_class_token")
LEG_TIMEOUT = {"kernel": 240, "cspnet_small": 420, "vit_class_token": 420}
ROUTES = {"cspnet_small": ("split_sweep", "nchw_kernels_on", "nchw_kernels_off", "tape"),
          "vit_class_token": ("nchw_kernels_on", "nchw_kernels_off", "tape")}


def _setup(rehearse: bool):
    import torch

    if rehearse:
        from laplace_amd import _lib
        from tests.emulated_slice_kernels import EmulatedSliceKernels

        _lib.set_kernels_for_testing(EmulatedSliceKernels())
        return torch, "cpu"
    if not torch.cuda.is_available():
        raise SystemExit("slice_bench: no ROCm device (a measurement does not fall back to the CPU)")
    return torch, "cuda"


def _median(v):
    return sorted(v)[len(v) // 2]


def leg_kernel(args):
    torch, dev = _setup(args.rehearse)
    from laplace_amd._lib import SplitTensor, get_kernels

    K = get_kernels()
    timer = _Timer(torch, dev)
    S, B = (2, 2) if args.rehearse else (9, 128)
    # (what, rows per sample, Ct, pieces (kind, c0, cs), whether the walk wants max|.|)
    shapes = [("CSPNetSmall stage 1: x.chunk(2, 1) of 64 channels at 32 x 32", 4 * 4 if args.rehearse else 32 * 32, 64,
               (("split", 32, 32), ("f32", 32, 32), ("f32", 0, 32)), True),
              ("ViTClassToken: qkv.split(192, dim=2), T = 65", 5 if args.rehearse else 65, 576,
               (("f32", 384, 192), ("f32", 192, 192), ("f32", 0, 192)), False)]
    rows = []
    for what, per_sample, Ct, pieces, want_amax in shapes:
        R = S * B * per_sample
        piece_bytes = sum(4 * R * cs for _, _, cs in pieces)  # (the two planes of a split piece take as much as an fp32 map)
        nbuf = 1 if args.rehearse else max(2, min(8, -(-(1 << 30) // (4 * R * Ct + piece_bytes))))

        def make(kind, cs):
            t = torch.randn(R, cs, device=dev)
            return K.split_f16x2(t) if kind == "split" else t

        bufs = [[(make(kind, cs), c0, cs) for kind, c0, cs in pieces] for _ in range(nbuf)]
        word = torch.zeros(1, device=dev)

        def ours(i):
            K.slice_vjp(bufs[i % nbuf], R, Ct, amax=word if want_amax else None)

        def stock(i):
            out = torch.zeros(R, Ct, device=dev)
            for p, c0, cs in bufs[i % nbuf]:
                out.narrow(1, c0, cs).add_(p.float() if isinstance(p, SplitTensor) else p)
            if want_amax:
                K.absmax(out)
            return out

        if not args.rehearse:  # the two routes agree on this data bit for bit (the same sums in the same order, 0 + v = v)
            assert torch.equal(K.slice_vjp(bufs[0], R, Ct), stock(0)), what
        iters = 2 if args.rehearse else max(2 * nbuf, 20)
        for fn in (ours, stock):
            for i in range(nbuf):
                fn(i)
        t = {"ours": [], "stock": []}
        for _ in range(1 if args.rehearse else 5):  # alternating rounds
            for name, fn in (("ours", ours), ("stock", stock)):
                t[name].append(timer(fn, iters))
        moved = 4 * R * Ct + piece_bytes
        med = {n: _median(v) for n, v in t.items()}
        mask = sum(1 << i for i, (kind, _, _) in enumerate(pieces) if kind == "split")
        rows.append({
            "what": what, "R": R, "Ct": Ct, "pieces": [list(p) for p in pieces], "S": S, "B": B, "amax": want_amax,
            "buffers_rotated": nbuf, "variant": K.slice_variant(mask, [p[1] for p in pieces], [p[2] for p in pieces], R, Ct, True),
            "slice_vjp_ms": med["ours"], "slice_vjp_ms_rounds": t["ours"], "slice_vjp_min_bytes": moved,
            "slice_vjp_TBps": moved / (med["ours"] * 1e-3) / 1e12,
            "torch_zeros_narrow_add_ms": med["stock"], "torch_zeros_narrow_add_ms_rounds": t["stock"],
        })
        print(f"{what}: slice_vjp {med['ours']:8.4f} ms ({rows[-1]['slice_vjp_TBps']:.2f} TB/s of its minimal bytes)   "
              f"torch sequence {med['stock']:8.4f} ms", flush=True)
        del bufs
    return {"shapes": rows}


def leg_kron(args, net):
    """`HipGGN.kron` per minibatch of 128 on the routes of `net`, alternating rounds in this process"""
    torch, dev = _setup(args.rehearse)
    from laplace_amd import HipGGN
    from laplace_amd.nets import CSPNetSmall, ViTClassToken
    from laplace_amd.sweep_nhwc import SplitSweep

    torch.manual_seed(0)
    B, hw = (2, 8) if args.rehearse else (128, 32)
    if net == "cspnet_small":
        model, name = (CSPNetSmall(widths=(64, 64), depth=1) if args.rehearse else CSPNetSmall()), "CSPNetSmall()"
    else:
        model, name = (ViTClassToken(image=8, dim=32, depth=1, heads=2) if args.rehearse else ViTClassToken()), "ViTClassToken()"
    model = model.to(dev).eval()
    X, y = torch.randn(B, 3, hw, hw, device=dev), torch.randint(10, (B,), device=dev)
    backends, default = {}, SplitSweep.nhwc_slice
    for route in ROUTES[net]:  # (`nhwc_slice` is read when a backend builds its sweep; `use_slice_kernels` in every reverse sweep)
        SplitSweep.nhwc_slice = route == "split_sweep"
        try:
            b = backends[route] = HipGGN(model, "classification")
            if route == "tape":
                b.use_sweep = False
            b.kron(X, y, N=B)
            sweep = getattr(b._tape(), "sweep", None)
            if sweep not in (None, False):
                sweep.use_slice_kernels = route != "nchw_kernels_off"
            for _ in range(0 if args.rehearse else 2):
                b.kron(X, y, N=B)
        finally:
            SplitSweep.nhwc_slice = default
    timer = _Timer(torch, dev)
    rounds = {route: [] for route in backends}
    for _ in range(1 if args.rehearse else 5):  # alternating rounds
        for route, b in backends.items():
            rounds[route].append(timer(lambda i, b=b: b.kron(X, y, N=B), 1 if args.rehearse else 4))
    out = {"network": name, "input_hw": hw, "batch": B, "nhwc_slice_default_of_this_build": bool(default)}
    for route, b in backends.items():
        sweep = getattr(b._tape(), "sweep", None)
        out[route] = {"kron_ms": _median(rounds[route]), "kron_ms_rounds": rounds[route],
                      "sweep": type(sweep).__name__ if sweep not in (None, False) else None,
                      "sweep_reason": getattr(b._tape(), "sweep_reason", None),
                      "split_ok": bool(getattr(sweep, "split_ok", False)), "split_reason": getattr(sweep, "split_reason", None),
                      "use_slice_kernels": bool(getattr(sweep, "use_slice_kernels", False))}
    if net == "cspnet_small":
        assert out["split_sweep"]["split_ok"] and not out["split_sweep"]["sweep_reason"], out
    for route in ("nchw_kernels_on", "nchw_kernels_off"):
        assert out[route]["sweep"] is not None and not out[route]["split_ok"] and not out[route]["sweep_reason"], out
    assert out["tape"]["sweep"] is None, out
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slice_bench.json"))
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg:  # child: one leg, result as the last line of stdout
        res = leg_kernel(args) if args.leg == "kernel" else leg_kron(args, args.leg)
        print("SLICE_BENCH_RESULT " + json.dumps(res), flush=True)
        return
    result = {"tool": "tools/slice_bench.py", "rehearsal_on_cpu_emulation_times_meaningless": bool(args.rehearse)}
    for leg in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg] + (["--rehearse"] if args.rehearse else [])
        t0 = time.time()
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT[leg], cwd=ROOT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"slice_bench: leg {leg} exceeded {LEG_TIMEOUT[leg]} s; stopping")
        sys.stdout.write(proc.stdout)
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr[-4000:])
            raise SystemExit(f"slice_bench: leg {leg} ended with status {proc.returncode}; stopping")
        line = [l for l in proc.stdout.splitlines() if l.startswith("SLICE_BENCH_RESULT ")][-1]
        result[leg] = json.loads(line[len("SLICE_BENCH_RESULT "):])
        result[leg]["leg_wall_s"] = round(time.time() - t0, 1)
    ms = {net: {route: result[net][route]["kron_ms"] for route in ROUTES[net]} for net in ROUTES}
    csp, vit = ms["cspnet_small"], ms["vit_class_token"]
    summary = {"kron_ms_per_minibatch_128": ms,
               "cspnet_tape_over_split_sweep": csp["tape"] / csp["split_sweep"],
               "cspnet_tape_over_nchw_kernels_on": csp["tape"] / csp["nchw_kernels_on"],
               "cspnet_nchw_kernels_on_over_split_sweep": csp["nchw_kernels_on"] / csp["split_sweep"],
               "cspnet_nchw_kernels_off_over_on": csp["nchw_kernels_off"] / csp["nchw_kernels_on"],
               "vit_tape_over_nchw_kernels_on": vit["tape"] / vit["nchw_kernels_on"],
               "vit_nchw_kernels_off_over_on": vit["nchw_kernels_off"] / vit["nchw_kernels_on"],
               "gate_1_no_sweep_slower_than_the_tape": bool(csp["split_sweep"] <= csp["tape"] and csp["nchw_kernels_on"] <= csp["tape"]
                                                            and vit["nchw_kernels_on"] <= vit["tape"]),
               "gate_2_kernels_on_not_slower_than_kernels_off": bool(csp["nchw_kernels_on"] <= csp["nchw_kernels_off"]
                                                                     and vit["nchw_kernels_on"] <= vit["nchw_kernels_off"])}
    result["summary"] = summary
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(summary))
    if not args.rehearse and not summary["gate_1_no_sweep_slower_than_the_tape"]:
        raise SystemExit("slice_bench: GATE 1 FAILED: a sweep is slower than the autograd tape (nhwc_slice belongs off by default "
                         "where it is the split sweep that loses)")
    if not args.rehearse and not summary["gate_2_kernels_on_not_slower_than_kernels_off"]:
        raise SystemExit("slice_bench: GATE 2 FAILED: use_slice_kernels = True is slower than False (the switch belongs off by default)")


if __name__ == "__main__":
    main()
