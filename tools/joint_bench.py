"""`la(X, joint=True)` with the joint kernels (csrc/lk_joint.hip) against the Jacobian route it replaces, and the kernel alone
against the as-written algebra of one layer (dev tool; writes profiles/joint_bench.json).

  python tools/joint_bench.py [--out profiles/joint_bench.json] [--only LEG]

  * e2e: `la(X, joint=True)` with `use_joint_kernels` on and off, Kron and diag posteriors over all weights, on c1 (MLP 1-50-1) at
    B = 1000 and on Linear(16,1024)-Tanh-Linear(1024,1024)-Tanh-Linear(1024,C) for C in {1, 4} at B in {64, 256, 1024}.
  * kernel: `HipKernels.kron_joint_linear` on the operands of one 1024 x 1024 layer against the torch form of what
    `Js`-assembly + `inv_square_form` do for that layer (the block of Js, the sandwich through both eigenbases and back, the
    [B C, P] x [P, B C] product), at the same C and B.
  The inputs rotate through NBUF buffers, the two sides alternate over ROUNDS rounds.
  GATE: on no line of `e2e` is the switch on slower than off beyond the spread (the larger max - min over the rounds of the two
  sides); the default of `_HipLaplace.use_joint_kernels` follows it.

One child process per leg, each under its own time limit; a failing leg ends the run.  Times are device events around synchronised
work after a warm-up; no profiler; no device, no measurement.
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

LEGS = ("e2e", "kernel")
LEG_TIMEOUT = {"e2e": 500, "kernel": 300}
ROUNDS, NBUF = 5, 3
WIDE = [(C, B) for C in (1, 4) for B in (64, 256, 1024)]


def _timed(torch, fn, iters):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _line(t_new, t_old):
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    spread = max(max(t_new) - min(t_new), max(t_old) - min(t_old))
    return {"on_ms": med(t_new), "off_ms": med(t_old), "on_ms_rounds": t_new, "off_ms_rounds": t_old, "spread_ms": spread,
            "speedup": med(t_old) / med(t_new), "not_slower_beyond_the_spread": bool(med(t_new) <= med(t_old) + spread)}


def _alternate(torch, new, old, warm, iters):
    for fn in (new, old):
        for i in range(warm):
            fn(i)
    t_new, t_old = [], []
    for _ in range(ROUNDS):  # alternating rounds
        t_new.append(_timed(torch, new, iters))
        t_old.append(_timed(torch, old, iters))
    return t_new, t_old


def _device():
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("joint_bench: no ROCm device (a measurement does not fall back to the CPU)")
    return torch


def leg_e2e(args):
    torch = _device()
    from torch import nn
    from torch.utils.data import DataLoader, TensorDataset

    from laplace_amd.laplace import HipLaplace

    def wide(C):
        return nn.Sequential(nn.Linear(16, 1024), nn.Tanh(), nn.Linear(1024, 1024), nn.Tanh(), nn.Linear(1024, C)), 16

    models = [("c1", lambda: (nn.Sequential(nn.Linear(1, 50), nn.Tanh(), nn.Linear(50, 1)), 1), 1, 1000)]
    models += [(f"wide_C{C}", lambda C=C: wide(C), C, B) for C, B in WIDE]
    out = {}
    for name, make, C, B in models:
        for hs in ("kron", "diag"):
            torch.manual_seed(5)
            model, d_in = make()
            model = model.cuda().eval()
            Xt, yt = torch.randn(256, d_in, device="cuda"), torch.randn(256, C, device="cuda")
            la = HipLaplace(model, "regression", "all", hs)
            la.fit(DataLoader(TensorDataset(Xt, yt), batch_size=128))
            Xs = [torch.randn(B, d_in, device="cuda") for _ in range(NBUF)]

            def call(on):
                def fn(i):
                    la.use_joint_kernels = on
                    return la(Xs[i % NBUF], joint=True)
                return fn

            t_new, t_old = _alternate(torch, call(True), call(False), 1, 10 if name == "c1" else (3 if B <= 256 else 1))
            key = f"{name}_B{B}_{hs}"
            out[key] = _line(t_new, t_old)
            print(f"{key}: on {out[key]['on_ms']:.3f} ms, off {out[key]['off_ms']:.3f} ms", flush=True)
            del la, Xs
            torch.cuda.empty_cache()
    return out


def leg_kernel(args):
    torch = _device()
    from laplace_amd._lib import get_kernels

    K, out, Do, Di = get_kernels(), {}, 1024, 1024
    g = torch.Generator("cuda").manual_seed(1)
    Q1, Q2 = (torch.linalg.qr(torch.randn(n, n, device="cuda", generator=g))[0] for n in (Do, Di))
    l1, l2 = torch.rand(Do, device="cuda", generator=g), torch.rand(Di, device="cuda", generator=g)
    delta = torch.ones(1, device="cuda")
    w = 1.0 / (torch.outer(l1, l2) + delta)
    for C, B in WIDE:
        gs = [torch.randn(C, B, Do, device="cuda", generator=g) for _ in range(NBUF)]
        acts = [torch.randn(B, Di, device="cuda", generator=g) for _ in range(NBUF)]
        cov = torch.zeros(B * C, B * C, device="cuda")

        def new(i):  # the two rotations of the driver and the kernel
            gg, a = gs[i % NBUF], acts[i % NBUF]
            u = (gg.reshape(C * B, Do) @ Q1).reshape(C, B, Do)
            return K.kron_joint_linear(u, a @ Q2, l1, l2, delta, cov.zero_())

        def old(i):  # the layer's block of Js, the sandwich of matrix.py:406-456 and the product of :458-461
            W = torch.einsum("cno,ni->ncoi", gs[i % NBUF], acts[i % NBUF]).reshape(B * C, Do, Di)
            SW = Q1 @ ((Q1.T @ W @ Q2) * w) @ Q2.T
            return W.reshape(B * C, -1) @ SW.reshape(B * C, -1).T

        t_new, t_old = _alternate(torch, new, old, 1, 3 if B <= 256 else 1)
        key = f"C{C}_B{B}_{Do}x{Di}"
        out[key] = {"variant": K.joint_linear_variant("kron", B, C, Do, Di), **_line(t_new, t_old)}
        print(f"{key}: kernel {out[key]['on_ms']:.3f} ms, as written {out[key]['off_ms']:.3f} ms", flush=True)
        del gs, acts, cov
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_bench.json"))
    ap.add_argument("--only", choices=LEGS)
    ap.add_argument("--leg", choices=LEGS, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        print("LEG_RESULT " + json.dumps(globals()["leg_" + args.leg](args)))
        return 0
    _device()
    res = {"what": "tools/joint_bench.py", "rounds": ROUNDS, "buffers": NBUF}
    for leg in LEGS if not args.only else (args.only,):
        t0 = time.time()
        cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT[leg]), sys.executable, os.path.abspath(__file__), "--leg", leg]
        proc = subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        lines = []
        for ln in proc.stdout:  # (each line as it comes: a long leg is not silent)
            lines.append(ln)
            if not ln.startswith("LEG_RESULT "):
                print(ln, end="", flush=True)
        if proc.wait() != 0:
            raise SystemExit(f"joint_bench: leg {leg} ended with status {proc.returncode}")
        res[leg] = json.loads([ln for ln in lines if ln.startswith("LEG_RESULT ")][-1][11:])
        res[leg + "_seconds"] = time.time() - t0
    if "e2e" in res:
        slow = [k for k, v in res["e2e"].items() if not v["not_slower_beyond_the_spread"]]
        res["gate"] = {"holds": not slow, "slower_lines": slow, "default_of_use_joint_kernels": not slow}
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(f"wrote {args.out}; gate: {res.get('gate', 'e2e leg not measured')}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
