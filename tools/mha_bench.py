"""Cost of serving nn.MultiheadAttention and the stock transformer encoder on the device (dev tool; writes profiles/mha_bench.json).

  python tools/mha_bench.py [--out profiles/mha_bench.json]

  * kron: `HipGGN.kron` per minibatch of 128 on `nets.ViTStock()`, four lines that alternate in one process: the sweep with the
    strided attention entry points, with `use_strided_attn = False` (contiguous copies of the three slices of the packed
    projection, the layout-1 entry points, a concatenation of the three cotangents), on the torch math
    (`use_attn_kernels = False`), and the autograd tape (`use_sweep = False`, the hook route).  `nets.ViTSmall()` (separate q / k /
    v Linear layers, the sweep) is measured beside them.
    GATE 1: no sweep line is slower than the tape (no margin).
    GATE 2: the strided line is not slower than `use_strided_attn = False` beyond the recorded spread (the larger of the two
    lines' max - min over the rounds).
  * kernel: at S = 9, B = 128, H = 3, T = 64, D = 64 each strided call against what it replaces: `lk_attn_fwd_strided_f32` on the
    packed `[B, T, 3 E]` projection against three slice copies plus `lk_attn_fwd_f32` (layout 1); `lk_attn_vjp_strided_f32` into
    one `[S B, T, 3 E]` buffer against `lk_attn_vjp_f32` (layout 1) plus the concatenation of its three results.  The buffers
    rotate through 1 GiB so that the 256 MiB last-level cache cannot hold them from one launch to the next.

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

LEGS = ("kron", "kernel")
LEG_TIMEOUT = {"kron": 300, "kernel": 200}


def _setup(rehearse: bool):
    import torch

    if rehearse:
        from laplace_amd import _lib
        from tests.emulated_mha_kernels import EmulatedMhaKernels

        _lib.set_kernels_for_testing(EmulatedMhaKernels())
        return torch, "cpu"
    if not torch.cuda.is_available():
        raise SystemExit("mha_bench: no ROCm device (a measurement does not fall back to the CPU)")
    return torch, "cuda"


class _Timer:
    """device events around the enclosed work (host clock around it on the rehearsal device)"""

    def __init__(self, torch, dev):
        self.torch, self.dev = torch, dev

    def __call__(self, fn, iters):
        torch = self.torch
        if self.dev == "cpu":
            t0 = time.perf_counter()
            for i in range(iters):
                fn(i)
            return (time.perf_counter() - t0) * 1e3 / iters
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters


def _median(v):
    return sorted(v)[len(v) // 2]


def _spread(*rounds):
    return max(max(r) - min(r) for r in rounds)


def leg_kron(args):
    torch, dev = _setup(args.rehearse)
    from laplace_amd import HipGGN
    from laplace_amd.nets import ViTSmall, ViTStock

    B = 4 if args.rehearse else 128
    small = dict(image=8, dim=16, depth=1, heads=1) if args.rehearse else {}
    torch.manual_seed(0)
    stock, vit = ViTStock(**small).to(dev).eval(), ViTSmall(**small).to(dev).eval()
    gen = torch.Generator().manual_seed(1)
    X = torch.randn(B, 3, small.get("image", 32), small.get("image", 32), generator=gen).to(dev)
    y = torch.randint(10, (B,), generator=gen).to(dev)
    timer = _Timer(torch, dev)
    lines = {"strided": (stock, {}), "copies": (stock, dict(use_strided_attn=False)), "math": (stock, dict(use_attn_kernels=False)),
             "tape": (stock, dict(use_sweep=False)), "vit_small": (vit, {})}
    backends = {}
    for name, (model, attrs) in lines.items():
        b = backends[name] = HipGGN(model, "classification")
        for k, v in attrs.items():
            setattr(b, k, v)

    def run(b):
        return lambda i: b.kron(X, y, N=B)[1].kfacs  # (the factors in their public layout: a lazy minibatch is read out)

    for b in backends.values():
        for _ in range(1 if args.rehearse else 2):
            run(b)(0)
    for name, b in backends.items():
        tape = b._tape()
        built = any(s not in (None, False) for s in tape.sweeps.values())
        assert built == (name != "tape") and (name == "tape" or getattr(tape, "sweep_reason", None) is None), (name, getattr(tape, "sweep_reason", None))
        assert tape.uncovered == []
    t = {name: [] for name in lines}
    for _ in range(1 if args.rehearse else 7):  # alternating rounds
        for name, b in backends.items():
            t[name].append(timer(run(b), 1 if args.rehearse else 3))
    med = {name: _median(v) for name, v in t.items()}
    spread = _spread(t["strided"], t["copies"])
    print("kron per minibatch of %d: " % B + ", ".join(f"{n} {m:.2f} ms" for n, m in med.items()) + f"; spread {spread:.2f} ms", flush=True)
    return {"batch": B, **{f"{n}_ms": m for n, m in med.items()}, **{f"{n}_ms_rounds": v for n, v in t.items()},
            "spread_ms_strided_and_copies": spread, "taps": len(backends["strided"]._tape().taps),
            "gate_1_no_sweep_line_slower_than_the_tape": bool(all(med[n] <= med["tape"] for n in ("strided", "copies", "math"))),
            "gate_2_strided_not_slower_than_copies_beyond_the_spread": bool(med["strided"] <= med["copies"] + spread)}


def leg_kernel(args):
    torch, dev = _setup(args.rehearse)
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    timer = _Timer(torch, dev)
    S, B, H, T, D = (2, 3, 2, 6, 4) if args.rehearse else (9, 128, 3, 64, 64)
    E, scale = H * D, float(D) ** -0.5
    g_bytes = 4 * S * B * T * E
    nbuf = 1 if args.rehearse else max(2, -(-(1 << 30) // (4 * g_bytes)))  # (go and the three cotangents per launch)
    qkvs = [torch.randn(B, T, 3 * E, device=dev) for _ in range(nbuf)]
    gos = [torch.randn(S * B, T, H, D, device=dev) for _ in range(nbuf)]
    dqkvs = [torch.empty(S * B, T, 3 * E, device=dev) for _ in range(nbuf)]
    views = lambda t, n: t.view(n, T, 3, H, D).unbind(2)  # noqa: E731
    o, lse = K.attn_forward_strided(*views(qkvs[0], B), scale, False)

    def fwd_new(i):
        K.attn_forward_strided(*views(qkvs[i % nbuf], B), scale, False)

    def fwd_base(i):
        K.attn_forward(*(t.contiguous().transpose(1, 2) for t in views(qkvs[i % nbuf], B)), scale, False)

    def vjp_new(i):
        K.attn_vjp_strided(gos[i % nbuf], *views(qkvs[0], B), o, lse, S, scale, False, *views(dqkvs[i % nbuf], S * B))

    q1, k1, v1 = (t.contiguous().transpose(1, 2) for t in views(qkvs[0], B))
    o1 = o.transpose(1, 2)

    def vjp_base(i):
        parts = K.attn_vjp(gos[i % nbuf].transpose(1, 2), q1, k1, v1, o1, lse, S, scale, False)
        torch.cat([d.transpose(1, 2).reshape(S * B, T, E) for d in parts], -1)

    vjp_new(0)
    want = torch.cat([d.transpose(1, 2).reshape(S * B, T, E) for d in K.attn_vjp(gos[0].transpose(1, 2), q1, k1, v1, o1, lse, S, scale, False)], -1)
    equal = bool(torch.equal(dqkvs[0], want)) if dev == "cuda" else None
    fns = {"fwd_strided": fwd_new, "fwd_copies": fwd_base, "vjp_strided": vjp_new, "vjp_copies": vjp_base}
    for fn in fns.values():
        for i in range(min(nbuf, 3)):
            fn(i)
    it = 1 if args.rehearse else max(nbuf, 10)
    t = {k: [] for k in fns}
    for _ in range(1 if args.rehearse else 7):  # alternating rounds
        for k, fn in fns.items():
            t[k].append(timer(fn, it))
    med = {k: _median(v) for k, v in t.items()}
    print(", ".join(f"{k} {m:.4f} ms" for k, m in med.items()) + f"; vjp bit-equal: {equal}", flush=True)
    return {"S": S, "B": B, "H": H, "T": T, "D": D, "buffers_rotated": nbuf, **{f"{k}_ms": m for k, m in med.items()},
            **{f"{k}_ms_rounds": v for k, v in t.items()}, "fwd_spread_ms": _spread(t["fwd_strided"], t["fwd_copies"]),
            "vjp_spread_ms": _spread(t["vjp_strided"], t["vjp_copies"]), "fwd_speedup": med["fwd_copies"] / med["fwd_strided"],
            "vjp_speedup": med["vjp_copies"] / med["vjp_strided"], "vjp_bit_equal_to_layout_1": equal,
            "variant": K.attn_variant(S, B, H, T, D, 1, False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mha_bench.json"))
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg:  # child: one leg, result as the last line of stdout
        res = {"kron": leg_kron, "kernel": leg_kernel}[args.leg](args)
        print("MHA_BENCH_RESULT " + json.dumps(res), flush=True)
        return
    result = {"tool": "tools/mha_bench.py", "rehearsal_on_cpu_emulation_times_meaningless": bool(args.rehearse)}
    for leg in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg] + (["--rehearse"] if args.rehearse else [])
        t0 = time.time()
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT[leg], cwd=ROOT)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"mha_bench: leg {leg} exceeded {LEG_TIMEOUT[leg]} s; stopping")
        sys.stdout.write(proc.stdout)
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr[-4000:])
            raise SystemExit(f"mha_bench: leg {leg} ended with status {proc.returncode}; stopping")
        line = [l for l in proc.stdout.splitlines() if l.startswith("MHA_BENCH_RESULT ")][-1]
        result[leg] = json.loads(line[len("MHA_BENCH_RESULT "):])
        result[leg]["leg_wall_s"] = round(time.time() - t0, 1)
    kr = result["kron"]
    result["summary"] = {
        "gate_1_no_sweep_line_slower_than_the_tape": kr["gate_1_no_sweep_line_slower_than_the_tape"],
        "gate_2_strided_not_slower_than_copies_beyond_the_spread": kr["gate_2_strided_not_slower_than_copies_beyond_the_spread"],
        **{f"kron_{n}_ms_per_minibatch_128": kr[f"{n}_ms"] for n in ("strided", "copies", "math", "tape", "vit_small")},
        "kron_spread_ms": kr["spread_ms_strided_and_copies"],
        "kernel_fwd_speedup": result["kernel"]["fwd_speedup"], "kernel_vjp_speedup": result["kernel"]["vjp_speedup"],
        "use_strided_attn_default": bool(kr["gate_2_strided_not_slower_than_copies_beyond_the_spread"]),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result["summary"]))
    if not args.rehearse and not (kr["gate_1_no_sweep_line_slower_than_the_tape"] and kr["gate_2_strided_not_slower_than_copies_beyond_the_spread"]):
        raise SystemExit("mha_bench: a gate is not met (see the file)")


if __name__ == "__main__":
    main()
