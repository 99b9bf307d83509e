"""The sampled-heads kernel of the `nn` predictive (csrc/lk_nnhead.hip) against the torch form of the same arithmetic, and the public
call against the per-draw loop it replaces (dev tool; writes profiles/nn_head_bench.json).

  python tools/nn_head_bench.py [--out profiles/nn_head_bench.json] [--only LEG]

  * kernel: `HipKernels.nn_head` against `baddbmm -> softmax -> mean` (regression: `baddbmm -> mean, var`) on cached features, at
    B = 128, S = 100 and (C, D) = (10, 512), (100, 512), (1000, 512), (1000, 2048); the moments at (1, 512) and (10, 512).  Both
    sides read the same `theta [S, P]` rows; features and draws rotate through NBUF buffers, the two sides alternate over 7 rounds.
  * e2e: `la(X, pred_type="nn", link_approx="mc")` on a last-layer Kron posterior of `nets.ResNet18()` at a batch of 128 with the
    kernel, with the switch off (one feature pass, a head launch per draw) and with the loop of n_samples model passes that both
    replace.  Every side includes the draw (`la.sample`).
  GATE: no line of `kernel` is slower with the kernel than the torch form beyond the spread (the larger max - min over the rounds
  of the two sides); the default of `_HipLaplace.use_nn_head_kernels` follows it.

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

LEGS = ("kernel", "e2e")
LEG_TIMEOUT = {"kernel": 300, "e2e": 420}
# (C, D, mode) at B = 128, S = 100
SHAPES = [(10, 512, "probs"), (100, 512, "probs"), (1000, 512, "probs"), (1000, 2048, "probs"), (1, 512, "moments"),
          (10, 512, "moments")]
B, N_SAMPLES, ROUNDS = 128, 100, 7


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
    return {"kernel_ms": med(t_new), "torch_ms": med(t_old), "kernel_ms_rounds": t_new, "torch_ms_rounds": t_old, "spread_ms": spread,
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
        raise SystemExit("nn_head_bench: no ROCm device (a measurement does not fall back to the CPU)")
    return torch


def leg_kernel(args):
    torch = _device()
    from laplace_amd._lib import get_kernels

    K, out = get_kernels(), {}
    for C, D, mode in SHAPES:
        g = torch.Generator("cuda").manual_seed(C + D)
        P = C * D + C
        nbuf = 16 if S_bytes(P) < (64 << 20) else 4  # (the draws of a 1000 x 2048 head are 0.8 GB)
        phis = [torch.randn(B, D, device="cuda", generator=g) for _ in range(nbuf)]
        thetas = [torch.randn(N_SAMPLES, P, device="cuda", generator=g) / D ** 0.5 for _ in range(nbuf)]
        outs = [torch.empty(B, C, device="cuda") for _ in range(2)]
        need = K.lib.lk_nn_head_work_bytes(B, C, D, N_SAMPLES, K.NN_HEAD_MODES[mode])
        work = torch.empty(max(need // 4, 4), device="cuda")

        def new(i):
            K.nn_head(phis[i % nbuf], thetas[i % nbuf], C, True, mode, out=outs[0], out2=outs[1] if mode == "moments" else None,
                      work=work)

        def old(i):
            phi, th = phis[i % nbuf], thetas[i % nbuf]
            f = torch.baddbmm(th[:, None, C * D:], phi.expand(N_SAMPLES, B, D), th[:, :C * D].view(N_SAMPLES, C, D).transpose(1, 2))
            return (f.mean(0), f.var(0)) if mode == "moments" else f.softmax(-1).mean(0)

        t_new, t_old = _alternate(torch, new, old, 3, 200 if P < 100000 else 20)
        key = f"B{B}_C{C}_D{D}_{mode}"
        out[key] = {"variant": K.nn_head_variant(B, C, D, N_SAMPLES, mode), "theta_MB": S_bytes(P) / 1e6, **_line(t_new, t_old)}
        print(f"{key}: kernel {out[key]['kernel_ms']:.4f} ms, torch {out[key]['torch_ms']:.4f} ms", flush=True)
        del phis, thetas
        torch.cuda.empty_cache()
    return out


def S_bytes(P):
    return 4 * N_SAMPLES * P


def leg_e2e(args):
    torch = _device()
    from torch.nn.utils import vector_to_parameters
    from torch.utils.data import DataLoader, TensorDataset

    from laplace_amd.laplace import HipLaplace
    from laplace_amd.nets import ResNet18

    torch.manual_seed(711)
    model = ResNet18().cuda().eval()
    g = torch.Generator().manual_seed(0)
    X, y = torch.randn(256, 3, 32, 32, generator=g).cuda(), torch.randint(10, (256,), generator=g).cuda()
    la = HipLaplace(model, "classification", "last_layer", "kron")
    la.fit(DataLoader(TensorDataset(X, y), batch_size=B))
    Xb = X[:B]

    def call(on):
        def fn(i):
            la.use_nn_head_kernels = on
            return la(Xb, pred_type="nn", link_approx="mc", n_samples=N_SAMPLES)
        return fn

    @torch.no_grad()
    def parent(i):  # the loop before this kernel: a scatter of the draw and a pass of the whole model per draw
        fs = []
        for sample in la.sample(N_SAMPLES):
            vector_to_parameters(sample, la.params)
            fs.append(la.model(Xb).detach())
        vector_to_parameters(la.mean, la.params)
        return torch.softmax(torch.stack(fs), dim=-1).mean(dim=0)

    out = {}
    for name, old in (("kernel_vs_model_pass_per_draw", parent), ("kernel_vs_cached_feature_loop", call(False))):
        t_new, t_old = _alternate(torch, call(True), old, 2, 3)
        out[name] = _line(t_new, t_old)
        print(f"{name}: kernel {out[name]['kernel_ms']:.3f} ms, without {out[name]['torch_ms']:.3f} ms", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn_head_bench.json"))
    ap.add_argument("--only", choices=LEGS)
    ap.add_argument("--leg", choices=LEGS, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        print("LEG_RESULT " + json.dumps(globals()["leg_" + args.leg](args)))
        return 0
    _device()
    res = {"what": "tools/nn_head_bench.py", "B": B, "n_samples": N_SAMPLES, "rounds": ROUNDS}
    for leg in LEGS if not args.only else (args.only,):
        t0 = time.time()
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg], cwd=ROOT, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True, timeout=LEG_TIMEOUT[leg])
        print(proc.stdout[-3000:], flush=True)
        if proc.returncode != 0:
            raise SystemExit(f"nn_head_bench: leg {leg} ended with status {proc.returncode}")
        res[leg] = json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith("LEG_RESULT ")][-1][11:])
        res[leg + "_seconds"] = time.time() - t0
    if "kernel" in res:
        slow = [k for k, v in res["kernel"].items() if not v["not_slower_beyond_the_spread"]]
        res["gate"] = {"holds": not slow, "slower_lines": slow, "default_of_use_nn_head_kernels": not slow}
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(f"wrote {args.out}; gate: {res.get('gate', 'kernel leg not measured')}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
