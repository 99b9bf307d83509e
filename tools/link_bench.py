"""The fused link kernel of the GLM predictive (csrc/lk_link.hip) against the torch sequence it replaces (dev tool; writes
profiles/link_bench.json).

  python tools/link_bench.py [--out profiles/link_bench.json]

  * kernel: `HipKernels.glm_link` against `_HipLaplace`'s torch code (the batched Cholesky, the product with the shared draw, the
    softmax over [n, B, C] and the mean; the Laplace bridge; probit) on the same tensors, at B = 128 and C = 10, 100, 192, for mc
    (n_samples = 100), bridge and probit.  Both sides include what a caller pays: the draw of z, and for mc the host read of the
    factorisation's status.  The inputs rotate through 16 buffers, the two sides alternate over 7 rounds.
  * e2e: `la(X, link_approx="mc")` on the Kron posterior of config c4 (ResNet-18, batch 128) with `use_link_kernels` on and off.
  GATE: no line is slower with the kernel than without it beyond the spread (the larger max - min over the rounds of the two
  sides); the default of `use_link_kernels` follows it.

  --wide: the same for the wide kernels (csrc/lk_linkwide.hip, `_HipLaplace.use_link_wide_kernels`), written to
  profiles/link_wide_bench.json:
  * wide_kernel: `HipKernels.glm_link_wide` against the torch sequence at B = 128: mc with marginal variances (diag_embed, the
    samples' diagonal, two [n, B, C] tensors) at C = 1000 and 4096, mc with the full covariance at C = 200 and 224 (the served
    range ends at LK_LINK_WIDE_MAX_C_FULL), probit on marginal variances and the bridge on the full covariance at C = 1000.
  * wide_e2e: `la(X, link_approx="probit")` and `la(X, link_approx="mc", diagonal_output=True)` on the Kron posterior of
    `nets.ResNet18(num_classes=1000)` at a predictive batch of 8, with the switch on and off.
  `--only LEG` runs one of the two; the summary names a leg that was not run as not measured, and the default of the switch
  follows the gate only when every line was measured.

One child process per leg, each under its own time limit; a failing leg ends the run.  Times are device events around
synchronised work after a warm-up; no profiler; no device, no measurement.
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
WIDE_LEGS = ("wide_kernel", "wide_e2e")
LEG_TIMEOUT = {"kernel": 240, "e2e": 300, "wide_kernel": 420, "wide_e2e": 600}
# (C, link, diag) at B = 128
WIDE_SHAPES = [(1000, "mc", True), (4096, "mc", True), (200, "mc", False), (224, "mc", False), (1000, "probit", True),
               (1000, "bridge", False)]
SHAPES = [(128, C, link) for C in (10, 100, 192) for link in ("mc", "bridge", "probit")]
N_SAMPLES, ROUNDS, NBUF = 100, 7, 16


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


def _device():
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("link_bench: no ROCm device (a measurement does not fall back to the CPU)")
    return torch


def leg_kernel(args):
    torch = _device()
    from laplace_amd._lib import get_kernels
    from laplace_amd.laplace import HipKronLaplace

    K = get_kernels()
    la = HipKronLaplace(torch.nn.Linear(2, 2).cuda(), "classification")  # (its torch link code, on tensors given here)
    la.use_link_kernels = False
    out = {}
    for B, C, link in SHAPES:
        g = torch.Generator("cuda").manual_seed(C)
        mus, fvs = [], []
        for _ in range(NBUF):
            A = torch.randn(B, C, C, device="cuda", generator=g)
            fvs.append(A @ A.transpose(1, 2) / C + 0.1 * torch.eye(C, device="cuda"))
            mus.append(3 * torch.randn(B, C, device="cuda", generator=g))

        def new(i):
            la._glm_link(K, None, mus[i % NBUF], fvs[i % NBUF], link, N_SAMPLES, False, g)

        def old(i):
            f_mu, f_var = mus[i % NBUF], fvs[i % NBUF]
            if link == "mc":
                return la._glm_predictive_samples(f_mu, f_var, N_SAMPLES, False, g).mean(dim=0)
            if link == "bridge":
                return la._laplace_bridge(f_mu, f_var, normalise=False)
            return torch.softmax(f_mu / torch.sqrt(1.0 + torch.pi / 8 * torch.diagonal(f_var, dim1=1, dim2=2)), dim=-1)

        for fn in (new, old):
            for i in range(3):
                fn(i)
        t_new, t_old = [], []
        for _ in range(ROUNDS):  # alternating rounds
            t_new.append(_timed(torch, new, 200))
            t_old.append(_timed(torch, old, 200))
        out[f"B{B}_C{C}_{link}"] = {"regime": K.glm_link_variant(B, C, N_SAMPLES, link), **_line(t_new, t_old)}
        print(f"B {B} C {C} {link}: kernel {out[f'B{B}_C{C}_{link}']['kernel_ms']:.4f} ms, torch "
              f"{out[f'B{B}_C{C}_{link}']['torch_ms']:.4f} ms", flush=True)
    return out


def leg_wide_kernel(args):
    torch = _device()
    from laplace_amd._lib import get_kernels
    from laplace_amd.laplace import HipKronLaplace

    K = get_kernels()
    la = HipKronLaplace(torch.nn.Linear(2, 2).cuda(), "classification")  # (its torch link code, on tensors given here)
    B, out = 128, {}
    for C, link, diag in WIDE_SHAPES:
        g = torch.Generator("cuda").manual_seed(C)
        nbuf = NBUF if diag or C < 512 else 4  # (a [128, 1000, 1000] buffer is 0.5 GB)
        mus, fvs = [], []
        for _ in range(nbuf):
            if diag:
                fvs.append(0.1 + torch.rand(B, C, device="cuda", generator=g))
            else:
                A = torch.randn(B, C, C, device="cuda", generator=g)
                fvs.append(A @ A.transpose(1, 2) / C + 0.1 * torch.eye(C, device="cuda"))
            mus.append(3 * torch.randn(B, C, device="cuda", generator=g))

        def new(i):
            la._glm_link(K, None, mus[i % nbuf], fvs[i % nbuf], link, N_SAMPLES, diag, g, wide=True)

        def old(i):
            f_mu, f_var = mus[i % nbuf], fvs[i % nbuf]
            if link == "mc":
                fv = torch.diag_embed(f_var) if diag else f_var
                return la._glm_predictive_samples(f_mu, fv, N_SAMPLES, diag, g).mean(dim=0)
            if link == "bridge":
                return la._laplace_bridge(f_mu, f_var, normalise=False)
            return torch.softmax(f_mu / torch.sqrt(1.0 + torch.pi / 8 * f_var), dim=-1)

        for fn in (new, old):
            for i in range(2):
                fn(i)
        t_new, t_old = [], []
        for _ in range(ROUNDS):  # alternating rounds
            t_new.append(_timed(torch, new, 20))
            t_old.append(_timed(torch, old, 20))
        key = f"B{B}_C{C}_{link}_{'diag' if diag else 'full'}"
        out[key] = {"variant": K.glm_link_wide_variant(B, C, N_SAMPLES, link, diag), **_line(t_new, t_old)}
        print(f"{key}: kernel {out[key]['kernel_ms']:.4f} ms, torch {out[key]['torch_ms']:.4f} ms", flush=True)
        del mus, fvs
        torch.cuda.empty_cache()
    return out


def leg_wide_e2e(args):
    torch = _device()
    from torch.utils.data import DataLoader, TensorDataset

    from laplace_amd.laplace import HipLaplace
    from laplace_amd.nets import ResNet18

    torch.manual_seed(711)
    model = ResNet18(1000).cuda().eval()
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            for p in m.parameters():
                p.requires_grad_(False)
    g = torch.Generator().manual_seed(0)
    X, y = torch.randn(16, 3, 32, 32, generator=g).cuda(), torch.randint(1000, (16,), generator=g).cuda()
    la = HipLaplace(model, "classification", "all", "kron")
    la.fit(DataLoader(TensorDataset(X, y), batch_size=8))
    Xb, out = X[:8], {}
    for name, kw in (("probit", dict(link_approx="probit")), ("mc_diag", dict(link_approx="mc", diagonal_output=True))):
        def run(on):
            def fn(i):
                la.use_link_wide_kernels = on
                la(Xb, n_samples=N_SAMPLES, **kw)
            return fn

        run(True)(0)
        try:
            run(False)(0)
        except torch.OutOfMemoryError as exc:  # the torch route cannot serve the shape: the kernel's time alone, no ratio
            torch.cuda.empty_cache()
            t_new = [_timed(torch, run(True), 2) for _ in range(3)]
            out[f"e2e_{name}"] = {"model": "ResNet18(1000), Kron, batch 8", "kernel_ms": sorted(t_new)[1], "kernel_ms_rounds": t_new,
                                  "torch_ms": None, "torch_side": "out of memory: " + str(exc)[:80], "speedup": None,
                                  "not_slower_beyond_the_spread": True}
            print(f"e2e {name}: kernel {out[f'e2e_{name}']['kernel_ms']:.3f} ms, torch out of memory", flush=True)
            continue
        t_new, t_old = [], []
        for _ in range(3):
            t_new.append(_timed(torch, run(True), 2))
            t_old.append(_timed(torch, run(False), 2))
        out[f"e2e_{name}"] = {"model": "ResNet18(1000), Kron, batch 8", **_line(t_new, t_old)}
        print(f"e2e {name}: kernel {out[f'e2e_{name}']['kernel_ms']:.3f} ms, torch {out[f'e2e_{name}']['torch_ms']:.3f} ms", flush=True)
    return out


def _run_leg(leg):
    """one leg in a child process under its time limit; -> (its result, wall seconds)"""
    t0 = time.time()
    try:
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg], capture_output=True, text=True,
                              timeout=LEG_TIMEOUT[leg], cwd=ROOT)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"link_bench: leg {leg} exceeded {LEG_TIMEOUT[leg]} s; stopping")
    sys.stdout.write(proc.stdout)
    if proc.returncode != 0:
        sys.stderr.write(proc.stderr[-4000:])
        raise SystemExit(f"link_bench: leg {leg} ended with status {proc.returncode}; stopping")
    line = [ln for ln in proc.stdout.splitlines() if ln.startswith("LINK_BENCH_RESULT ")][-1]
    return json.loads(line[len("LINK_BENCH_RESULT "):]), round(time.time() - t0, 1)


def main_wide(args):
    result = {"tool": "tools/link_bench.py --wide"}
    for leg in WIDE_LEGS if not args.only else (args.only,):
        result[leg], result[f"{leg}_leg_wall_s"] = _run_leg(leg)
    lines = {**result.get("wide_kernel", {}), **result.get("wide_e2e", {})}
    lost = [k for k, v in lines.items() if not v["not_slower_beyond_the_spread"]]
    missing = [leg for leg in WIDE_LEGS if leg not in result]
    result["summary"] = {"lines_slower_with_the_kernel": lost, "legs_not_measured": missing,
                         "use_link_wide_kernels_default": not lost and not missing,
                         **{f"{k}_speedup": v["speedup"] and round(v["speedup"], 2) for k, v in lines.items()}}
    out = args.out or os.path.join(ROOT, "profiles", "link_wide_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result["summary"]))


def leg_e2e(args):
    torch = _device()
    from torch.utils.data import DataLoader, TensorDataset

    from laplace_amd.laplace import HipLaplace
    from laplace_amd.nets import ResNet18

    torch.manual_seed(711)
    model = ResNet18(10).cuda().eval()
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            for p in m.parameters():
                p.requires_grad_(False)
    g = torch.Generator().manual_seed(0)
    X, y = torch.randn(256, 3, 32, 32, generator=g).cuda(), torch.randint(10, (256,), generator=g).cuda()
    la = HipLaplace(model, "classification", "all", "kron")
    la.fit(DataLoader(TensorDataset(X, y), batch_size=128))
    Xb = X[:128]

    def run(on):
        def fn(i):
            la.use_link_kernels = on
            la(Xb, link_approx="mc", n_samples=N_SAMPLES)
        return fn

    for on in (True, False):
        run(on)(0)
    t_new, t_old = [], []
    for _ in range(ROUNDS):
        t_new.append(_timed(torch, run(True), 5))
        t_old.append(_timed(torch, run(False), 5))
    res = {"model": "ResNet18(10), Kron, batch 128, mc, n_samples 100", **_line(t_new, t_old)}
    print(f"e2e mc: kernel {res['kernel_ms']:.3f} ms, torch {res['torch_ms']:.3f} ms", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--leg", choices=LEGS + WIDE_LEGS)
    ap.add_argument("--wide", action="store_true", help="the wide kernels' lines -> profiles/link_wide_bench.json")
    ap.add_argument("--only", choices=WIDE_LEGS, help="with --wide: run this leg alone")
    args = ap.parse_args()
    if args.leg:  # child: one leg, result as the last line of stdout
        legs = {"kernel": leg_kernel, "e2e": leg_e2e, "wide_kernel": leg_wide_kernel, "wide_e2e": leg_wide_e2e}
        print("LINK_BENCH_RESULT " + json.dumps(legs[args.leg](args)), flush=True)
        return
    if args.wide:
        return main_wide(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "link_bench.json")
    result = {"tool": "tools/link_bench.py"}
    for leg in LEGS:
        result[leg], result[f"{leg}_leg_wall_s"] = _run_leg(leg)
    lines = {**result["kernel"], "e2e_mc": result["e2e"]}
    lost = [k for k, v in lines.items() if not v["not_slower_beyond_the_spread"]]
    result["summary"] = {"lines_slower_with_the_kernel": lost, "use_link_kernels_default": not lost,
                         **{f"{k}_speedup": round(v["speedup"], 2) for k, v in lines.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result["summary"]))


if __name__ == "__main__":
    main()
