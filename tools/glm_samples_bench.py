"""The GLM samples kernel (csrc/lk_glmsamples.hip) against the torch sequence it replaces (dev tool; writes
profiles/glm_samples_bench.json), after tools/link_bench.py.

  python tools/glm_samples_bench.py [--out profiles/glm_samples_bench.json]

  * kernel: `HipKernels.glm_samples` against the torch sequence of `_HipLaplace._glm_functional_samples` /
    `_glm_predictive_samples` (the batched Cholesky, the product with the shared draw, the broadcast add, for the softmax lines a
    softmax over the permuted [n, B, C] view) on the same tensors, at B = 128, n_samples = 100: C = 10, 64, 100, 192 with the full
    covariance, C = 1000, 4096 with marginal variances [B, C]; logits and softmax each.  Both sides include what a caller pays: the
    draw of z, and with the full covariance the host read of the factorisation's status.  The inputs rotate through NBUF buffers,
    the two sides alternate over 7 rounds.  `out_stream_fraction`: the bytes of the [n, B, C] output over the kernel side's
    median time, as a fraction of 8 TB/s (the whole call: draw, launch and status read, not the kernel alone).
  * e2e: `la.predictive_samples(X)` on the last-layer Kron posterior of `nets.ResNet18()` at a batch of 128 with
    `use_glm_sample_kernels` on and off.
  GATE: no line is slower with the kernel than without it beyond the spread (the larger max - min over the rounds of the two
  sides); the default of `use_glm_sample_kernels` follows it.

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

from tools.link_bench import _device, _line, _timed  # noqa: E402

LEGS = ("kernel", "e2e")
LEG_TIMEOUT = {"kernel": 300, "e2e": 300}
# (C, diag) at B = 128, n_samples = 100
SHAPES = [(10, False), (64, False), (100, False), (192, False), (1000, True), (4096, True)]
B, N_SAMPLES, ROUNDS, NBUF = 128, 100, 7, 8
HBM_BYTES_PER_S = 8e12


def leg_kernel(args):
    torch = _device()
    from laplace_amd._lib import get_kernels
    from laplace_amd.laplace import HipKronLaplace

    K = get_kernels()
    out = {}
    for C, diag in SHAPES:
        g = torch.Generator("cuda").manual_seed(C)
        mus, fvs = [], []
        for _ in range(NBUF):
            if diag:
                fvs.append(0.1 + torch.rand(B, C, device="cuda", generator=g))
            else:
                A = torch.randn(B, C, C, device="cuda", generator=g)
                fvs.append(A @ A.transpose(1, 2) / C + 0.1 * torch.eye(C, device="cuda"))
            mus.append(3 * torch.randn(B, C, device="cuda", generator=g))
        for softmax in (False, True):
            la = HipKronLaplace(torch.nn.Linear(2, 2).cuda(), "classification" if softmax else "regression")
            la.use_glm_sample_kernels = False  # (its torch code, on tensors given here)

            def new(i):
                z = torch.randn(C, N_SAMPLES, device="cuda", generator=g)
                res, info = K.glm_samples(mus[i % NBUF], fvs[i % NBUF], z, diag=diag, softmax=softmax)
                if not diag:
                    bool(info.cpu().any())
                return res

            def old(i):
                f_mu, f_var = mus[i % NBUF], fvs[i % NBUF]
                if not diag:
                    return la._glm_predictive_samples(f_mu, f_var, N_SAMPLES, False, g)
                z = torch.randn(C, N_SAMPLES, device="cuda", generator=g)  # the lines of _glm_functional_samples on [B, C] variances
                fs = (f_mu.unsqueeze(-1) + f_var.sqrt().unsqueeze(-1) * z.unsqueeze(0)).permute(2, 0, 1)
                return torch.softmax(fs, dim=-1) if softmax else fs

            iters = 20 if diag else 50
            for fn in (new, old):
                for i in range(3):
                    fn(i)
            t_new, t_old = [], []
            for _ in range(ROUNDS):  # alternating rounds
                t_new.append(_timed(torch, new, iters))
                t_old.append(_timed(torch, old, iters))
            key = f"B{B}_C{C}_{'diag' if diag else 'full'}_{'softmax' if softmax else 'logits'}"
            line = _line(t_new, t_old)
            out[key] = {"variant": K.glm_samples_variant(B, C, N_SAMPLES, diag, softmax), **line,
                        "out_stream_fraction": 4.0 * N_SAMPLES * B * C / (line["kernel_ms"] * 1e-3) / HBM_BYTES_PER_S}
            print(f"{key}: kernel {line['kernel_ms']:.4f} ms, torch {line['torch_ms']:.4f} ms", flush=True)
        del mus, fvs
        torch.cuda.empty_cache()
    return out


def leg_e2e(args):
    torch = _device()
    from torch.utils.data import DataLoader, TensorDataset

    from laplace_amd.laplace import HipLaplace
    from laplace_amd.nets import ResNet18

    torch.manual_seed(711)
    model = ResNet18().cuda().eval()
    g = torch.Generator().manual_seed(0)
    X, y = torch.randn(256, 3, 32, 32, generator=g).cuda(), torch.randint(10, (256,), generator=g).cuda()
    la = HipLaplace(model, "classification", "last_layer", "kron")
    la.fit(DataLoader(TensorDataset(X, y), batch_size=128))
    Xb = X[:128]

    def run(on):
        def fn(i):
            la.use_glm_sample_kernels = on
            la.predictive_samples(Xb, n_samples=N_SAMPLES)
        return fn

    for on in (True, False):
        run(on)(0)
    t_new, t_old = [], []
    for _ in range(ROUNDS):
        t_new.append(_timed(torch, run(True), 5))
        t_old.append(_timed(torch, run(False), 5))
    res = {"model": "ResNet18(), last-layer Kron, batch 128, predictive_samples, n_samples 100", **_line(t_new, t_old)}
    print(f"e2e predictive_samples: kernel {res['kernel_ms']:.3f} ms, torch {res['torch_ms']:.3f} ms", flush=True)
    return res


def _run_leg(leg):
    """one leg in a child process under its time limit; -> (its result, wall seconds)"""
    t0 = time.time()
    try:
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg], capture_output=True, text=True,
                              timeout=LEG_TIMEOUT[leg], cwd=ROOT)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"glm_samples_bench: leg {leg} exceeded {LEG_TIMEOUT[leg]} s; stopping")
    sys.stdout.write(proc.stdout)
    if proc.returncode != 0:
        sys.stderr.write(proc.stderr[-4000:])
        raise SystemExit(f"glm_samples_bench: leg {leg} ended with status {proc.returncode}; stopping")
    line = [ln for ln in proc.stdout.splitlines() if ln.startswith("GLM_SAMPLES_BENCH_RESULT ")][-1]
    return json.loads(line[len("GLM_SAMPLES_BENCH_RESULT "):]), round(time.time() - t0, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--leg", choices=LEGS)
    args = ap.parse_args()
    if args.leg:  # child: one leg, result as the last line of stdout
        print("GLM_SAMPLES_BENCH_RESULT " + json.dumps({"kernel": leg_kernel, "e2e": leg_e2e}[args.leg](args)), flush=True)
        return
    args.out = args.out or os.path.join(ROOT, "profiles", "glm_samples_bench.json")
    result = {"tool": "tools/glm_samples_bench.py"}
    for leg in LEGS:
        result[leg], result[f"{leg}_leg_wall_s"] = _run_leg(leg)
    lines = {**result["kernel"], "e2e_predictive_samples": result["e2e"]}
    lost = [k for k, v in lines.items() if not v["not_slower_beyond_the_spread"]]
    result["summary"] = {"lines_slower_with_the_kernel": lost, "use_glm_sample_kernels_default": not lost,
                         **{f"{k}_speedup": round(v["speedup"], 2) for k, v in lines.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result["summary"]))


if __name__ == "__main__":
    main()
