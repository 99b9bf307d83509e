"""Cost of serving token models on the device (dev tool; writes profiles/embed_bench.json).

  python tools/embed_bench.py [--out profiles/embed_bench.json]

  * kron: `HipGGN.kron` per minibatch of 128 on `nets.TextTransformer(freeze_embed=True)` (embedding and positions frozen), the
    seed-batched sweep against the autograd tape (`use_sweep = False`), alternating in one process.
    GATE 1: the sweep is not slower (no margin).
  * diag / generic: `HipGGN.diag` per minibatch of 128 on `nets.TextTransformer()` (everything tracked but the norms) on the
    device route, and on the generic `torch.func` route (`use_embed_kernels = False`) at the largest power-of-two batch that
    completes within 60 s, scaled per sample.
  * kernel: `lk_diag_embed_f32` and `lk_jac_embed_f32` at the workload's shape (S = 9, B = 128, T = 64, D = 192, V = 1000): time
    and the rate of the bytes that must move (the cotangent once, the written columns once), beside the `index_add_`
    formulation on the same data (one `index_add_` of the flattened cotangent into the zeroed `[B, S, V, D]` block; for the
    diagonal that block square-summed by `lk_sq_colsum_f32`; the zero fill the formulation needs is part of its time, the
    zero fill of `Js` that BOTH Jacobian routes need is timed for neither).  Uniform ids and the skewed case: half of all tokens
    are one id.  Both alternate in one process; the cotangent buffers rotate through 1 GiB so that the 256 MiB last-level cache
    cannot hold them from one launch to the next.
    GATE 2: at both id distributions neither kernel is slower than the `index_add_` formulation (no margin).

One child process per leg, each under its own time limit; a failing leg ends the run.  Times are device events around
synchronised work after a warm-up; no profiler.  `--rehearse` runs tiny shapes on the CPU emulation to check the host logic
and writes no times worth reading (the file says so).
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

LEGS = ("kron", "diag", "generic", "kernel")
LEG_TIMEOUT = {"kron": 200, "diag": 150, "generic": 300, "kernel": 300}
HBM_TBPS = 6.29  # the copy rate the measuring guide gives for the device


def _setup(rehearse: bool):
    import torch

    if rehearse:
        from laplace_amd import _lib
        from tests.emulated_embed_kernels import EmulatedEmbedKernels

        _lib.set_kernels_for_testing(EmulatedEmbedKernels())
        _switch_on()
        return torch, "cpu"
    _switch_on()
    if not torch.cuda.is_available():
        raise SystemExit("embed_bench: no ROCm device (a measurement does not fall back to the CPU)")
    return torch, "cuda"


def _switch_on():
    """the route ships opt-in: every leg of this tool measures it switched on (the generic leg switches its backend off again)"""
    from laplace_amd.backend import _HipCurvatureMixin

    _HipCurvatureMixin.use_embed_kernels = True


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


def _model(torch, dev, rehearse, **kw):
    from laplace_amd.nets import TextTransformer

    torch.manual_seed(0)
    small = dict(vocab=50, T=8, dim=16, depth=1, heads=1) if rehearse else {}
    return TextTransformer(**small, **kw).to(dev).eval()


def _batch(torch, dev, model, B):
    gen = torch.Generator().manual_seed(1)
    T, V = model.pos.shape[1], model.embed.num_embeddings
    return torch.randint(0, V, (B, T), generator=gen).to(dev), torch.randint(10, (B,), generator=gen).to(dev)


def leg_kron(args):
    torch, dev = _setup(args.rehearse)
    from laplace_amd import HipGGN

    B = 4 if args.rehearse else 128
    model = _model(torch, dev, args.rehearse, freeze_embed=True)
    X, y = _batch(torch, dev, model, B)
    timer = _Timer(torch, dev)
    sweep, tape = HipGGN(model, "classification"), HipGGN(model, "classification")
    tape.use_sweep = False

    def run(b):
        return lambda i: b.kron(X, y, N=B)[1].kfacs  # (the factors in their public layout: a lazy minibatch is read out)

    for b in (sweep, tape):
        for _ in range(1 if args.rehearse else 2):
            run(b)(0)
    st = sweep._tape()
    assert getattr(st, "sweep_reason", None) is None and st.sweep, getattr(st, "sweep_reason", None)
    assert not getattr(tape._tape(), "sweep", None)
    t_s, t_t = [], []
    for _ in range(1 if args.rehearse else 5):  # alternating rounds
        t_s.append(timer(run(sweep), 1 if args.rehearse else 3))
        t_t.append(timer(run(tape), 1 if args.rehearse else 3))
    ms_s, ms_t = _median(t_s), _median(t_t)
    print(f"kron per minibatch of {B}: sweep {ms_s:.2f} ms, tape {ms_t:.2f} ms", flush=True)
    return {"batch": B, "sweep_ms": ms_s, "sweep_ms_rounds": t_s, "tape_ms": ms_t, "tape_ms_rounds": t_t, "speedup": ms_t / ms_s,
            "sweep": type(st.sweep).__name__, "gate_sweep_not_slower": bool(ms_s <= ms_t)}


def leg_diag(args):
    """`HipGGN.diag` per minibatch of 128 on the device route"""
    torch, dev = _setup(args.rehearse)
    from laplace_amd import HipGGN

    B = 4 if args.rehearse else 128
    model = _model(torch, dev, args.rehearse)
    X, y = _batch(torch, dev, model, B)
    b = HipGGN(model, "classification")
    assert b._supported()
    timer = _Timer(torch, dev)
    for _ in range(1 if args.rehearse else 3):
        b.diag(X, y)
    tape = b._tape()
    assert getattr(tape, "sweep_reason", None) is None
    rounds = [timer(lambda i: b.diag(X, y), 1 if args.rehearse else 5) for _ in range(1 if args.rehearse else 3)]
    return {"batch": B, "diag_ms": _median(rounds), "diag_ms_rounds": rounds, "ms_per_sample": _median(rounds) / B,
            "n_params": tape.n_params, "embed_taps": len(tape.embed_taps), "param_taps": len(tape.param_taps)}


def leg_generic(args):
    """the route such a model takes without the switch (`use_embed_kernels = False`: the generic torch.func Jacobian), at growing
    power-of-two batches while a call stays within 60 s and its Jacobian within the free memory"""
    torch, dev = _setup(args.rehearse)
    from laplace_amd import HipGGN

    model = _model(torch, dev, args.rehearse)
    b = HipGGN(model, "classification")
    b.use_embed_kernels = False
    assert not b._supported()
    P = sum(p.numel() for p in model.parameters() if p.requires_grad)
    runs, timer = [], _Timer(torch, dev)
    B = 1
    while B <= (2 if args.rehearse else 128):
        need = 3 * B * 10 * P * 4  # the [B, C, P] Jacobian, its per-parameter pieces before the concatenation, slack
        free = torch.cuda.mem_get_info()[0] if dev == "cuda" else 1 << 40
        if need > 0.8 * free:
            runs.append({"batch": B, "status": f"not run: about {need / 1e9:.0f} GB needed, {free / 1e9:.0f} GB free"})
            break
        X, y = _batch(torch, dev, model, B)
        try:
            if B == 1:
                b.diag(X, y)  # warm-up (code objects, allocator) at the first size only
            ms = timer(lambda i: b.diag(X, y), 1)
        except torch.OutOfMemoryError as e:
            runs.append({"batch": B, "status": f"out of memory: {str(e)[:80]}"})
            break
        runs.append({"batch": B, "status": "ok", "diag_ms": ms, "ms_per_sample": ms / B})
        print(f"generic route, batch {B}: {ms:.1f} ms", flush=True)
        print("EMBED_BENCH_PARTIAL " + json.dumps(runs[-1]), flush=True)
        if ms > 60e3:
            runs[-1]["status"] = "over 60 s"
            break
        if ms * 2 > 60e3:  # (the next size would not fit the window)
            break
        B *= 2
    ok = [r for r in runs if r["status"] == "ok"]
    return {"runs": runs, "largest_ok": ok[-1] if ok else None, "n_params": P}


def leg_kernel(args):
    torch, dev = _setup(args.rehearse)
    from laplace_amd._lib import get_kernels

    K = get_kernels()
    timer = _Timer(torch, dev)
    S, B, T, D, V = (2, 3, 8, 4, 10) if args.rehearse else (9, 128, 64, 192, 1000)
    g_bytes = 4 * S * B * T * D
    nbuf = 1 if args.rehearse else max(2, -(-(1 << 30) // g_bytes))
    gen = torch.Generator().manual_seed(3)
    gs = [torch.randn(S, B, T, D, device=dev) for _ in range(nbuf)]
    rows = []
    for dist in ("uniform", "skewed"):
        ids = torch.randint(0, V, (B, T), generator=gen)
        if dist == "skewed":  # half of all tokens are one id (a padding id that is not padding_idx)
            ids[torch.rand(B, T, generator=gen) < 0.5] = 7
        ids = ids.to(dev)
        runs_b = sum(len(set(r.tolist())) for r in ids.cpu())  # (sample, id) runs: what the Jacobian writes
        ids_v = len(set(ids.reshape(-1).tolist()))
        Js = torch.zeros(B, S, V * D, device=dev)
        Jb = torch.zeros(B, S, V * D, device=dev)
        h, hb = torch.zeros(V * D, device=dev), torch.zeros(V * D, device=dev)
        idx = ((torch.arange(B, device=dev)[None, :, None] * S + torch.arange(S, device=dev)[:, None, None]) * V + ids[None]).reshape(-1)

        def jac_new(i):
            K.jac_embed(gs[i % nbuf], ids, V, None, Js, 0)

        def jac_base(i):  # (Js zeroed by the caller in both routes: not timed)
            Jb.view(B * S * V, D).index_add_(0, idx, gs[i % nbuf].reshape(-1, D))

        def diag_new(i):
            K.diag_embed(gs[i % nbuf], ids, V, None, 1.0, h)

        def diag_base(i):  # (the block this formulation needs, zero fill included, then its columns square-summed)
            Jb.zero_()
            Jb.view(B * S * V, D).index_add_(0, idx, gs[i % nbuf].reshape(-1, D))
            K.sq_colsum(Jb, 0, V * D, 1.0, hb)

        jac_new(0), jac_base(0)
        agree_j = float((Js - Jb).abs().max() / Jb.abs().max())
        h.zero_(), hb.zero_()
        diag_new(0), diag_base(0)
        agree_d = float((h - hb).abs().max() / hb.abs().max())
        Jb.zero_()
        for fn in (jac_new, jac_base, diag_new, diag_base):
            for i in range(min(nbuf, 3)):
                fn(i)
            Jb.zero_()
        it = 1 if args.rehearse else max(nbuf, 10)
        t = {k: [] for k in ("jac_new", "jac_base", "diag_new", "diag_base")}
        for _ in range(1 if args.rehearse else 5):  # alternating rounds
            for k, fn, n in (("jac_new", jac_new, it), ("jac_base", jac_base, it), ("diag_new", diag_new, it),
                             ("diag_base", diag_base, max(it // 4, 1))):
                t[k].append(timer(fn, n))
                if k == "jac_base":
                    Jb.zero_()
        med = {k: _median(v) for k, v in t.items()}
        jac_bytes = g_bytes + 4 * runs_b * S * D + 16 * B * T
        diag_bytes = g_bytes + 8 * ids_v * D + 16 * B * T
        rows.append({
            "ids": dist, "S": S, "B": B, "T": T, "D": D, "V": V, "cotangent_bytes": g_bytes, "buffers_rotated": nbuf,
            "sample_id_runs": runs_b, "distinct_ids": ids_v,
            "jac_embed_ms": med["jac_new"], "jac_embed_ms_rounds": t["jac_new"], "jac_bytes_that_must_move": jac_bytes,
            "jac_embed_GBps": jac_bytes / (med["jac_new"] * 1e-3) / 1e9,
            "jac_index_add_ms": med["jac_base"], "jac_index_add_ms_rounds": t["jac_base"], "jac_speedup": med["jac_base"] / med["jac_new"],
            "diag_embed_ms": med["diag_new"], "diag_embed_ms_rounds": t["diag_new"], "diag_bytes_that_must_move": diag_bytes,
            "diag_embed_GBps": diag_bytes / (med["diag_new"] * 1e-3) / 1e9,
            "diag_index_add_ms": med["diag_base"], "diag_index_add_ms_rounds": t["diag_base"],
            "diag_speedup": med["diag_base"] / med["diag_new"],
            "jac_max_normalised_difference": agree_j, "diag_max_normalised_difference": agree_d,
            "gate_not_slower": bool(med["jac_new"] <= med["jac_base"] and med["diag_new"] <= med["diag_base"]),
        })
        r = rows[-1]
        print(f"{dist:8s} jac_embed {r['jac_embed_ms']:.4f} ms ({r['jac_embed_GBps']:.0f} GB/s) vs index_add_ {r['jac_index_add_ms']:.4f} ms"
              f"   diag_embed {r['diag_embed_ms']:.4f} ms ({r['diag_embed_GBps']:.0f} GB/s) vs index_add_ + sq_colsum "
              f"{r['diag_index_add_ms']:.4f} ms   diff {agree_j:.1e} / {agree_d:.1e}", flush=True)
    return {"cases": rows, "gate_met_at_both_distributions": all(r["gate_not_slower"] for r in rows)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "embed_bench.json"))
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--legs", default=",".join(LEGS), help="legs to run (the others are kept from --base)")
    ap.add_argument("--base", help="result file of an earlier run whose other legs are kept")
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg:  # child: one leg, result as the last line of stdout
        res = {"kron": leg_kron, "diag": leg_diag, "generic": leg_generic, "kernel": leg_kernel}[args.leg](args)
        print("EMBED_BENCH_RESULT " + json.dumps(res), flush=True)
        return
    result = {"tool": "tools/embed_bench.py", "rehearsal_on_cpu_emulation_times_meaningless": bool(args.rehearse),
              "hbm_copy_rate_guide_TBps": HBM_TBPS}
    if args.base:
        with open(args.base) as fh:
            result = {**json.load(fh), **result}
    failed = None
    for leg in [l for l in LEGS if l in args.legs.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg] + (["--rehearse"] if args.rehearse else [])
        t0 = time.time()
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT[leg], cwd=ROOT)
        except subprocess.TimeoutExpired as e:
            # what the leg had finished is kept (the generic route reports every batch size as it completes); the run ends here
            out = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
            sys.stdout.write(out)
            part = [json.loads(l[len("EMBED_BENCH_PARTIAL "):]) for l in out.splitlines() if l.startswith("EMBED_BENCH_PARTIAL ")]
            result[leg] = {"status": f"child process exceeded its limit of {LEG_TIMEOUT[leg]} s", "runs": part,
                           "largest_ok": part[-1] if part else None}
            failed = f"embed_bench: leg {leg} exceeded {LEG_TIMEOUT[leg]} s; stopping"
            break
        sys.stdout.write(proc.stdout)
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr[-4000:])
            raise SystemExit(f"embed_bench: leg {leg} ended with status {proc.returncode}; stopping")
        line = [l for l in proc.stdout.splitlines() if l.startswith("EMBED_BENCH_RESULT ")][-1]
        result[leg] = json.loads(line[len("EMBED_BENCH_RESULT "):])
        result[leg]["leg_wall_s"] = round(time.time() - t0, 1)
    kr, de, ge = result.get("kron"), result.get("diag"), (result.get("generic") or {}).get("largest_ok")
    kern = result.get("kernel", {})
    result["summary"] = {
        "gate_1_kron_sweep_not_slower_than_tape": kr and kr.get("gate_sweep_not_slower"),
        "kron_sweep_ms_per_minibatch_128": kr and kr.get("sweep_ms"), "kron_tape_ms_per_minibatch_128": kr and kr.get("tape_ms"),
        "gate_2_kernels_not_slower_than_index_add": kern.get("gate_met_at_both_distributions"),
        "device_route_diag_ms_per_minibatch_128": de and de.get("diag_ms"),
        "device_route_ms_per_sample": de and de.get("ms_per_sample"),
        "generic_route_largest_batch": ge and ge["batch"], "generic_route_ms_per_sample": ge and ge["ms_per_sample"],
        "gain_per_sample": de and ge and "ms_per_sample" in de and ge["ms_per_sample"] / de["ms_per_sample"],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result["summary"]))
    if failed:
        raise SystemExit(failed)
    if not args.rehearse and (kr and not kr.get("gate_sweep_not_slower") or kern and not kern.get("gate_met_at_both_distributions")):
        raise SystemExit("embed_bench: a gate is not met (see the file): the switch ships opt-in")


if __name__ == "__main__":
    main()
