"""csrc/lk_spectral.hip on the device: every row of tests/spectral_fixtures.py through the C ABI against the derived bound, and
``HipFullLaplace(spectral=True)`` end to end against the fp64 oracle and against its own per-point loop."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import spectral_fixtures as sf  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64  # floats of NaN on either side of an output
REPORT = os.path.join(ROOT, "profiles", "spectral_instances.md")
_worst = {}


@pytest.fixture(scope="module")
def K():
    from laplace_amd._lib import get_kernels

    return get_kernels()


def _banded(shape, dev, fill):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
    out = buf[GUARD:GUARD + n].view(*shape)
    if fill is not None:
        out.fill_(fill)
    return buf, out


def _run(K, idx, dev):
    """one call through the C ABI: NaN bands around the output, a NaN-filled workspace of exactly the advertised size"""
    c = sf.CASES[idx]
    X, Q, lam, hfac, deltas = sf.operands(idx)
    N, C, DP, G = c["N"], c["C"], c["DP"], c["G"]
    off = 1 if c["unaligned"] else 0
    xb = torch.empty(X.numel() + off, dtype=torch.float32, device=dev)
    xb[off:] = X.float().reshape(-1).to(dev)
    Xd = xb[off:].view(*X.shape)
    lamd, dd = lam.float().to(dev), deltas.float().to(dev).contiguous()
    nb = K.lib.lk_spectral_workspace_bytes(sf.form_of(c), N, C, DP, G)
    assert nb > 0
    ws = torch.full((nb // 4,), float("nan"), dtype=torch.float32, device=dev)
    grid = c["epi"] == "grid"
    buf, out = _banded((G, N, C) if grid else (N, C, C), dev, 0.0 if grid else None)
    st = torch.cuda.current_stream(dev).cuda_stream
    p = lambda t: t.data_ptr()  # noqa: E731
    if c["loader"] == "ll":
        Qd = Q.float().to(dev).contiguous()
        if grid:
            rc = K.lib.lk_spectral_grid_ll_f32(p(Xd), p(Qd), p(lamd), hfac, p(dd), G, N, C, DP, c["bias"], p(out), p(ws), nb, st)
        else:
            rc = K.lib.lk_spectral_quadform_ll_f32(p(Xd), p(Qd), p(lamd), hfac, p(dd), N, C, DP, c["bias"], p(out), p(ws), nb, st)
    elif grid:
        rc = K.lib.lk_spectral_grid_f32(p(Xd), p(lamd), hfac, p(dd), G, N, C, DP, p(out), p(ws), nb, st)
    else:
        rc = K.lib.lk_spectral_quadform_f32(p(Xd), p(lamd), hfac, p(dd), N, C, DP, p(out), p(ws), nb, st)
    assert rc == 0, K.lib.lk_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), "wrote outside the output"
    return out.cpu().clone()


@pytest.mark.parametrize("idx", range(len(sf.CASES)), ids=[sf.case_id(c) for c in sf.CASES])
def test_case_meets_the_bound_and_repeats_bit_for_bit(K, idx):
    c = sf.CASES[idx]
    got = _run(K, idx, torch.device("cuda"))
    r = sf.ratio(got, idx)
    key = (c["loader"], c["epi"])
    _worst[key] = max(_worst.get(key, 0.0), r)
    print(f"{sf.case_id(c)}: worst |err| / bound = {r:.3f}")
    assert r <= 1.0, f"{sf.case_id(c)}: |err| / bound = {r:.3f}"
    if c["exact"]:
        assert torch.equal(got.double(), sf.reference(idx)[0]), "integer case is not bit-equal"
    if c["epi"] == "cov":
        assert torch.equal(got, got.transpose(1, 2)), "fvar is not exactly symmetric"
    again = _run(K, idx, torch.device("cuda"))
    assert torch.equal(got, again), "a second call gave other bits"


# ---- end to end ----------------------------------------------------------------------------------------------------------------
E2E = [(n, sow, lik) for n in ("mlp", "conv") for sow in ("all", "last_layer") for lik in ("classification", "regression")]


def _fit(name, subset, spectral, likelihood="classification"):
    from laplace_amd.laplace import HipLaplace
    from oracle.make_golden import PRIOR_PREC, SIGMA_NOISE
    from tests.conftest import golden_model, load_golden

    g = load_golden(name, likelihood)
    model, X, y = golden_model(name, g, dtype=torch.float32, device="cuda")
    sig = SIGMA_NOISE if likelihood == "regression" else 1.0
    la = HipLaplace(model, likelihood, subset, "full", spectral=spectral, prior_precision=PRIOR_PREC, sigma_noise=sig)
    la.fit(torch.utils.data.DataLoader(torch.utils.data.TensorDataset(X, y), batch_size=5))
    return la, g, X, y


def _rel(got, want):
    """largest deviation relative to the block's largest entry"""
    want = torch.as_tensor(want, dtype=torch.float64).reshape(-1)
    got = torch.as_tensor(got).detach().double().cpu().reshape(-1)
    return float((got - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("name,subset,lik", E2E)
def test_end_to_end_against_the_fp64_oracle(name, subset, lik):
    """``f_var``, the log marginal likelihood and ``log det`` of both routes at the golden prior against the arrays the fp64
    reference wrote into tests/golden (oracle/make_golden.py): the standing 1e-4 bar, curvature and Jacobians included"""
    errs = {}
    for spectral in (False, True):
        la, g, X, _ = _fit(name, subset, spectral, lik)
        _, fvar = la._glm_predictive_distribution(X)
        tag = f"la.{subset}.full"
        errs[spectral] = (_rel(fvar, g[f"{tag}.f_var"]), _rel(la.log_marginal_likelihood(), g[f"{tag}.marglik"]),
                          _rel(la.log_det_posterior_precision, g[f"{tag}.logdet_post"]))
    _worst[("e2e", f"{name}/{subset}/{lik}")] = (errs[False], errs[True])
    print(f"{name}/{subset}/{lik}: (f_var, marglik, logdet) vs the fp64 golden: Cholesky route "
          + ", ".join(f"{e:.2e}" for e in errs[False]) + "; spectral " + ", ".join(f"{e:.2e}" for e in errs[True]))
    assert max(errs[True]) < 1e-4, errs


def test_grid_matches_the_loop_and_picks_the_same_prior():
    """batched grid against the per-point loop on the spectral route: the losses within the propagated kernel bounds of
    ``spectral_fixtures.grid_loop_case`` (which asserts, in fp64 on the CPU, that the two best points lie further apart), the
    same argmin, the same installed prior"""
    case = sf.grid_loop_case()
    grid, tol = case["grid"], case["tol"]
    la, _, X, y = _fit("mlp", "all", True)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(X, y), batch_size=4)
    batched = la.validation_loss_grid(loader, grid).cpu()
    loop = []
    for pp in grid:
        la.prior_precision = pp
        p = la(X, link_approx="probit")
        loop.append(float(-torch.log(p[torch.arange(len(y)), y.long()].clamp_min(1e-30)).double().mean()))
    loop = torch.tensor(loop, dtype=torch.float64)
    print(f"grid vs loop: largest loss difference {float((batched - loop).abs().max()):.2e}, bound {tol:.2e}; "
          f"against the fp64 losses {float((batched - case['losses']).abs().max()):.2e}")
    assert float((batched - loop).abs().max()) <= tol, (batched, loop, tol)
    assert int(batched.argmin()) == int(loop.argmin()) == case["argmin"]
    la.prior_precision = 123.0
    want = la.gridsearch_prior_precision(loader, -2, 2, 9).clone()
    la.prior_precision = 123.0
    got = la.gridsearch_prior_precision(loader, -2, 2, 9, batched=True)
    assert torch.equal(got, want) and float(got) == pytest.approx(float(grid[case["argmin"]]))


def test_default_object_still_has_no_batched_grid():
    la, _, X, y = _fit("mlp", "last_layer", False)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(X, y), batch_size=X.shape[0])
    with pytest.raises(NotImplementedError):
        la.validation_loss_grid(loader, torch.logspace(-1, 1, 3))


def test_zz_write_the_report():
    """the worst ratios seen above, for the record: written only by a run that measured every family and every golden (a
    selection of tests leaves the committed report alone)"""
    families = {(lo, ep) for lo in ("ll", "r") for ep in ("cov", "grid")}
    goldens = {("e2e", f"{n}/{s}/{k}") for n, s, k in E2E}
    if not (families | goldens) <= set(_worst):
        return
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    lines = ["# lk_spectral.hip on the device: worst |err| / bound per launch family, and end-to-end errors", "",
             "| family | worst \\|err\\| / derived bound |", "|---|---|"]
    for key in sorted(families):
        lines.append(f"| {key[0]} loader, {key[1]} epilogue | {_worst[key]:.3f} |")
    lines += ["", "Against the fp64 goldens of tests/golden at the golden prior, relative to the largest entry (bar 1e-4):", "",
              "| golden | Cholesky route: f_var, marglik, logdet | spectral route: f_var, marglik, logdet |", "|---|---|---|"]
    for key in sorted(goldens):
        c, s = _worst[key]
        lines.append(f"| {key[1]} | " + ", ".join(f"{e:.2e}" for e in c) + " | " + ", ".join(f"{e:.2e}" for e in s) + " |")
    with open(REPORT, "w") as fh:
        fh.write("\n".join(lines) + "\n")
