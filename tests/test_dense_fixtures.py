"""The dense fixtures (tests/dense_fixtures.py) on the CPU: a plain float32 evaluation of the kernels' formulas -- the
last-layer GGN with its class-diagonal blocks as Gram(sqrt(p_j s_j) Pt) -- sits inside every bound that tests/test_gpu_dense.py
asks of the device; the case tables reach every launch form of the C entry points; each mutant leaves the bounds on at
least one case of each check it touches; and the subtracting form of the GGN, Gram(sqrt(p_j) Pt) - Gram(p_j Pt) in fp32,
leaves them on the saturated batches."""
import pytest
import torch

from tests import dense_fixtures as DF

K32 = DF.Fp32Kernels()


@pytest.mark.parametrize("check", DF.CHECKS)
def test_plain_fp32_meets_every_bound(check):
    res = getattr(DF, check)(K32, DF.cpu_dev)
    for name, r in res.items():
        print(f"{check} {name}: {r:.4f}")
    bad = {n: r for n, r in res.items() if not DF.ok(r)}
    assert not bad, bad


@pytest.mark.parametrize("mutant", list(DF.MUTANTS), ids=lambda m: m.__name__)
def test_mutants_leave_the_bounds(mutant):
    for check in DF.MUTANTS[mutant]:
        res = getattr(DF, check)(mutant(), DF.cpu_dev)
        out = [n for n, r in res.items() if not DF.ok(r)]
        print(f"{mutant.__name__} {check}: {len(out)} of {len(res)} cases outside")
        assert out, f"{mutant.__name__} passes every case of {check}"


def test_subtracting_ggn_leaves_the_bounds_on_saturated_batches():
    """every saturated batch is outside, on the elements and on the eigenvalue condition at once somewhere;
    the regression cases, which have nothing to subtract, stay inside"""
    sat = [c for c in DF.LL_CASES if c["kind"] in DF.SATURATED]
    res = DF.check_ll_ggn(DF.SubtractingGGN(), DF.cpu_dev, sat)
    figs = dict(DF.LL_FIGURES)
    for c in sat:
        el, eig, neg = figs[DF.ll_id(c)]
        print(f"{DF.ll_id(c)}: element {el:.3g} eigenvalue {eig:.3g} negative diagonal entries {neg}")
    big = [DF.ll_id(c) for c in sat if not c["base"]]  # (a start of magnitude 1 hides entries of 1e-5)
    assert big and all(not DF.ok(res[n]) for n in big), {n: res[n] for n in big}
    assert any(figs[n][0] > 1e2 for n in big), "the cancellation is orders of magnitude, not a rounding"
    assert any(figs[n][1] > 1 for n in big), "the eigenvalue condition sees it too"
    reg = [c for c in DF.LL_CASES if c["kind"] == "regression"]
    assert all(DF.ok(r) for r in DF.check_ll_ggn(DF.SubtractingGGN(), DF.cpu_dev, reg).values())


def test_inputs_are_fp32_numbers():
    for c in DF.LL_CASES:
        r = DF.ll_reference(c)
        for t in (r["phi"], r["p32"], r["H0"]):
            assert t is None or torch.equal(t, t.float().double())
        if c["kind"] == "one_class":
            assert not r["H"].any() or c["base"]
            assert not r["bound"].any(), "C = 1 with probabilities: every entry is exactly 0"
    for c in DF.QF_CASES:
        r = DF.qf_reference(c)
        assert torch.equal(r["Sigma"], r["Sigma"].float().double()) and torch.equal(r["Sigma"], r["Sigma"].T)
    sat = DF.ll_reference(next(c for c in DF.LL_CASES if c["kind"] == "correct30" and c["B"] == 130 and c["C"] == 10))
    assert sat["p32"].max() > 1 - 1e-6, "saturated rows: the largest probability rounds to within an ulp of 1"


def test_tables_reach_every_launch_form():
    # ll_ggn_full: both paths, every B, C and D~ of the issue, alpha != 1, a non-zero start, C = 1 with probabilities
    assert {DF.ll_form(c)[0] for c in DF.LL_CASES} == {"regression", "classification"}
    cls = [c for c in DF.LL_CASES if c["kind"] in DF.LL_KINDS]
    assert {c["B"] for c in cls} == {1, 5, 130} and {c["C"] for c in cls} == {2, 3, 10}
    assert {c["D"] + c["bias"] for c in cls} == {1, 16, 17, 33} and {c["bias"] for c in cls} == {True, False}
    assert {c["kind"] for c in cls} == set(DF.LL_KINDS)
    for kind in DF.LL_KINDS:
        assert any(c["kind"] == kind and (c["B"], c["C"], c["D"], c["bias"]) == (130, 10, 32, True) for c in cls)
    assert any(c["kind"] == "one_class" for c in DF.LL_CASES) and any(c["C"] == 1 and c["kind"] == "regression" for c in DF.LL_CASES)
    assert any(c["alpha"] != 1 for c in DF.LL_CASES) and any(c["base"] for c in DF.LL_CASES)
    # dense_quadform_ll: one tile and two, a full and a partial last tile, one / two / three q-steps, partial p-chunks, and
    # the 128 / 129 edges with more than one class
    forms = [DF.qf_form(c) for c in DF.QF_CASES]
    assert {f[0] for f in forms} == {1, 2} and {f[1] for f in forms} >= {1, 127, 128}
    assert {f[3] for f in forms} == {1, 2, 3} and {f[4] for f in forms} >= {1, 15, 16}
    assert {c["B"] for c in DF.QF_CASES} == {1, 127, 128, 129} and {c["C"] for c in DF.QF_CASES} == {1, 2, 3, 10}
    assert {c["D"] + c["bias"] for c in DF.QF_CASES} == {1, 15, 16, 17, 33, 128, 129, 257}
    assert {c["delta"] for c in DF.QF_CASES} == {1e-4, 1.0, 1e4}
    for B in (128, 129):
        assert any(c["B"] == B and c["C"] > 1 for c in DF.QF_CASES)
    for Dt in (128, 129):
        assert any(c["D"] + c["bias"] == Dt and c["C"] > 1 for c in DF.QF_CASES)
    assert any(c["kind"] in DF.SATURATED for c in DF.QF_CASES)
    # jac_last_layer: float4 and scalar stores, one trip and two, C = 1, with and without a bias
    forms = {DF.jll_form(*c) for c in DF.JLL_CASES}
    assert forms == {(True, 1), (False, 1), (False, 2)} or forms == {(True, 1), (False, 1), (True, 2), (False, 2)}
    assert DF.jll_form(96, 10, 512, True)[1] == 2
    assert any(c[1] == 1 for c in DF.JLL_CASES) and {c[3] for c in DF.JLL_CASES} == {True, False}
    # diag_ggn_linear
    forms = [DF.dg_form(c) for c in DF.DG_CASES]
    assert {f[0] for f in forms} == {1, 2, 3} and {f[1] for f in forms} == {1, 63, 64, 2}
    assert {f[2] for f in forms} == {1, 2, 3} == {f[3] for f in forms} and {f[4] for f in forms} == {True, False}
    assert {c["Di"] for c in DF.DG_CASES} == {1, 15, 16, 17, 33} == {c["Do"] for c in DF.DG_CASES}
    assert {c["S"] for c in DF.DG_CASES} == {1, 3}
    assert any(c["start"] and c["hb"] for c in DF.DG_CASES) and any(c["start"] and not c["hb"] for c in DF.DG_CASES)
    # jac_linear: one trip and two, with and without the bias columns
    assert {DF.jlin_form(c[2], c[3], c[5]) for c in DF.JLIN_CASES} >= {(1, True), (1, False), (2, True)}
    # jac_conv: L = 1, partial and whole chunks of L and Dk, two blocks of Do, with and without the bias column
    forms = [DF.cv_form(c) for c in DF.CV_CASES]
    assert {f[0] for f in forms} >= {1, 2, 4} and {f[1] for f in forms} >= {1, 9, 16} and {f[3] for f in forms} >= {9, 11, 16}
    assert {f[4] for f in forms} == {1, 2} and {f[5] for f in forms} == {True, False}
    assert {c["Do"] for c in DF.CV_CASES} >= {1, 17} and any(c["d"] == (2, 2) for c in DF.CV_CASES)
    assert any(c["s"] == (2, 2) for c in DF.CV_CASES) and any(2 * c["p"][0] > c["k"][0] for c in DF.CV_CASES)
    # sq_colsum: no launch, one workgroup and two; no row, one, several
    assert {DF.sq_form(c[0], c[1]) for c in DF.SQ_CASES} == {(w, r) for w in (0, 1, 2) for r in (0, 1, 7)}
    assert any(c[2] > 0 and c[3] > 0 for c in DF.SQ_CASES) and any(c[4] for c in DF.SQ_CASES)
    # vjp_scale_mask: each reason gives the form it names, for every multiplier kind
    by = {}
    for c in DF.VJP_CASES:
        by.setdefault(c["reason"], set()).add((DF.vjp_form(c), c["m"], c["scale"], c["g2"]))
    combos = {(m, s, g2) for m in DF.M_KINDS for s in (True, False) for g2 in (True, False)}
    assert {x[1:] for x in by["vec"]} == combos and {x[0] for x in by["vec"]} == {("vec", 1)}
    assert {x[0] for x in by["vec-many"]} == {("vec", 2)} and {x[0] for x in by["per%4"]} == {("scalar", 1)}
    assert {(x[0][0], x[2]) for x in by["hw%4"]} == {("scalar", True), ("vec", False)}
    assert {(x[0], x[2]) for x in by["hw%4-many"]} == {(("scalar", 5), True), (("vec", 2), False)}
    for r in ("mis-g", "mis-g2", "mis-out", "mis-m"):
        assert {x[0] for x in by[r]} == {("scalar", 1)}, r
    assert {x[1] for x in by["mis-m"]} == {"bool", "u8", "float"}
    assert {x[0] for x in by["mis-g-many"]} == {("scalar", 5)}
    assert {x[0] for x in by["S0"]} == {(None, 0)} == {x[0] for x in by["per0"]}
    # bn_act_forward
    by = {}
    for c in DF.BN_CASES:
        by.setdefault(c["reason"], set()).add(DF.bn_form(c))
    assert by["vec"] == {("vec", 1, True), ("vec", 1, False)} and by["vec-many"] == {("vec", 2, True), ("vec", 2, False)}
    assert by["hw%4"] == {("scalar", 1, True), ("scalar", 1, False)} and {f[:2] for f in by["hw%4-many"]} == {("scalar", 5)}
    for r in ("mis-x", "mis-y", "mis-addend"):
        assert by[r] == {("scalar", 1, True), ("scalar", 1, False)}, r
    assert by["mis-mask"] == {("scalar", 1, True)}


def test_figures_react_to_damage():
    ref, bound = torch.tensor([1.0, 0.0]).double(), torch.tensor([1e-6, 0.0]).double()
    assert DF.ratio(ref.clone(), ref, bound) == 0
    assert DF.ratio(torch.tensor([1.0 + 2e-6, 0.0], dtype=torch.float64), ref, bound) == pytest.approx(2.0, rel=1e-3)
    assert DF.ratio(torch.tensor([1.0, 1e-40]).double(), ref, bound) == float("inf"), "an expected zero must come back as zero"
    r = DF.ratio(torch.tensor([float("nan"), 0.0]).double(), ref, bound)
    assert r != r and not DF.ok(r)
    w = torch.tensor([1.0, float("nan")])
    assert DF.same(w.clone(), w) == 0 and DF.same(torch.tensor([1.0, 0.0]), w) == float("inf")


@pytest.mark.parametrize("kind", list(DF.MODEL_SCALES))
def test_model_check_on_the_cpu(kind):
    """the model-level check of tests/test_gpu_dense.py with the fp32 softmax and the plain fp32 GGN in the backend's place:
    inside the bound; with the subtracting GGN the saturated model is outside it and below the eigenvalue condition"""
    def batch_of(K):
        P = DF.MODEL_C * (DF.MODEL_D + 1)
        return lambda X, y, phi, f: K.ll_ggn_full(phi.float(), torch.softmax(f.float(), 1), DF.MODEL_C, True, 1.0, torch.zeros(P, P))

    r, lam, nb, neg, ld, ld_want = DF.model_figures(kind, batch_of(K32))
    print(f"model {kind}: element error / bound {r:.4f}, lambda_min {lam:.3e}, ||bound||_F {nb:.3e}")
    assert DF.ok(r) and lam >= -nb and neg == 0 and abs(ld - ld_want) <= 1e-4 * abs(ld_want)
    r, lam, nb, neg, ld, ld_want = DF.model_figures(kind, batch_of(DF.SubtractingGGN()))
    if kind == "saturated":
        assert r > 1e3 and lam < -nb
    else:
        assert DF.ok(r)
