"""The fixture table of the norm-tap Jacobian kernel (tests/normtap_fixtures.py) does what tests/test_gpu_normtap.py relies on, and
the host rule of the NHWC sweep for tapped normalisation layers (``SplitSweep.nhwc_norm_taps``) - on the CPU:

* through ``lk_normtap_variant`` (pure host code of csrc/lk_normtap.hip) the table reaches every vector class, the seeds in one
  slice and split over grid.y (also a split slice longer than one pass), and a seed loop that ends one short of, at and one past
  the seeds per pass; an unaligned base turns the wide paths off;
* the emulation (tests/emulated_normtap_kernels.py: by index, in the kernel's order of operations) meets every assertion of the
  device test, and three MUTANTS fail the cases they should: a cotangent that already carries the BatchNorm scale, a dropped low
  plane, ``xhat`` without the mean subtracted;
* with the switch on ``SplitSweep`` admits the end-to-end fixtures and its tap gradients, ``jacobians`` and ``diag`` equal those of
  the NCHW sweep; with it off it gives the old reason verbatim; tapped ``BatchNorm1d``, tapped ``LayerNorm`` and a kernel object
  without the entry point are refused by node and cause;
* the ReLU fixtures keep every pre-activation clear of zero in the float64 forward.
"""
import copy
import os

import pytest
import torch
from torch import nn

from tests import normtap_fixtures as nf
from tests.emulated_normtap_kernels import EmulatedNormtapKernels

SENTINEL = -7.25


@pytest.fixture(scope="module")
def variant():
    from laplace_amd._lib import LIB_PATH, HipKernels

    if not os.path.exists(LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    K = HipKernels()
    return lambda c, aligned=None: K.normtap_variant(c["S"], c["B"], c["L"], c["Ch"], c["affine"],
                                                     not c["off"] if aligned is None else aligned)


def test_the_table_reaches_every_path(variant):
    plans = [variant(c) for c in nf.CASES]
    assert all(p is not None for p in plans)
    for c, p in zip(nf.CASES, plans):
        vec, _, R, SC, tiles = nf.plan(c["Ch"], c["off"])
        assert (p["vec"], p["lane_rows"], p["seeds_per_pass"], p["channel_tiles"]) == (vec, R, SC, tiles), nf.case_id(c)
        assert p["affine"] == c["affine"]
    assert {(p["vec"], p["seed_split"]) for p in plans} == {(v, s) for v in (1, 4, 8) for s in (False, True)}
    assert {p["vec"] for c, p in zip(nf.CASES, plans) if not c["off"]} == {1, 4, 8}
    assert max(p["channel_tiles"] for p in plans) > 1, "no case has more channel vectors than one workgroup spans"
    lanes = {256 // p["lane_rows"] for p in plans}
    assert lanes == {1, 2, 4, 8, 16, 32, 64}, sorted(lanes)  # (every depth of the shuffle tree)
    # a count of channel vectors that is no power of two leaves channel lanes of the workgroup dead
    assert any((c["Ch"] // p["vec"]) & (c["Ch"] // p["vec"] - 1) for c, p in zip(nf.CASES, plans))
    # the seeds a lane loops over: the slice, and the last slice's remainder - for each vector class's seeds per pass
    for vec in (4, 8):
        loops, SC = set(), nf.plan(8 if vec == 8 else 4)[3]
        for c, p in zip(nf.CASES, plans):
            if p["vec"] == vec:
                loops |= {min(p["seeds_per_slice"], c["S"]), c["S"] - (-(-c["S"] // p["seeds_per_slice"]) - 1) * p["seeds_per_slice"]}
        assert {SC - 1, SC, SC + 1} <= loops, (vec, sorted(loops))
    assert [c for c, p in zip(nf.CASES, plans) if p["seed_split"] and p["seeds_per_slice"] > p["seeds_per_pass"]], \
        "no case splits the seeds AND loops more than one pass in a slice"
    # an unaligned base turns the wide paths off for channel counts that would take them
    for ch, wide in ((8, 8), (12, 4), (72, 8)):
        c = next(c for c in nf.CASES if c["off"] and c["Ch"] == ch)
        assert variant(c, True)["vec"] == wide and variant(c, False)["vec"] == 1


def test_the_table_holds_what_the_device_test_lists():
    for i, ch in enumerate(nf.CHANNELS):  # the crossed part: every channel count with the six position counts of ITS lane rows
        mine = nf.CASES[6 * i:6 * i + 6]
        assert all(c["Ch"] == ch for c in mine)
        for j, c in enumerate(mine):
            R = nf.plan(ch, c["off"])[2]
            assert c["L"] == (1, 2, R - 1, R, R + 1, 2 * R + 3)[j], nf.case_id(c)
        assert {c["B"] for c in mine} == {1, 3}
    for sc in (4, 8):
        assert {c["S"] for c in nf.CASES} >= {1, 2, 9, 17, sc - 1, sc, sc + 1}
    assert {c["sexp"] for c in nf.CASES} == {-3, 0, 12}
    assert {c["affine"] for c in nf.CASES} == {False, True} and {c["off"] for c in nf.CASES} == {0, 1}
    assert {(c["wcol"], c["bcol"]) for c in nf.CASES} == {(True, True), (True, False), (False, True)}
    for c in nf.CASES:
        P, w0, b0 = nf.columns(c)
        assert P > 2 * c["Ch"] and max(w0, b0) + c["Ch"] < P


def _run(K, c, aligned=None):
    """the kernel-level assertions of tests/test_gpu_normtap.py on a kernel object -> list of failures"""
    gen = torch.Generator().manual_seed(53 + nf.CASES.index(c))
    aligned = not c["off"] if aligned is None else aligned
    P, w0, b0 = nf.columns(c)
    Ch, bad = c["Ch"], []
    g, x, mu, rstd = nf.make_inputs(c, gen)
    Js = torch.full((c["B"], c["S"], P), SENTINEL)
    K.jac_norm_affine_nhwc(g, x, mu, rstd, c["S"], Js, w0, b0, aligned=aligned)
    Jw, Jb, bw, bb = nf.reference(c, g.planes, g.sexp, x, mu, rstd)
    keep = torch.ones(P, dtype=torch.bool)
    if w0 >= 0:
        keep[w0:w0 + Ch] = False
        if not bool(((Js[..., w0:w0 + Ch].double() - Jw).abs() <= bw).all()):
            bad.append("w")
    if b0 >= 0:
        keep[b0:b0 + Ch] = False
        if not bool(((Js[..., b0:b0 + Ch].double() - Jb).abs() <= bb).all()):
            bad.append("b")
    if not bool((Js[..., keep] == SENTINEL).all()):
        bad.append("sentinel")
    g, x, mu, rstd = nf.make_integer_inputs(c, gen)
    Ji = torch.full((c["B"], c["S"], P), SENTINEL)
    K.jac_norm_affine_nhwc(g, x, mu, rstd, c["S"], Ji, w0, b0, aligned=aligned)
    Jw, Jb, _, _ = nf.reference(c, g.planes, g.sexp, x, mu, rstd)
    if (w0 >= 0 and not torch.equal(Ji[..., w0:w0 + Ch].double(), Jw)) or (b0 >= 0 and not torch.equal(Ji[..., b0:b0 + Ch].double(), Jb)):
        bad.append("integer")
    return bad


@pytest.mark.parametrize("c", nf.CASES, ids=nf.case_id)
def test_the_emulation_meets_the_references(c):
    assert _run(EmulatedNormtapKernels(), c) == []


def _mutant(**kw):
    K = EmulatedNormtapKernels()
    for k, v in kw.items():
        setattr(K, k, v)
    return K


def test_a_cotangent_that_already_carries_the_scale_fails_the_affine_cases():
    for c in nf.CASES:
        bad = _run(_mutant(scaled_cotangent=True), c)
        assert ("w" in bad) == (c["affine"] and c["wcol"]) and ("b" in bad) == (c["affine"] and c["bcol"]), nf.case_id(c)
        assert "integer" not in bad and "sentinel" not in bad  # (rstd = 1 there)


def test_a_dropped_low_plane_fails_every_full_mantissa_case():
    for c in nf.CASES:
        bad = _run(_mutant(drop_low=True), c)
        g = nf.make_inputs(c, torch.Generator().manual_seed(53 + nf.CASES.index(c)))[0]
        low = bool(g.planes[1].any())  # (a single element is cut at the top of the fp16 range: its low plane is zero)
        assert low or c["S"] * c["B"] * c["L"] * c["Ch"] == 1, nf.case_id(c)
        # the low planes are worth ~ 2^-12 sqrt(L) of a sum's magnitude bound and the tolerance (L + 8) 2^-24 of it: the issue's
        # bound tells them apart up to a few hundred positions (2^12 / 64^1.5 = 8 at L = 64), which is where this is asserted
        if c["L"] <= 64:
            assert ("w" in bad) == (c["wcol"] and low) and ("b" in bad) == (c["bcol"] and low), nf.case_id(c)
        assert "integer" not in bad  # (the integer planes have a zero low plane)


def test_xhat_without_the_mean_fails_the_weight_columns_of_the_affine_cases():
    for c in nf.CASES:
        bad = _run(_mutant(no_mean=True), c)
        assert ("w" in bad) == (c["affine"] and c["wcol"]) and "b" not in bad, nf.case_id(c)


# ---- the host rule, on the emulation -------------------------------------------------------------------------------------------------
@pytest.fixture
def nt_kernels():
    from laplace_amd import _lib

    prev = _lib.set_kernels_for_testing(EmulatedNormtapKernels())
    yield
    _lib.set_kernels_for_testing(prev)


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300)).item()


def test_the_default_is_off():
    from laplace_amd import HipGGN
    from laplace_amd.sweep_nhwc import SplitSweep

    assert SplitSweep.nhwc_norm_taps is False and HipGGN.nhwc_norm_taps is False


@pytest.mark.parametrize("name", nf.E2E)
def test_the_split_sweep_admits_the_end_to_end_fixtures_with_the_switch_on_only(nt_kernels, name):
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep_nhwc import SplitSweep

    m64, _, _ = nf.e2e_fixture(name)
    model = copy.deepcopy(m64).float()
    on = SplitSweep(model, nf.e2e_taps(model), kernels=get_kernels, nhwc_norm_taps=True)
    assert on.split_reason is None and on.split_ok
    assert set(nf.norm_names(model)) <= on.tap_names and len(nf.norm_names(model)) in (2, 3, 6)
    off = SplitSweep(model, nf.e2e_taps(model), kernels=get_kernels)
    first = sorted(nf.norm_names(model))[0]
    kind = "BatchNorm" if name != "gnblock" else "GroupNorm"
    assert not off.split_ok and off.split_reason == f"{first}: tapped {kind} (its cotangent is delivered by the NCHW sweep)"


def test_refusals_name_the_node_and_the_cause():
    from laplace_amd import _lib
    from laplace_amd._lib import get_kernels
    from laplace_amd.sweep_nhwc import SplitSweep
    from tests.emulated_pool_kernels import EmulatedPoolKernels

    conv = lambda: [nn.Conv2d(3, 32, 3, padding=1), nn.BatchNorm2d(32), nn.Tanh(), nn.AdaptiveAvgPool2d(1), nn.Flatten()]  # noqa: E731
    bn1d = nn.Sequential(*conv(), nn.Linear(32, 8), nn.BatchNorm1d(8), nn.Tanh(), nn.Linear(8, 3)).eval()
    ln = nn.Sequential(*conv(), nn.Linear(32, 8), nn.LayerNorm(8), nn.Tanh(), nn.Linear(8, 3)).eval()
    bn2d = nn.Sequential(*conv(), nn.Linear(32, 3)).eval()
    prev = _lib.set_kernels_for_testing(EmulatedNormtapKernels())
    try:
        sw = SplitSweep(bn1d, {"6": bn1d[6]}, kernels=get_kernels, nhwc_norm_taps=True)
        assert sw.split_reason == "6: tapped BatchNorm (its cotangent is delivered by the NCHW sweep)"
        sw = SplitSweep(ln, {"6": ln[6]}, kernels=get_kernels, nhwc_norm_taps=True)
        assert sw.split_reason == "6: tapped LayerNorm (its cotangent is delivered by the NCHW sweep)"
        assert SplitSweep(bn2d, {"0": bn2d[0], "1": bn2d[1]}, kernels=get_kernels, nhwc_norm_taps=True).split_ok
        # a BatchNorm without running statistics normalises by the batch: the old reason
        nostats = nn.Sequential(nn.Conv2d(3, 32, 3, padding=1), nn.BatchNorm2d(32, track_running_stats=False), nn.Tanh(),
                                nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(32, 3)).eval()
        sw = SplitSweep(nostats, {"0": nostats[0], "1": nostats[1]}, kernels=get_kernels, nhwc_norm_taps=True)
        assert sw.split_reason == "1: tapped BatchNorm (its cotangent is delivered by the NCHW sweep)"
        _lib.set_kernels_for_testing(EmulatedPoolKernels())  # (the stock emulations have no jac_norm_affine_nhwc)
        sw = SplitSweep(bn2d, {"0": bn2d[0], "1": bn2d[1]}, kernels=get_kernels, nhwc_norm_taps=True)
        assert not sw.split_ok and sw.split_reason == "1: tapped BatchNorm (kernels without the NHWC norm-tap entry point)"
    finally:
        _lib.set_kernels_for_testing(prev)


@pytest.mark.parametrize("name", nf.E2E)
def test_tap_gradients_of_both_sweeps_agree(nt_kernels, name):
    from laplace_amd._lib import SplitTensor, get_kernels
    from laplace_amd.sweep import SeedBatchedSweep
    from laplace_amd.sweep_nhwc import NhwcNormGrad, SplitSweep

    m64, X, _ = nf.e2e_fixture(name)
    model = copy.deepcopy(m64).float()
    taps, S, B = nf.e2e_taps(model), 4, X.shape[0]
    seeds = torch.randn(S, B, nf.E2E_CLASSES, generator=torch.Generator().manual_seed(3))
    ref = SeedBatchedSweep(model, taps, kernels=get_kernels)
    f0 = ref.forward(X.float())
    want = ref.backward(seeds)
    for keep_split in (False, True):
        sw = SplitSweep(model, taps, kernels=get_kernels, nhwc_norm_taps=True)
        assert sw.split_ok, sw.split_reason
        f = sw.forward(X.float())
        grads = sw.backward(seeds, keep_split=keep_split)
        assert _rel(f, f0) < 1e-4 and sw.grad_scale == {}, "grad_scale leaked to a caller that did not ask for it"
        for n, mod in taps.items():
            g = grads[n]
            if isinstance(mod, nf.NORMS):  # norm taps leave in NHWC form whatever keep_split says
                assert isinstance(g, NhwcNormGrad if isinstance(mod, nn.GroupNorm) else SplitTensor), (n, type(g))
                g = SplitSweep.norm_grad_nchw(g, S, B)
            elif isinstance(g, SplitTensor):
                assert keep_split
                g = SplitSweep.norm_grad_nchw(g, S, B)
            assert tuple(g.shape) == tuple(want[n].shape), n
            assert _rel(g, want[n]) < 1e-4, (n, keep_split, _rel(g, want[n]))
    if name != "gnblock":  # a caller that asks for the deferred scale receives it, for the convolutions in front of a BatchNorm
        sw = SplitSweep(model, taps, kernels=get_kernels, nhwc_norm_taps=True)
        sw.forward(X.float())
        grads = sw.backward(seeds, defer_bn_scale=True)
        assert sw.grad_scale
        for n, sc in sw.grad_scale.items():
            assert _rel(grads[n] * sc.reshape(1, 1, -1, 1, 1), want[n]) < 1e-4, n


def _in_two_batches(b, X, y):
    parts = [(*b.jacobians(X[i:i + 2]), b.diag(X[i:i + 2], y[i:i + 2])[1]) for i in range(0, X.shape[0], 2)]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), sum(p[2] for p in parts)


@pytest.mark.parametrize("name", nf.E2E)
def test_jacobians_and_diag_equal_those_of_the_nchw_sweep(nt_kernels, name):
    from laplace_amd import HipGGN
    from laplace_amd.sweep_nhwc import SplitSweep

    m64, X, y = nf.e2e_fixture(name)
    model = copy.deepcopy(m64).float()
    X = X.float()
    on = HipGGN(model, "classification")
    on.nhwc_norm_taps = True
    Js, f, h = _in_two_batches(on, X, y)
    sweep = on._tape().sweeps[frozenset({"norm"})]
    assert isinstance(sweep, SplitSweep) and sweep.split_ok, getattr(sweep, "split_reason", None)
    off = HipGGN(copy.deepcopy(m64).float(), "classification")
    Js0, f0, h0 = _in_two_batches(off, X, y)
    sweep0 = off._tape().sweeps[frozenset({"norm"})]
    assert isinstance(sweep0, SplitSweep) and not sweep0.split_ok and "delivered by the NCHW sweep" in sweep0.split_reason
    assert _rel(f, f0) < 1e-4
    for n, lo, hi in nf.blocks(model):
        assert _rel(Js[..., lo:hi], Js0[..., lo:hi]) < 1e-4, (n, _rel(Js[..., lo:hi], Js0[..., lo:hi]))
        assert _rel(h[lo:hi], h0[lo:hi]) < 1e-4, (n, _rel(h[lo:hi], h0[lo:hi]))
    # the seed-chunked branch of grad_fn hands the norm taps over in the NCHW sweep's form
    on.sweep_max_rows = 4
    Js2, _ = on.jacobians(X)
    assert _rel(Js2, Js0) < 1e-4


@pytest.mark.parametrize("lik", ("classification", "regression"))
def test_the_golden_model_keeps_its_numbers_with_the_switch_on(nt_kernels, lik):
    """``normbn`` has 4-channel convolutions, outside the implicit-GEMM kernels' coverage: whatever the switch says it runs through
    the NCHW sweep, for that reason and not for its BatchNorm, and computes the goldens"""
    from laplace_amd import HipGGN
    from tests.norm_fixtures import golden_model, load_golden

    g = load_golden("normbn", lik)
    model, X, y = golden_model("normbn", g)
    b = HipGGN(model, lik)
    b.nhwc_norm_taps = True
    Js, f = b.jacobians(X)
    _, h = b.diag(X, y)
    sweep = b._tape().sweeps[frozenset({"norm"})]
    assert not sweep.split_ok and sweep.split_reason == "0: convolution outside the implicit-GEMM kernel's coverage"
    assert _rel(Js, torch.as_tensor(g["Js"])) < 1e-4 and _rel(h, torch.as_tensor(g["h_ggn"])) < 1e-4


@pytest.mark.parametrize("name", nf.E2E)
def test_the_relu_fixtures_keep_their_decisions_clear_of_zero(name):
    margin, seen = nf.e2e_relu_margin(name)
    assert seen >= 16384, seen  # (the probes looked at every ReLU of the network)
    assert margin > nf.RELU_MARGIN, f"a float64 pre-activation lies {margin:.2e} from zero: take another seed"
