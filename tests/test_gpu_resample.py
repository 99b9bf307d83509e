"""csrc/lk_resample.hip on the device: every case of tests/resample_fixtures.py through the C ABI inside guard bands, with a
NaN-prefilled ``dx``, against the fp64 sum with the SAME fp32 tables to the element-wise bound ``(n + 3) 2^-24 sum |wh ww g|``
(``n``: the element's tap count; the bound holds for any summation order, either factoring and fused multiply-adds); two runs
bit-equal; untapped inputs exactly ``+0.0``.  Both end-to-end fixtures with the switch on and off against fp64 autograd and the
oracle.  Every case prints its worst error / bound (the table of profiles/resample_instances.md)."""
import pytest
import torch

from tests import conv1d_fixtures as cf
from tests import resample_fixtures as rf

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64  # floats on either side of dx
RUN = rf.runnable()


def _operands(c, gen):
    """``(g, packed axes, dx view, whole dx buffer)`` on the device: ``dx`` is cut ``off`` floats into a NaN-filled buffer with
    guard bands (``off % 4 != 0``: an unaligned base - the scalar path)"""
    from laplace_amd._lib import get_kernels

    K, t = get_kernels(), rf.tables(c)
    OH, OW = rf.out_extent(c)
    g = rf.make_g(c, gen).to(DEV)
    axes = tuple(K.resample_pack(*(a.to(DEV) for a in axis), L, OL) for axis, L, OL in ((t.csr_h, c["H"], OH), (t.csr_w, c["W"], OW)))
    n = c["P"] * c["H"] * c["W"]
    buf = torch.full((GUARD + c["off"] + n + GUARD,), float("nan"), device=DEV)
    return K, t, g, axes, buf, buf[GUARD + c["off"]:GUARD + c["off"] + n].view(c["P"], c["H"], c["W"])


def _launch(K, c, g, axes, dx):
    (ph, ih, wh, H, OH, _), (pw, iw, ww, W, OW, _) = axes
    K._rc(K.lib.lk_resample_vjp_f32(g.data_ptr(), c["P"], OH, OW, H, W, ph.data_ptr(), ih.data_ptr(), wh.data_ptr(), pw.data_ptr(),
                                    iw.data_ptr(), ww.data_ptr(), dx.data_ptr(), K._stream(g.device)), "lk_resample_vjp_f32")


@pytest.mark.parametrize("c", RUN, ids=[rf.case_id(c) for c in RUN])
def test_every_case_meets_the_reference_inside_guard_bands(c):
    gen = torch.Generator().manual_seed(5)
    K, t, g, axes, buf, dx = _operands(c, gen)
    assert dx.data_ptr() % 16 == (4 * c["off"]) % 16
    v = K.resample_variant(c["P"], *rf.out_extent(c), c["H"], c["W"], *t.taps, aligned=c["off"] % 4 == 0)
    assert v is not None and v["vec"] == (dx.data_ptr() % 16 == 0 and c["W"] % 4 == 0)
    _launch(K, c, g, axes, dx)
    torch.cuda.synchronize()
    first = dx.clone()
    n = dx.numel()
    assert bool(torch.isnan(buf[:GUARD + c["off"]]).all()) and bool(torch.isnan(buf[GUARD + c["off"] + n:]).all())  # (the guard bands)
    assert not bool(torch.isnan(dx).any())  # (every element written)
    ref, bound, untapped = rf.vjp_reference(g.cpu(), t.csr_h, t.csr_w)
    got = first.cpu()
    err = (got.double() - ref).abs()
    ratio = (err / bound.clamp(min=1e-300))[bound > 0].max().item() if bool((bound > 0).any()) else 0.0
    print(f"{rf.case_id(c)}: worst |dx - ref| / bound = {ratio:.3f}, path {v}")
    assert bool((err <= bound).all()), (ratio, err.max().item())
    zeros = got[untapped.expand_as(got)]
    assert bool((zeros == 0).all()) and not bool(torch.signbit(zeros).any())  # (exactly +0.0)
    dx.fill_(float("nan"))
    _launch(K, c, g, axes, dx)
    torch.cuda.synchronize()
    assert torch.equal(dx, first)  # (one owner per element, a fixed order: the same bits)
    # ... and through the wrapper, which cuts its own output
    assert torch.equal(K.resample_vjp(g, *axes), first)


@pytest.mark.parametrize("kernels_on", [True, False], ids=["kernels", "torch-math"])
@pytest.mark.parametrize("name", sorted(rf.FIXTURES))
def test_fixture_matches_the_oracle_on_the_device(name, kernels_on, monkeypatch):
    """kron, the Kron predictive, diag, full and jacobians against fp64 autograd and the oracle, with the switch on and off"""
    from laplace_amd.sweep import SeedBatchedSweep

    monkeypatch.setattr(SeedBatchedSweep, "use_resample_kernels", kernels_on)
    out = cf.run_curvature_checks(DEV, rf.FIXTURES[name]())
    tape = out["backend"]._tape()
    assert getattr(tape, "sweep_reason", None) is None
    routes = [v for s in tape.sweeps.values() if s for v in getattr(s, "resample_route", {}).values()]
    assert routes and all((v == "kernel") == kernels_on for v in routes), routes
    print(name, "kernels" if kernels_on else "torch math", out["ratios"])


def test_two_jacobian_calls_are_bit_equal_with_the_kernel(monkeypatch):
    """stock bilinear upsampling backward accumulates with atomics; the rule has one owner per element"""
    import copy

    from laplace_amd import HipGGN
    from laplace_amd.nets import FPNSmall
    from laplace_amd.sweep import SeedBatchedSweep

    monkeypatch.setattr(SeedBatchedSweep, "use_resample_kernels", True)
    torch.manual_seed(3)
    model = FPNSmall(10, (32, 32, 64), 32, mode="bilinear").eval().to(DEV)
    X = torch.randn(8, 3, 16, 16, device=DEV)
    backend = HipGGN(copy.deepcopy(model), "classification")
    (Ja, fa), (Jb, fb) = backend.jacobians(X), backend.jacobians(X)
    routes = backend._tape().sweep.resample_route
    assert routes and set(routes.values()) == {"kernel"}
    assert torch.equal(Ja, Jb) and torch.equal(fa, fb)
