"""The Kron-algebra fixtures (tests/kronalg_fixtures.py) are well-posed for fp32: a plain torch-float32 evaluation of the
same formulas on the CPU -- fp64 only for the final scalar reduction of the logdets, as the kernels do -- meets, on every
case, the bound that tests/test_gpu_kron_spectra.py asks of the device, so a failure there is the kernel's, not the
input's."""
import pytest
import torch

from tests import kronalg_fixtures as KF

K32 = KF.Fp32Kernels()


def _assert(w):
    assert w, "nothing was measured"
    for name, value in w.items():
        print(f"{name}: {value:.2e} (bound {KF.bound_of(name):g})")
    for name, value in w.items():
        assert value < KF.bound_of(name), (name, value)


@pytest.mark.parametrize("n1,n2", KF.SIZES)
@pytest.mark.parametrize("family", KF.FAMILIES)
def test_pow_and_logdet(family, n1, n2):
    _assert(KF.check_pow(K32, KF.cpu_f32, family, n1, n2))
    _assert(KF.check_logdet(K32, KF.cpu_f32, family, n1, n2))


@pytest.mark.parametrize("scale", [None, 2.0 ** -10, 5e4])
def test_logdet_blocks(scale):
    _assert(KF.check_logdet_blocks(K32, KF.cpu_f32, scale))


@pytest.mark.parametrize("pi,po", KF.SANDWICH_SIZES)
@pytest.mark.parametrize("family", KF.FAMILIES)
def test_sandwich(family, pi, po):
    _assert(KF.check_sandwich(K32, KF.cpu_f32, family, pi, po))


@pytest.mark.parametrize("shape", KF.LINEAR_SHAPES, ids=str)
@pytest.mark.parametrize("family", KF.FAMILIES)
def test_linear_quadforms(family, shape):
    _assert(KF.check_quad_linear(K32, KF.cpu_f32, family, shape))
    _assert(KF.check_grid_linear(K32, KF.cpu_f32, family, shape))


@pytest.mark.parametrize("shape", KF.SHARED_SHAPES, ids=str)
@pytest.mark.parametrize("family", KF.FAMILIES)
def test_shared_quadforms(family, shape):
    _assert(KF.check_quad_shared(K32, KF.cpu_f32, family, shape))


def test_the_spectra_are_what_they_say():
    for fam in KF.FAMILIES:
        for k in KF.SCALES:
            lam = KF.eigs(fam, 65, k)
            assert lam.dtype == torch.float64 and torch.equal(lam, lam.float().double()) and bool((lam >= 0).all())
            assert torch.equal(lam, KF.eigs(fam, 65, 0) * 2.0 ** k), "a power of two moves nothing else"
    assert bool((KF.eigs("zero", 33) == 0).all())
    ones = KF.eigs("ones", 33)
    assert abs(ones[-1].item() - 33) < 1e-5 and bool((ones[:-1] == 0).all()), "rank 1, exact zeros"
    g = KF.eigs("graded", 65)
    assert g.max() / g[g > 0].min() > 1e5
    blocks, deltas = KF.logdet_blocks_case()
    assert len(blocks) > 32 and {len(b) for b in blocks} == {1, 2} and set(deltas.tolist()) == {float(KF.delta_t(d)) for d in KF.DELTAS}
    s, z = KF.sample_scales(9, True)
    assert s[z] == 0 and s.max() == 2.0 ** 20 and s[s > 0].min() == 2.0 ** -20


def test_metrics_see_a_wrong_sample():
    want = torch.tensor([1.0, 1e-12, 0.0], dtype=torch.float64)
    assert KF.elem_err(want, want) == 0
    assert KF.elem_err(want * torch.tensor([1, 1 + 1e-3, 1]), want) == pytest.approx(1e-3, rel=1e-3)
    assert KF.elem_err(want + torch.tensor([0, 0, 1e-40]), want) == float("inf")
    w = KF.Worst()
    w.see("a", 1e-7), w.see("a", 3e-7), w.see("a", 2e-7)
    assert w["a"] == 3e-7
    w.see("a", float("nan")), w.see("a", 1.0)
    assert w["a"] != w["a"], "NaN sticks"
