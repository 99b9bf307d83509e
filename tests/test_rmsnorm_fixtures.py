"""The shape table, reference and bounds of tests/rmsnorm_fixtures.py, proved on the CPU: the table reaches every launch variant of
csrc/lk_rmsnorm.hip (through the host-only lk_rmsnorm_variant), an fp32 evaluation of the formulas holds the bounds on every case,
and the two mutants that turn RMSNorm back into LayerNorm - the centred variance in the forward, the ``- mean_row(t)`` term in the
VJP - fail them on every case.  The emulation of tests/emulated_rmsnorm_kernels.py holds them too."""
import pytest
import torch

from laplace_amd._lib import HipKernels
from tests import rmsnorm_fixtures as rf


def _gen(c):
    return torch.Generator().manual_seed(1000 + rf.CASES.index(c))


def test_constants_are_the_kernels():
    assert rf.kernel_constants() == {"RMS_SC": rf.RMS_SC, "RMS_NV": rf.RMS_NV}


def _variant(c):
    v = HipKernels().rmsnorm_variant(c["S"], c["rows"], c["D"], aligned=not c["off"])
    assert v is not None, c
    return v


def test_the_table_reaches_every_variant():
    seen = {(v["vec"], v["two_pass"], v["seed_split"], v["lanes"]) for v in map(_variant, rf.CASES)}
    lanes = (1, 2, 4, 8, 16, 32, 64)
    for vec in (False, True):
        # every lane group on chip, with the seeds split (few rows)
        assert {(vec, False, True, w) for w in lanes} <= seen, sorted(seen)
        # the two-pass path exists with 64 lanes only; each path with and without the seed split
        for two_pass in (False, True):
            for split in (False, True):
                assert (vec, two_pass, split, 64) in seen, (vec, two_pass, split)
    assert not any(tp and w != 64 for _, tp, _, w in seen)
    # one seed is never split; the numbers of seeds around the pair in flight; an odd count in one slice
    assert {c["S"] for c in rf.CASES} >= {1, rf.RMS_SC, rf.RMS_SC + 1, 9} and {c["rows"] for c in rf.CASES} >= {1, 2, 3, 2048}
    assert all(not _variant(c)["seed_split"] for c in rf.CASES if c["S"] == 1)
    per = {_variant(c)["seeds_per_slice"] for c in rf.CASES}
    assert {1, 2} <= per  # (a slice of one seed: half of the pair in flight is masked; a full pair)


def test_the_edges_of_the_paths_are_where_the_table_puts_them():
    K = HipKernels()
    for vec, mul in ((False, 1), (True, 4)):
        for w in (2, 4, 8, 16, 32, 64):
            assert K.rmsnorm_variant(3, 2, mul * w, aligned=vec)["lanes"] == w
            assert K.rmsnorm_variant(3, 2, mul * (w - 1), aligned=vec)["lanes"] == (w if w > 2 else 1)
            assert K.rmsnorm_variant(3, 2, mul * (w + 1), aligned=vec)["lanes"] == min(2 * w, 64)
        on = rf.ROW_LANES * rf.RMS_NV
        assert not K.rmsnorm_variant(3, 2, mul * on, aligned=vec)["two_pass"]
        assert K.rmsnorm_variant(3, 2, mul * (on + 1), aligned=vec)["two_pass"]
    # a misaligned pointer or a row that is no multiple of four floats takes 4-byte loads
    assert K.rmsnorm_variant(3, 2, 64, aligned=True)["vec"] and not K.rmsnorm_variant(3, 2, 64, aligned=False)["vec"]
    assert not K.rmsnorm_variant(3, 2, 66, aligned=True)["vec"]


@pytest.mark.parametrize("c", rf.CASES, ids=rf.case_id)
def test_fp32_holds_the_bounds_and_the_mutants_fail(c):
    x, g, w = rf.make_inputs(c, _gen(c))
    y, rstd = rf.forward_fp32(x, w)
    dx = rf.vjp_fp32(g, x, rstd, w)
    assert rf.violations(c, y, rstd, dx, x, g, w) == []
    # the forward with LayerNorm's centred variance
    ym, rm = rf.forward_fp32(x, w, mutant="centred")
    bad = rf.violations(c, ym, rm, None, x, g, w)
    assert any(b.startswith("rstd") for b in bad) and (w is not None and c["D"] == 1 or any(b.startswith("y") for b in bad)), bad
    # the VJP that keeps the mean term
    bad = rf.violations(c, None, rstd, rf.vjp_fp32(g, x, rstd, w, mutant="mean-term"), x, g, w)
    assert bad and bad[0].startswith("dx"), bad


@pytest.mark.parametrize("c", [c for c in rf.CASES if c["rows"] <= 3], ids=rf.case_id)
def test_the_emulation_holds_the_bounds(c):
    from tests.emulated_rmsnorm_kernels import EmulatedRmsNormKernels

    K = EmulatedRmsNormKernels()
    x, g, w = rf.make_inputs(c, _gen(c))
    y, rstd = K.rmsnorm_forward(x, w, rf.EPS)
    amax = torch.zeros(1)
    dx = K.rmsnorm_vjp(g.reshape(-1, c["D"]), x, rstd, w, c["S"], amax=amax)
    assert rf.violations(c, y, rstd, dx, x, g, w) == []
    assert float(amax) == float(dx.abs().max())
    assert [s[0] for s in K.seen] == ["rmsnorm_forward", "rmsnorm_vjp"]


def test_the_sweeps_torch_math_is_the_same_rule():
    from laplace_amd.sweep import rmsnorm_forward_math, rmsnorm_vjp_math

    for c in rf.CASES[:12]:
        x, g, w = rf.make_inputs(c, _gen(c))
        y, rstd = rmsnorm_forward_math(x, w, rf.EPS)
        dx = rmsnorm_vjp_math(g.reshape(-1, c["D"]), x, rstd, w, c["S"])
        assert rf.violations(c, y, rstd, dx, x, g, w) == []
