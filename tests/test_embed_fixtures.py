"""What the kernel-case table of tests/embed_fixtures.py reaches, proven without a device: through ``lk_embed_variant`` every
vector class, more than one pass over ``d`` and the long-run path of csrc/lk_embed.hip; through two mutant emulations, that
the checks the device tests run (``check_jac_case`` / ``check_diag_case``) notice the two mistakes such a kernel invites.
"""
import pytest
import torch

from tests.embed_fixtures import (EMBED_FIXTURES, KERNEL_CASES, VOCAB, case_P, check_diag_case, check_jac_case, check_quad_case,
                                  draw_ids, make_case)
from tests.emulated_embed_kernels import EmulatedEmbedKernels, run_sums


def _variant(c, kernel):
    """the variant a case takes on the device: what the entry point calls ``aligned`` is decided by the case's pointers"""
    from laplace_amd._lib import HipKernels

    aligned = not c["misalign"]
    if kernel == "jac":
        aligned = aligned and case_P(c) % 4 == 0 and c["col0"] % 4 == 0
    return HipKernels().embed_variant(c["S"], c["B"], c["T"], c["D"], aligned)


def test_table_reaches_every_vector_class_and_the_long_run_path():
    seen = {"vec": set(), "chunks>1": set(), "slots": set()}
    long_runs = []
    for c in KERNEL_CASES:
        for kernel in c["kernels"]:
            v = _variant(c, kernel)
            assert v is not None, c["name"]
            assert v["vec"] == (4 if c["D"] % 4 == 0 and not c["misalign"] and (kernel != "jac" or (case_P(c) % 4 == 0 and c["col0"] % 4 == 0))
                                else 1)
            assert v["lanes"] * v["slots"] == 1024 and v["lanes"] * v["chunks"] * v["vec"] >= c["D"]
            seen["vec"].add((kernel, v["vec"]))
            if v["chunks"] > 1:
                seen["chunks>1"].add((kernel, v["vec"]))
            if kernel == "diag":
                seen["slots"].add(v["slots"])
                _, ids, _ = make_case(c)
                longest = int(torch.bincount(ids[(ids >= 0) & (ids < c["V"])].reshape(-1), minlength=1).max())
                if v["slots"] > 1 and longest > v["slots"]:  # every slot of the workgroup walks a part of one run
                    long_runs.append((c["name"], longest, v["slots"]))
    assert seen["vec"] == {(k, v) for k in ("jac", "diag", "quad") for v in (1, 4)}
    assert {("diag", 1), ("diag", 4)} <= seen["chunks>1"]  # (D = 65 and D = 260: more vectors of d than a workgroup has lanes)
    assert len(seen["slots"]) >= 3 and min(seen["slots"]) == 64  # (16 lanes x 64 slots at the widest)
    assert ("skew_4096", 4096, 512) in long_runs, long_runs
    # a run shorter than the slots (most slots empty) and the single-position run are in the table too
    assert any(c["T"] == 1 for c in KERNEL_CASES) and any(c["ids"] == "distinct" for c in KERNEL_CASES)


def test_table_covers_the_axes_of_the_issue():
    by = lambda k: {c[k] for c in KERNEL_CASES}  # noqa: E731
    assert {1, 7, 64} <= by("T") and {1, 3, 4, 64, 65, 260} <= by("D") and {1, 2, 9} <= by("S") and {1, 3} <= by("B")
    assert {1, 2, 1000} <= by("V") and {"equal", "distinct", "oob", "random"} <= by("ids")
    assert any(c["misalign"] for c in KERNEL_CASES) and any(c["col0"] > 0 for c in KERNEL_CASES)
    base = next(c for c in KERNEL_CASES if c["name"] == "base")
    _, ids, _ = make_case(base)
    assert 0 in ids and base["V"] - 1 in ids
    pad_in = next(c for c in KERNEL_CASES if c["name"] == "pad_in_data")
    assert pad_in["pad"] in make_case(pad_in)[1]
    pad_un = next(c for c in KERNEL_CASES if c["name"] == "pad_unused")
    assert pad_un["pad"] not in make_case(pad_un)[1]
    oob = make_case(next(c for c in KERNEL_CASES if c["name"] == "oob"))[1]
    assert bool((oob >= 5).any()) and bool((oob < 0).any())


@pytest.mark.parametrize("name", EMBED_FIXTURES)
def test_golden_ids_have_the_properties_the_goldens_pin(name):
    ids = draw_ids(name)
    assert ids.shape == (10, 5) and int(ids.max()) < VOCAB[name] and int(ids.min()) >= 0
    assert all(len(set(r.tolist())) < 5 for r in ids)
    if name == "tok_mean":
        assert bool((ids == 0).any())  # (the padding id)


def test_emulation_passes_every_case():
    K = EmulatedEmbedKernels()
    for c in KERNEL_CASES:
        for integer in (True, False):
            if "jac" in c["kernels"]:
                check_jac_case(K, c, "cpu", integer)
            if "diag" in c["kernels"]:
                check_diag_case(K, c, "cpu", integer)
            if "quad" in c["kernels"]:
                check_quad_case(K, c, "cpu", integer)


class DropsSecondOccurrence(EmulatedEmbedKernels):
    """a scatter without the segmented sum: of the positions of a row that hold one id, only the first contributes"""

    def jac_embed(self, g, ids, V, padding_idx, Js, col0):
        B, T = ids.shape
        first = torch.ones_like(ids, dtype=torch.bool)
        for b in range(B):
            seen = set()
            for t in range(T):
                first[b, t] = int(ids[b, t]) not in seen
                seen.add(int(ids[b, t]))
        super().jac_embed(g * first.to(g.dtype)[None, :, :, None], ids, V, padding_idx, Js, col0)


class SumsAcrossSamples(EmulatedEmbedKernels):
    """the diagonal of the batch-summed gradient: runs of one id are added over the samples BEFORE they are squared"""

    def diag_embed(self, g, ids, V, padding_idx, alpha, h):
        R, _ = run_sums(g, ids, V, padding_idx)
        h += alpha * (R.sum(1) ** 2).sum(0).reshape(-1)


def _failing(check, K, kernel):
    failed = []
    for c in KERNEL_CASES:
        if kernel not in c["kernels"]:
            continue
        for integer in (True, False):
            try:
                check(K, c, "cpu", integer)
            except AssertionError:
                failed.append((c["name"], integer))
    return failed


def test_mutant_that_drops_a_repeated_id_fails_the_jacobian_check():
    failed = _failing(check_jac_case, DropsSecondOccurrence(), "jac")
    assert ("T7_equal", True) in failed and ("T7_equal", False) in failed and ("base", True) in failed
    assert ("T7_distinct", True) not in failed and ("T1", False) not in failed  # (no repeats: the mutant is right there)


def test_mutant_that_sums_across_samples_fails_the_diag_check():
    failed = _failing(check_diag_case, SumsAcrossSamples(), "diag")
    assert ("base", True) in failed and ("base", False) in failed and ("skew_4096", False) in failed
    assert ("B1", True) not in failed  # (one sample: nothing to sum across)
