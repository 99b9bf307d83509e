"""tests/attn_fixtures.py checked on the CPU:

* through ``lk_attn_variant`` (pure host code of csrc/lk_attn.hip) the table reaches every launch form of both owner passes - the
  resident and the rebuilt probability block in every instantiation, seeds split over grid.y or not, one and several owner
  blocks, both layouts, causal or not - and both sides of the resident limit;
* the fixtures' copies of the kernel's ``constexpr`` limits agree with the source;
* both fp32 restatements stay inside the analytic bounds on every case; every mutant leaves them somewhere.
"""
import pytest
import torch

from tests import attn_fixtures as af


@pytest.fixture(scope="module")
def variant():
    from laplace_amd._lib import HipKernels

    K = HipKernels()
    return lambda c: K.attn_variant(c["S"], c["B"], c["H"], c["T"], c["D"], c["layout"], c["causal"])


@pytest.fixture(scope="module")
def worked():
    """per case: operands, reference and the two restatements (computed once)"""
    out = []
    for c in af.CASES:
        ops = af.make_operands(c)
        out.append((c, ops, af.reference(c, *ops)))
    return out


def test_constants_match_the_kernel_source():
    have = af.kernel_constants()
    assert have == {"ATTN_BM": af.ATTN_BM, "ATTN_BN": af.ATTN_BN, "ATTN_TILE": af.ATTN_TILE,
                    "ATTN_RESIDENT_MAX_T": af.ATTN_RESIDENT_MAX_T, "ATTN_MAX_D": af.ATTN_MAX_D}
    from laplace_amd._lib import HipKernels

    assert HipKernels.ATTN_RESIDENT_MAX_T == af.ATTN_RESIDENT_MAX_T
    header = open(af.ROOT + "/include/laplace_hip.h").read()
    assert f"#define LK_ATTN_RESIDENT_MAX_T {af.ATTN_RESIDENT_MAX_T}\n" in header


def test_table_reaches_every_launch_form(variant):
    plans = [variant(c) for c in af.CASES]
    assert all(p is not None for p in plans)
    forms = {(p["resident"], p["dp"]) for p in plans}
    assert forms == {(r, dp) for r in (True, False) for dp in (16, 32, 64, 128)}
    for key in ("seed_split", "causal", "resident"):
        for layout in (0, 1):
            assert {p[key] for p in plans if p["layout"] == layout} == {True, False}, (key, layout)
    # seeds: not split with S == 1, split, and NOT split with S > 1 (enough row blocks)
    assert any(not p["seed_split"] and c["S"] > 1 for c, p in zip(af.CASES, plans))
    assert any(p["seed_split"] and p["seeds_per_slice"] > 1 for p in plans) or any(p["seed_split"] for p in plans)
    assert {1, 2, 3, 5} <= {p["owner_blocks"] for p in plans}
    # both sides of the resident limit, in every instantiation beyond it
    Ts = {c["T"] for c in af.CASES}
    assert {af.ATTN_RESIDENT_MAX_T - 1, af.ATTN_RESIDENT_MAX_T, af.ATTN_RESIDENT_MAX_T + 1} <= Ts
    for c, p in zip(af.CASES, plans):
        assert p["resident"] == (c["T"] <= af.ATTN_RESIDENT_MAX_T)
        assert p["dp"] == next(d for d in (16, 32, 64, 128) if c["D"] <= d)
        assert p["owner_blocks"] == -(-c["T"] // af.ATTN_BM)
    # the table the issue asks for
    assert {1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129} <= Ts
    assert {4, 8, 12, 16, 20, 32, 64, 124, 128} <= {c["D"] for c in af.CASES}
    assert {c["H"] for c in af.CASES} >= {1, 3} and {c["S"] for c in af.CASES} >= {1, 2, 9} and {c["B"] for c in af.CASES} >= {1, 2}


def test_variant_refuses_what_lies_outside_the_contract(variant):
    ok = dict(S=2, B=2, H=2, T=5, D=8, layout=0, causal=False)
    assert variant(ok) is not None
    for bad in (dict(D=6), dict(D=132), dict(D=0), dict(T=0), dict(T=1 << 15), dict(S=0), dict(B=-1), dict(H=0), dict(H=1 << 16),
                dict(layout=2), dict(S=1 << 16, B=1 << 15), dict(B=1 << 20, H=1 << 10, T=1 << 10, D=4)):
        assert variant({**ok, **bad}) is None, bad


def test_big_cases_put_the_largest_score_above_the_overflow_threshold(worked):
    big = [(c, ref) for c, _, ref in worked if c["big"]]
    assert len(big) >= 4
    for c, ref in big:
        assert 95.0 <= ref["max_score"] <= 110.0, (af.case_id(c), ref["max_score"])


def test_operands_have_either_sign_and_the_requested_layout(worked):
    for c, (q, k, v, go), _ in worked:
        assert tuple(q.shape) == (c["B"], c["H"], c["T"], c["D"]) and tuple(go.shape) == (c["S"] * c["B"], c["H"], c["T"], c["D"])
        for t in (q, k, v, go):
            assert (t.contiguous() if c["layout"] == 0 else t.transpose(1, 2)).is_contiguous()
        if v.numel() >= 16:
            assert (v > 0).any() and (v < 0).any() and (go > 0).any() and (go < 0).any()


def test_restatements_stay_inside_the_bounds(worked):
    worst = {}
    for c, ops, ref in worked:
        for name, fn in (("rowwise", af.rowwise_fp32), ("blocked", af.blocked_fp32)):
            for out, r in af.ratios(ref, fn(c, *ops)).items():
                assert r <= 1.0, (name, af.case_id(c), out, r)
                worst[(name, out)] = max(worst.get((name, out), 0.0), r)
    print("worst bound ratios:", {f"{n}/{o}": round(r, 4) for (n, o), r in sorted(worst.items())})
    assert max(worst.values()) > 1e-3  # (the bounds are not vacuous: some output uses more than a thousandth of its bound)


@pytest.mark.parametrize("mutant", af.MUTANTS)
def test_every_mutant_leaves_the_bounds(worked, mutant):
    hit = []
    for c, ops, ref in worked:
        if mutant == "strict-causal" and not c["causal"]:
            continue
        r = af.ratios(ref, af.rowwise_fp32(c, *ops, mutant=mutant))
        if max(r.values()) > 1.0:
            hit.append(af.case_id(c))
    assert hit, f"{mutant} passes every case"


def test_t1_is_exact_in_the_reference():
    c = next(c for c in af.CASES if c["T"] == 1 and not c["big"])
    q, k, v, go = af.make_operands(c)
    ref = af.reference(c, q, k, v, go)
    assert torch.equal(ref["dv"], go.double()) and not ref["dq"].any() and not ref["dk"].any()
