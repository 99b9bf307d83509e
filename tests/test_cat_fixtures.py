"""tests/cat_fixtures.py checked on the CPU: the table of kernel cases reaches every path lk_cat_vjp_nhwc_f32 can take (asked of the
library's own host-only ``lk_cat_variant``), the reference of tests/test_gpu_cat.py tells two wrong kernels from the right one, and
the ReLU end-to-end fixture keeps every pre-activation clear of zero."""
import pytest
import torch

from tests import cat_fixtures as cf

SMALL = [c for c in cf.CASES if not c["huge"] and c["R"] <= 1024]


@pytest.fixture(scope="module")
def K():
    from laplace_amd._lib import LIB_PATH, HipKernels
    import os

    if not os.path.exists(LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return HipKernels()


def _variant(K, c, aligned=None):
    return K.cat_variant(len(c["kinds"]), cf.split_mask(c), c["R"], c["Ct"], c["c0"], c["Cs"], not c["off"] if aligned is None else aligned)


def test_the_table_reaches_every_path(K):
    seen = [(_variant(K, c), c) for c in cf.CASES]
    assert all(v is not None for v, _ in seen)
    assert {v["vec"] for v, _ in seen} == {True, False}
    for vec in (True, False):  # on the vector and on the scalar path: every number of parts, every kind of mix
        sub = [(v, c) for v, c in seen if v["vec"] == vec and c["R"] > 0]
        assert {v["nparts"] for v, _ in sub} == {1, 2, 3, 4}, vec
        full = {(v["nparts"], v["split_mask"] == 0, v["split_mask"] == (1 << v["nparts"]) - 1) for v, _ in sub}
        for n in (1, 2, 3, 4):
            assert (n, True, False) in full and (n, False, True) in full, (vec, n)  # all-fp32 and all-split
            assert n == 1 or (n, False, False) in full, (vec, n)  # mixed
    # what the variant reports is what was asked, and the vector path is exactly "multiples of four and aligned"
    for v, c in seen:
        assert v["nparts"] == len(c["kinds"]) and v["split_mask"] == cf.split_mask(c)
        assert v["vec"] == (not c["off"] and c["Ct"] % 4 == 0 and c["c0"] % 4 == 0 and c["Cs"] % 4 == 0), cf.case_id(c)
        assert not v["wide_index"]
    # one workgroup, several, and a grid that strides (more lanes than 2048 workgroups of 256 hold), on both paths
    blocks = {(v["vec"], min(v["blocks"], 3) if v["blocks"] < 2048 else "full") for v, c in seen if c["R"] > 0}
    for vec in (True, False):
        assert {(vec, 1), (vec, 2), (vec, "full")} <= blocks, blocks
    strided = [c for v, c in seen if v["blocks"] == 2048]
    assert all(c["R"] * (c["Cs"] // 4 if _variant(K, c)["vec"] else c["Cs"]) > cf.GRID_LANES for c in strided) and len(strided) >= 2
    # an unaligned base sends a shape of multiples of four to the scalar path
    assert any(c["off"] and c["Ct"] % 4 == 0 and c["c0"] % 4 == 0 and c["Cs"] % 4 == 0 for c in cf.CASES)
    assert any(c["R"] == 0 for c in cf.CASES) and any(c["huge"] and c["R"] * c["Ct"] > 1 << 31 for c in cf.CASES)
    assert {c["R"] for c in cf.CASES} >= {0, 1, 63, 64, 65, 257, cf.GRID_LANES + 1}
    assert {c["Cs"] for c in cf.CASES} >= {1, 3, 4, 8, 32, 36} and {c["c0"] for c in cf.CASES} >= {0, 3, 4, 32}
    for Cs in (1, 3, 4, 8, 32, 36):
        for c0 in (0, 3, 4, 32):
            assert {c["Ct"] == c0 + Cs for c in cf.CASES if (c["Cs"], c["c0"]) == (Cs, c0)} == {True, False}, (Cs, c0)


def test_the_variant_refuses_what_the_entry_point_refuses(K):
    assert K.cat_variant(0, 0, 8, 8, 0, 8) is None and K.cat_variant(5, 0, 8, 8, 0, 8) is None
    assert K.cat_variant(2, 4, 8, 8, 0, 8) is None  # (a mask bit beyond the parts)
    assert K.cat_variant(1, 0, 8, 8, 4, 5) is None and K.cat_variant(1, 0, 8, 8, 0, 0) is None
    assert K.cat_variant(1, 0, -1, 8, 0, 8) is None and K.cat_variant(1, 0, 1 << 37, 8, 0, 8) is None
    assert K.cat_variant(1, 0, (1 << 37) - 1, 8, 0, 8)["wide_index"]  # (2^38 lanes)
    assert K.cat_variant(3, 5, 9 * 128 * 32 * 32, 192, 160, 32) == {"vec": True, "nparts": 3, "split_mask": 5, "wide_index": False,
                                                                     "blocks": 2048}


@pytest.mark.parametrize("c", SMALL, ids=cf.case_id)
def test_the_data_are_finite_and_not_integers_and_the_reference_is_the_slice_of_the_sum(c):
    gen = torch.Generator().manual_seed(5 + cf.CASES.index(c))
    parts = cf.make_parts(c, gen)
    vals = [cf.part_value(p) for p in parts]
    for v in vals:
        assert v.dtype == torch.float32 and bool(torch.isfinite(v).all())
        assert v.numel() == 0 or bool((v != v.round()).any())
        assert v.numel() == 0 or float(v.abs()[v != 0].min()) > 2.0 ** -100  # (nothing near the subnormals)
    want = cf.vjp_reference(c, parts)
    assert tuple(want.shape) == (c["R"], c["Cs"])
    exact = sum(v.double() for v in vals)[:, c["c0"]:c["c0"] + c["Cs"]]
    if c["R"]:
        assert float((want.double() - exact).abs().max()) <= len(parts) * 2.0 ** -23 * float(sum(v.abs() for v in vals).max())


def test_split_values_are_formed_as_split_tensor_float_forms_them():
    from laplace_amd._lib import SplitTensor

    c = next(c for c in SMALL if c["kinds"] == ("split", "split") and c["R"] > 1)
    for p in cf.make_parts(c, torch.Generator().manual_seed(1)):
        st = SplitTensor(torch.stack([p[0], p[1]]), torch.tensor([p[2]], dtype=torch.int32))
        assert torch.equal(st.float(), cf.part_value(p))


def test_the_mutants_fail_the_check_of_the_table():
    """a kernel that ignores c0 and one that sums in another order: ``torch.equal`` with the reference tells both"""
    failed = {"ignore-c0": [], "reversed": []}
    for c in SMALL:
        gen = torch.Generator().manual_seed(5 + cf.CASES.index(c))
        parts = cf.make_parts(c, gen)
        want = cf.vjp_reference(c, parts)
        for mutant in failed:
            if not torch.equal(cf.vjp_reference(c, parts, mutant), want):
                failed[mutant].append(c)
    # every case with rows and an offset catches the first; every case chosen for it (three or four generic parts) the second
    assert {cf.case_id(c) for c in failed["ignore-c0"]} == {cf.case_id(c) for c in SMALL if c["c0"] > 0 and c["R"] > 0}
    assert [c for c in SMALL if cf.order_matters(c)] and all(c in failed["reversed"] for c in SMALL if cf.order_matters(c))
    assert all(len(c["kinds"]) >= 3 for c in failed["reversed"])  # (a sum of two commutes)


def test_the_emulation_states_the_same_rule_and_its_mutants_bite():
    from laplace_amd._lib import SplitTensor
    from tests.emulated_cat_kernels import EmulatedCatKernels

    c = next(c for c in SMALL if cf.order_matters(c) and c["c0"] > 0 and "split" in c["kinds"] and "f32" in c["kinds"])
    parts = cf.make_parts(c, torch.Generator().manual_seed(9))
    ops = [p.reshape(1, 1, *p.shape) if torch.is_tensor(p) else
           SplitTensor(torch.stack([p[0], p[1]]).reshape(2, 1, 1, *p[0].shape), torch.tensor([p[2]], dtype=torch.int32)) for p in parts]
    want = cf.vjp_reference(c, parts)
    K, word = EmulatedCatKernels(), torch.zeros(1)
    assert torch.equal(K.cat_vjp(ops, c["c0"], c["Cs"], amax=word).reshape(want.shape), want)
    assert torch.equal(word, want.abs().max().reshape(1))
    for flag in ("ignore_c0", "reverse_sum"):
        M = EmulatedCatKernels()
        setattr(M, flag, True)
        assert not torch.equal(M.cat_vjp(ops, c["c0"], c["Cs"]).reshape(want.shape), want), flag


def test_every_relu_of_the_lattice_fixture_decides_clear_of_zero():
    m, X, _ = cf.e2e_fixture("relu")
    gaps = cf.relu_gaps(m, X)
    assert len(gaps) == 10 and sum(n for _, _, n in gaps) > 100000  # (every ReLU of two blocks of two layers, all elements)
    for i, (gap, positive, _) in enumerate(gaps):
        assert gap >= cf.GAP, (i, gap)
        assert 0.25 < positive < 0.75, (i, positive)  # (the masks decide: neither all ones nor all zeros)
    # the lattice: every pre-activation is an odd multiple of h, exactly representable in fp16
    seen = []
    hooks = [mod.register_forward_pre_hook(lambda mod_, inp: seen.append(inp[0].detach())) for mod in m.modules()
             if isinstance(mod, torch.nn.ReLU)]
    with torch.no_grad():
        f = m(X)
    for h in hooks:
        h.remove()
    for z in seen:
        k = z / cf.H_STEP
        assert torch.equal(k, k.round()) and bool((k.abs() % 2 == 1).all()) and float(z.abs().max()) < 2048 * cf.H_STEP
    assert bool(torch.isfinite(f).all()) and float(f.std()) > 0.1
    # the fixture is deterministic
    m2, X2, _ = cf.e2e_fixture("relu")
    assert torch.equal(X, X2) and all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))


def test_the_fixture_networks_are_the_ones_the_issue_names():
    for kind in ("tanh", "relu"):
        m, X, y = cf.e2e_fixture(kind)
        assert tuple(X.shape) == (4, 3, 8, 8) and tuple(y.shape) == (4,) and m.fc.out_features == 5
        cats = sum(isinstance(mod, type(m.layers[0])) for mod in m.layers)
        pools = sum(isinstance(mod, torch.nn.AvgPool2d) for mod in m.modules())
        assert (cats, pools) == (4, 1)


def test_the_block_wise_kron_variance_is_the_oracles():
    """tests/cat_fixtures.functional_variance_kron against the oracle's dense form, on a model small enough for it"""
    from oracle import curvature_oracle as co

    torch.manual_seed(8)
    nn = torch.nn
    m = nn.Sequential(nn.Conv2d(2, 3, 3, 1, 1), nn.Tanh(), nn.Conv2d(3, 4, 2, bias=False), nn.Tanh(), nn.Flatten(),
                      nn.Linear(36, 3)).double()
    X, y = torch.randn(5, 2, 4, 4, dtype=torch.float64), torch.randint(3, (5,))
    Js, _ = co.jacobians(m, X)
    _, kf = co.kfac_ggn(m, X, y, 5, "classification")
    Qs, ls = co.kron_decompose(kf)
    for prior, h in ((0.7, 1.0), (2.5, 0.3)):
        want = co.functional_variance_kron(Js, Qs, ls, prior, h_factor=h)
        got = cf.functional_variance_kron(Js, Qs, ls, prior, h_factor=h)
        assert tuple(got.shape) == tuple(want.shape) and cf.rel(got, want) < 1e-12
