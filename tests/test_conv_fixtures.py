"""The table of tests/conv_fixtures.py reaches EVERY instantiation and structural edge of the split-fp16 convolution engine, and
its tolerance holds for the kernels' arithmetic while three mutants of that arithmetic exceed it (CPU only:
``lk_conv_launch_variant`` is a host function of the built library; the kernels are stood in for by ``conv_fixtures.emulate``).

A rule that moves in the launchers (the occupancy rule, the position-major limit, the window form's eligibility, co-location,
the split tail) moves the query's answer with it — both call the same helpers of csrc/lk_conv.hip — and fails here instead of
silently un-covering a kernel in tests/test_gpu_conv_instances.py."""
import itertools
import os

import pytest

from tests import conv_fixtures as cf


@pytest.fixture(scope="module")
def K():
    from laplace_amd._lib import LIB_PATH, HipKernels

    if not os.path.exists(LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return HipKernels()


def queried(K, family=None):
    for row in cf.ROWS:
        if family and row["family"] != family:
            continue
        row = cf.resolve(row, K)
        for la in cf.launches(row):
            var = cf.variant(K, row, la)
            assert var is not None, row["name"]
            yield row, la, var


def test_every_row_reports_the_variant_it_claims(K):
    n = 0
    for row, la, var in queried(K):
        ex = dict(row["expect"])
        walk = ex.pop("walk", False)
        assert {k: var[k] for k in ex} == ex, (row["name"], var)
        entry = {"plain": "plain", "planes": "planes", "forward": "forward", "vjp": "vjp", "strided": "vjp"}[row["entry"]]
        assert var["epilogue"] == entry, (row["name"], var)
        if row["family"] != "window":
            assert var["kernel"] == ("strided" if row["entry"] == "strided" else "generic"), (row["name"], var)
        if walk or "split_S" in ex:
            assert var["grid"] + 1 <= var["n_tiles"] <= 1.5 * var["grid"], (row["name"], var)
        if "nstage" in row:
            assert len(la["taps"]) * row["Kc"] // 32 == row["nstage"]
        n += 1
    assert n >= len(cf.ROWS)


def test_the_query_refuses_what_the_entry_points_refuse(K):
    q = K.conv_launch_variant
    t1, t9 = [(0, 0, 0)], [(a - 1, b - 1, 3 * a + b) for a in range(3) for b in range(3)]
    assert q(K.CONV_PLAIN, 4, 6, 6, 64, 40, 6, 6, t9)["kernel"] == "generic"
    assert q(K.CONV_PLAIN, 4, 6, 6, 48, 40, 6, 6, t9) is None and q(K.CONV_PLAIN, 0, 6, 6, 64, 40, 6, 6, t9) is None
    assert q(K.CONV_PLAIN, 4, 6, 6, 64, 40, 6, 6, t9 + t1) is None  # ten taps
    assert q(K.CONV_PLAIN, 4, 6, 6, 64, 40, 6, 6, t9, in_nsexp=4) is not None and q(K.CONV_PLAIN, 4, 6, 6, 64, 40, 6, 6, t9, in_nsexp=3) is None
    assert q(K.CONV_VJP, 4, 6, 6, 64, 40, 6, 6, t9, in_nsexp=4) is None and q(K.CONV_VJP, 4, 6, 6, 64, 36, 6, 6, t9) is None
    assert q(K.CONV_PLANES, 4, 6, 6, 64, 40, 6, 6, t9) is None and q(K.CONV_PLANES, 4, 4, 8, 64, 3, 4, 8, t9)["epilogue"] == "planes"
    assert q(K.CONV_BN_ACT, 4, 6, 6, 64, 36, 6, 6, t9) is None and q(K.CONV_BN_ACT, 4, 6, 6, 64, 40, 6, 6, t9, in_nsexp=4)["epilogue"] == "forward"
    assert q(K.CONV_PLAIN, 4, 3, 3, 64, 40, 3, 3, t9, config=2 | 16) is None  # position-contiguous: Ho Wo % 4
    assert q(K.CONV_PLAIN, 4, 6, 6, 64, 40, 6, 6, t9, Hc=3, Wc=3, out_step=2, config=2 | 16) is None  # ... and a dense grid
    assert q(4, 4, 6, 6, 64, 40, 6, 6, t9) is None and q(-1, 4, 6, 6, 64, 40, 6, 6, t9) is None
    s = K.conv_strided_launch_variant
    rows = cf.launches(cf.BY_NAME["strided-co64-pair"])[0]["taps"]
    assert s(5, 3, 3, 32, 64, 6, 6, 2, rows, True)["kernel"] == "strided"
    assert s(5, 3, 3, 32, 64, 6, 6, 2, rows, False) is None  # a tap of a second source that is not there
    assert s(5, 3, 3, 32, 64, 6, 6, 2, rows[9:], True) is None  # classes without taps
    assert s(5, 3, 3, 32, 68, 6, 6, 2, rows, True) is None and s(5, 3, 3, 32, 64, 7, 6, 2, rows, True) is None
    assert s(5, 2, 2, 32, 64, 6, 6, 3, rows, True) is None


def test_the_table_reaches_every_instantiation(K):
    generic = {(v["bm"], v["bn"], v["epilogue"]) for _, _, v in queried(K, "generic")}
    assert generic == set(itertools.product([64, 128, 256], [64, 128], ["plain", "planes", "vjp", "forward"])) - {
        (256, 128, e) for e in ("plain", "planes", "vjp", "forward")}
    win = {(v["kernel"], v["coloc"]) for _, _, v in queried(K, "window") if v["kernel"] != "generic"}
    assert win == set(itertools.product(["window-256", "window-512"], [1, 2, 4])), win
    assert {(v["kernel"], v["split_S"]) for _, _, v in queried(K, "window")} >= set(itertools.product(["window-256", "window-512"], [1, 2, 4]))
    assert {(v["bm"], v["bn"]) for _, _, v in queried(K, "strided")} == {(256, 64), (128, 128)}
    assert {(bool(r.get("pair")), v["bm"]) for r, _, v in queried(K, "strided")} == set(itertools.product([False, True], [256, 128]))
    assert {v["ncls"] for _, _, v in queried(K, "strided")} == {1, 4}


def test_the_table_holds_the_structural_cases(K):
    gen = list(queried(K, "generic"))
    M = lambda r, la: r["N"] * la["Hc"] * la["Wc"]  # noqa: E731
    for bm in (64, 128, 256):
        ms = {(M(r, la) < bm, M(r, la) % bm == bm - 1 and M(r, la) > bm, M(r, la) % bm == 1) for r, la, v in gen if v["bm"] == bm}
        assert {m[0] for m in ms} >= {True} and any(m[1] for m in ms) and any(m[2] for m in ms), bm
    for e in ("plain", "vjp", "forward"):
        cos = {(r["Nc"], v["bn"]) for r, _, v in gen if v["epilogue"] == e}
        assert any(co == 8 for co, _ in cos) and any(co == bn + 8 for co, bn in cos), e
    assert {r["Nc"] for r, _, v in gen if v["epilogue"] == "plain"} >= {1, 3}
    assert {(r["nstage"], v["epilogue"]) for r, _, v in gen if "nstage" in r} == set(itertools.product((1, 2, 3), ("plain", "planes", "vjp", "forward")))
    assert any(r["Kc"] == 96 and len(la["taps"]) == 9 for r, la, _ in gen)
    assert {((r["k"], r["p"]), r["dir"]) for r, _, _ in gen} >= set(itertools.product(
        [((1, 1), (0, 0)), ((3, 3), (1, 1)), ((3, 3), (0, 0)), ((2, 2), (0, 0)), ((1, 3), (0, 1))], ["fwd", "bwd"]))
    ragged = lambda r: (r["H"] + 2 * r["p"][0] - r["k"][0]) % r["s"] or (r["W"] + 2 * r["p"][1] - r["k"][1]) % r["s"]  # noqa: E731
    assert {(la["in_mul"], v["epilogue"]) for r, la, v in gen if ragged(r)} >= {(2, "plain"), (3, "plain"), (2, "forward")}
    # class launches: all four (oh0, ow0) on odd and even sizes
    cls = {(la["oh0"], la["ow0"], r["H"] % 2, r["W"] % 2) for r, la, v in gen if la["out_step"] == 2}
    assert cls == set(itertools.product((0, 1), (0, 1), (0, 1), (0, 1)))
    assert all(not v["dense"] for r, la, v in gen if la["out_step"] == 2)
    assert {(r["H"], r["W"]) for r, _, _ in gen} >= {(1, 1), (1, 9), (9, 1), (3, 5), (7, 7), (17, 17)}
    assert any(r["H"] * r["W"] < v["bm"] and M(r, la) > v["bm"] for r, la, v in gen)       # a tile spans several images
    assert any(r["H"] * r["W"] > v["bm"] == 256 for r, la, v in gen)                      # an image spans several tiles
    # position-major rows on both sides of each limit, per epilogue
    for e in ("plain", "vjp", "forward"):
        pm = {(r["N"], la["Hc"] * la["Wc"], v["pmajor"]) for r, la, v in gen if v["epilogue"] == e}
        assert {(64, 4, True), (63, 4, False), (64, 64, True), (64, 65, False), (64, 81, True), (70, 9, True), (64, 16, True), (64, 16, False)} <= pm, e
        assert any(v["pmajor"] and v["bm"] == 64 and r["N"] == 64 and len(la["taps"]) == 9 for r, la, v in gen if v["epilogue"] == e)
        assert any(v["pmajor"] and r["N"] % v["bm"] and (r["N"] * 2) % v["bm"] for r, la, v in gen if v["epilogue"] == e)  # tiles straddle positions
    assert {bool(r.get("accumulate")) for r, _, v in gen if v["epilogue"] == "plain"} == {False, True}
    assert any(v["out_nchw"] and v["epilogue"] == "plain" for _, _, v in gen)
    assert all((la["Hc"] * la["Wc"]) % 16 == 0 for r, la, v in gen if v["epilogue"] == "planes")
    assert {v["epilogue"] for r, _, v in gen if r.get("per_image")} == {"plain", "planes", "forward"}
    vj = [(r, v) for r, _, v in gen if v["epilogue"] == "vjp"]
    assert {r["vjp"] for r, _ in vj} == set(cf.VJP_VARIANTS)
    assert {(r.get("seeds", 1), bool(r.get("amax"))) for r, _ in vj} >= {(1, False), (2, True), (3, False)}
    assert any(r.get("seeds", 1) == 3 and (r["N"] // 3) * r["H"] * r["W"] < v["bm"] for r, v in vj)  # mask_rows wraps inside a tile
    fw = [r for r, _, v in gen if v["epilogue"] == "forward"]
    assert {(r["act"], r.get("addend", 0), r.get("namax", 1)) for r in fw} >= set(itertools.product((0, 1), (0, 1, "N"), (1, "N"))) - {
        (a, 0, "N") for a in (0, 1)} - {(a, 1, 1) for a in (0, 1)}
    assert any(r.get("mask") is False for r in fw) and any(r.get("planes") is False for r in fw)
    # window form
    win = [(r, v) for r, _, v in queried(K, "window")]
    px = {(r["N"], r["H"], r["W"]) for r, v in win if v["kernel"] != "generic"}
    assert {(32, 4, 4), (32, 2, 8), (32, 1, 16), (32, 16, 1), (11, 1, 47), (6, 2, 47), (21, 5, 5), (2, 20, 20), (2, 17, 17), (1, 24, 24)} <= px
    for kern in ("window-256", "window-512"):
        mine = [(r, v) for r, v in win if v["kernel"] == kern]
        assert {r["Kc"] for r, _ in mine} >= {32, 96} and {r["Nc"] for r, _ in mine} == {64, 128, 192, 256}
        assert {r["vjp"] for r, _ in mine} >= {"none", "add", "mask", "scale", "all"}
        assert {bool(r["config"] & cf.BIT_HALO) for r, _ in mine} == {False, True} and {v["wg_per_cu"] for _, v in mine} == {1, 2 if kern == "window-256" else 1}
        assert any(r["config"] & cf.BIT_COLOC * 3 and v["coloc"] == c for r, v in mine for c in (2, 4))
    assert any(v["kernel"] == "generic" and r["vjp"] == "fmult" for r, v in win)
    st = [(r, v) for r, _, v in queried(K, "strided")]
    assert {r["Nc"] for r, _ in st} >= {8, 64, 72, 136} and {(r["H"], r["W"]) for r, _ in st} >= {(2, 2), (2, 6), (6, 2)}
    assert {r["vjp"] for r, _ in st} >= {"none", "add", "mask", "fmult", "allf"}
    assert any(r["N"] * (r["H"] // 2) * (r["W"] // 2) % v["bm"] and v["nb_m"] > 1 for r, v in st)
    assert any(r.get("x2_scale", 1) / r.get("x_scale", 1) >= 2.0 ** 29 for r, _ in st)


def test_defaults_of_the_benchmark_launches_are_pinned(K):
    """what the occupancy rule and the window form choose for the ResNet-18 (c4) launches at 9 x 128 images, with 256 CUs"""
    N = 9 * 128
    bwd = [(1 - a, 1 - b, 3 * a + b) for a in range(3) for b in range(3)]
    fwd = [(a - 1, b - 1, 3 * a + b) for a in range(3) for b in range(3)]
    pick = lambda v: (v["kernel"], v["bm"], v["bn"], v["pmajor"], v["grid"], v["coloc"], v["split_S"])  # noqa: E731
    want_win = {(64, 32): ("window-256", 256, 64, False, 512, 1, 1), (128, 16): ("window-256", 256, 64, False, 512, 2, 1),
                (256, 8): ("window-256", 256, 64, False, 512, 4, 1), (512, 4): ("window-256", 256, 64, False, 512, 4, 1)}
    for (c, h), want in want_win.items():
        assert pick(K.conv_launch_variant(K.CONV_VJP, N, h, h, c, c, h, h, bwd, have_wc=True, config=2)) == want, (c, h)
    # the same launches without chunk-major weights, and the forward's fused BatchNorm launches: the occupancy rule
    want_gen = {(64, 32): (256, 64, False, 4608), (128, 16): (128, 128, False, 2304), (256, 8): (128, 128, True, 1152),
                (512, 4): (64, 128, True, 1152)}
    for (c, h), want in want_gen.items():
        for entry, taps in ((K.CONV_VJP, bwd), (K.CONV_BN_ACT, fwd)):
            v = K.conv_launch_variant(entry, N, h, h, c, c, h, h, taps, config=2)
            assert (v["kernel"], v["bm"], v["bn"], v["pmajor"], v["grid"]) == ("generic",) + want, (c, h, v)
    # batch 128 (the forward of one minibatch): the deep layers fall back to the smaller tiles
    small = {(64, 32): (256, 64), (128, 16): (64, 128), (256, 8): (64, 64), (512, 4): (64, 64)}
    for (c, h), want in small.items():
        v = K.conv_launch_variant(K.CONV_BN_ACT, 128, h, h, c, c, h, h, fwd, in_nsexp=128, config=2)
        assert (v["bm"], v["bn"]) == want, (c, h, v)
    # the down-sampling blocks: the strided form's tile
    for cin, h in ((64, 32), (128, 16), (256, 8)):
        row = dict(cf.BY_NAME["strided-co64-pair"], Kc=2 * cin, Nc=cin, H=h, W=h, N=N)
        v = cf.variant(K, row, cf.launches(row)[0])
        assert (v["bm"], v["bn"], v["ncls"]) == ((256, 64, 4) if cin == 64 else (128, 128, 4)), (cin, v)


# ---- the tolerance: it holds for the arithmetic, and it is sharp ---------------------------------------------------------------
NAMES = [r["name"] for r in cf.ROWS]


@pytest.mark.parametrize("name", NAMES)
def test_tolerance_holds_for_the_arithmetic_and_is_sharp(K, name):
    """every row through the three-product emulation (rows of more than EMULATED_IMAGES images on their first ones: the walk and
    split-tail rows of the window form, the position-major rows — listed by test_subsampled_rows_are_the_large_ones): within HALF
    the tolerance; with a cross term dropped, one out-of-image tap read from its flat address, or the mask off by one sample: outside"""
    row = cf.resolve(cf.BY_NAME[name], K)
    o = cf.build(row)
    keep = min(row["N"], cf.EMULATED_IMAGES)
    got = cf.emulate(row, o, keep)
    r = cf.ratio(got, o.want[:keep], o.tol[:keep])
    print(f"{name}: emulation / tolerance = {r:.3g}")
    assert r <= 0.5, r
    applied = 0
    for mutant in ("cross", "tap", "mask"):
        bad = cf.emulate(row, o, keep, mutant=mutant)
        if bad is None:
            continue
        applied += 1
        rm = cf.ratio(bad, o.want[:keep], o.tol[:keep])
        assert rm > 1.0, (mutant, rm)
    assert applied >= 1


def test_subsampled_rows_are_the_large_ones(K):
    sub = sorted(r["name"] for r in (cf.resolve(r, K) for r in cf.ROWS) if r["N"] > cf.EMULATED_IMAGES)
    assert all(n.startswith(("pmajor-", "win256-walk", "win512-walk", "win256-split", "win512-split")) for n in sub), sub
    # which mutant applies where: every row with taps that leave the image has the stray tap, every shared mask the shifted one
    for row in cf.ROWS:
        if row["p"] != (0, 0) and row["s"] == 1 and row["N"] != "walk" and row["N"] > 1 and row["H"] * row["W"] > 1:
            assert cf._stray_tap(row, cf.build(row), min(row["N"], cf.EMULATED_IMAGES)) is not None, row["name"]
