"""The table of tests/gram16_fixtures.py reaches EVERY launch form of the split-fp16 Gram engine (laplace_amd/csrc/lk_sweep16.hip) at
the edges of its loops, every claim of a row agrees with the built library's own host functions, and the bit equality of its
``ints`` and ``scale`` rows holds for the kernels' arithmetic while five mutants of that arithmetic fail (CPU only: the kernels
are stood in for by ``gram16_fixtures.emulate``).

A rule that moves in the launchers (the split plan, the tile choice of the pixel-pair tables, their slot order) moves
``lk_gram_tn_f16x2_workspace_bytes`` / ``lk_conv3x3_pixpair_plan`` / ``lk_conv3x3_pixpair_tables`` with it and fails here instead
of silently un-covering a form in tests/test_gpu_gram16_instances.py."""
import ctypes
import os

import numpy as np
import pytest

from tests import gram16_fixtures as gf


@pytest.fixture(scope="module")
def K():
    from laplace_amd._lib import LIB_PATH, HipKernels

    if not os.path.exists(LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return HipKernels()


def on_cpu(row):
    return row["R"] <= gf.CPU_MAX_ROWS


def host_plan(K, row):
    out = (ctypes.c_int64 * 3)()
    a = ctypes.addressof(out)
    rc = K.lib.lk_conv3x3_pixpair_plan(row["H"], row["W"], row["Cin"], ctypes.c_void_p(a), ctypes.c_void_p(a + 8), ctypes.c_void_p(a + 16))
    assert rc == 0, row["name"]
    return int(out[0]), int(out[1]), int(out[2])


def test_the_table_is_well_formed():
    assert len(gf.BY_NAME) == len(gf.ROWS)
    for row in gf.ROWS:
        assert row["form"] in gf.FORMS and row["kind"] in ("ints", "mant", "scale") and row["claim"]["kernel"] == row["form"], row["name"]
        if row["entry"] == "tn":
            assert row["form"] == ("tn64" if row["C"] == 64 else "tn128") and (row["C"] == 64 or row["C"] % 128 == 0), row["name"]
            assert row["R"] * row["C"] <= 262208 * 64, row["name"]  # (the largest operand)
        else:
            assert row["R"] == row["B"] and row["Cin"] % 64 == 0, row["name"]
        if row["kind"] != "ints":
            assert row["launches"] == 1, row["name"]


def test_every_claim_agrees_with_the_host_functions(K):
    for row in gf.ROWS:
        c = row["claim"]
        if row["entry"] == "tn":
            nbytes = int(K.lib.lk_gram_tn_f16x2_workspace_bytes(row["R"], row["C"]))
            per = c["npairs"] * c["nb"] * c["nb"] * 4
            assert nbytes % per == 0 and nbytes // per == c["nsplit"], (row["name"], nbytes, c)
            assert c["nbc"] * c["nb"] == row["C"] and c["rows_per_split"] % c["bkr"] == 0 and c["rows_per_split"] >= 8 * c["bkr"]
            assert (c["nsplit"] - 1) * c["rows_per_split"] < row["R"] <= c["nsplit"] * c["rows_per_split"], row["name"]
            continue
        T, n_tiles, n_blocks = host_plan(K, row)
        assert (T, n_tiles, n_blocks) == (c["tile"], c["n_tiles"], c["n_blocks"]), (row["name"], T, n_tiles, n_blocks)
        assert c["stages"] == -(-row["B"] // c["bkr"]) and (row["form"] == "pix13" or c["bkr"] == (64 if T == 64 else 32))
        tiles = np.zeros((n_tiles, 3), np.int32)
        slots = np.zeros((row["H"] * row["W"], 13), np.int32)
        rc = K.lib.lk_conv3x3_pixpair_tables(row["H"], row["W"], row["Cin"], ctypes.c_void_p(tiles.ctypes.data), ctypes.c_void_p(slots.ctypes.data))
        assert rc == 0
        mine_t, mine_s = gf.pixpair_tables(row["H"], row["W"], row["Cin"])
        assert np.array_equal(tiles, mine_t) and np.array_equal(slots, mine_s), row["name"]
        # a slot exists exactly where the shifted pixel is inside the map, and the slots count the blocks
        want = [[gf.in_map(row["H"], row["W"], y, x, dy, dx) for dy, dx in gf.HALF] for y in range(row["H"]) for x in range(row["W"])]
        assert np.array_equal(slots >= 0, np.array(want)) and sorted(slots[slots >= 0].tolist()) == list(range(n_blocks))


def test_the_host_functions_refuse_what_the_entry_points_refuse(K):
    wb = K.lib.lk_gram_tn_f16x2_workspace_bytes
    assert wb(100, 32) == 0 and wb(100, 192) == 0 and wb(100, 64) > 0 and wb(100, 128) > 0 and wb(0, 64) == 64 * 64 * 4
    out = (ctypes.c_int64 * 3)()
    a = ctypes.addressof(out)
    plan = lambda H, W, C: K.lib.lk_conv3x3_pixpair_plan(H, W, C, ctypes.c_void_p(a), ctypes.c_void_p(a + 8), ctypes.c_void_p(a + 16))  # noqa: E731
    assert plan(3, 3, 64) == 0 and plan(3, 3, 192) == 0 and plan(3, 3, 96) != 0 and plan(0, 3, 64) != 0


def test_the_table_reaches_every_form_and_edge():
    rows = lambda form, kind="ints": [r for r in gf.ROWS if r["form"] == form and r["kind"] == kind]  # noqa: E731
    for kind in ("ints", "mant", "scale"):
        assert {r["form"] for r in gf.ROWS if r["kind"] == kind} == set(gf.FORMS), kind
    # tn64: rows, and the partial counts at the edges of reduce4's loops
    t64 = rows("tn64")
    assert {r["R"] for r in t64} >= {1, 15, 16, 17, 63, 64, 65, 511, 512, 513, 262144, 262208}
    last1 = {r["claim"]["nsplit"] for r in t64 if (r["R"] - 1) % r["claim"]["rows_per_split"] == 0 and r["claim"]["nsplit"] > 1}
    whole = {r["claim"]["nsplit"] for r in t64 if r["R"] % r["claim"]["rows_per_split"] == 0}
    assert last1 >= {2} | set(gf.NSPLIT_EDGES) and whole >= {1, 4, 32, 64, 512}, (last1, whole)
    assert any(r["claim"]["rows_per_split"] > 8 * 64 for r in t64)
    walks = {gf.reduce4_walk(r["claim"]["nsplit"]) for r in t64}
    idle = lambda w: sum(d + t == 0 for d, t in w)  # noqa: E731  waves that sum nothing
    deep = lambda w: sum(d > 0 for d, t in w)  # noqa: E731  waves that enter the eight-deep loop
    assert {idle(w) for w in walks} >= {3, 2, 1, 0}  # 1, 2, 3 partials, and 4 or more
    assert {deep(w) for w in walks} >= {0, 1, 4}  # 28: nobody; 29: wave 0 alone; 32: everybody
    assert gf.reduce4_walk(28) == ((0, 7),) * 4 and gf.reduce4_walk(29) == ((1, 0), (0, 7), (0, 7), (0, 7))
    assert gf.reduce4_walk(32) == ((1, 0),) * 4 and gf.reduce4_walk(33) == ((1, 1), (1, 0), (1, 0), (1, 0)) and gf.reduce4_walk(36) == ((1, 1),) * 4
    assert gf.reduce4_walk(64) == ((2, 0),) * 4 and gf.reduce4_walk(65)[0] == (2, 1) and gf.reduce4_walk(512) == ((16, 0),) * 4
    assert {28, 29, 32, 33, 36, 64, 65, 512} <= {r["claim"]["nsplit"] for r in t64}
    # tn128
    t128 = rows("tn128")
    assert {r["R"] for r in t128 if r["C"] == 128} >= {1, 31, 32, 33, 255, 256, 257}
    assert {r["claim"]["nsplit"] for r in t128 if r["C"] == 128} >= {1, 2, 4, 29, 33}
    assert {(r["C"], r["claim"]["npairs"]) for r in t128} >= {(256, 3), (384, 6), (640, 15), (1024, 36)}
    for C in (256, 384, 640):
        assert any(r["C"] == C and r["claim"]["nsplit"] >= 2 and r["R"] % 32 for r in t128), C
    assert any(r["C"] == 1024 and r["R"] == 40 for r in t128)
    # pixel pairs
    maps = lambda rs: {(r["H"], r["W"]) for r in rs}  # noqa: E731
    p64, p128, p13 = rows("pp64"), rows("pp128"), rows("pix13")
    assert {r["Cin"] for r in p64} == {64, 192, 320} and any(r["Cin"] % 128 == 64 and r["Cin"] > 64 for r in p64)
    assert {r["B"] for r in p64} >= {1, 63, 64, 65, 129} and maps(p64) >= {(1, 1), (1, 3), (3, 1), (2, 2), (3, 3), (5, 7)}
    assert {r["Cin"] for r in p128} == {128, 256, 384}
    assert {r["B"] for r in p128} >= {1, 31, 32, 33, 65} and maps(p128) >= {(1, 1), (1, 3), (3, 1), (2, 2), (3, 3), (5, 7)}
    for rs in (p64, p128):
        assert any(r["claim"]["n_tiles"] % 8 and r["claim"]["n_tiles"] > 8 for r in rs)  # (xcd_tile_order: ragged ranges per XCD)
        assert any(r["launches"] == 2 for r in rs)
    assert {r["B"] for r in p13} >= {1, 15, 16, 17, 32, 33, 48, 49, 64, 100} and {r["claim"]["stages"] for r in p13} >= {1, 2, 3, 4, 7}
    assert maps(p13) >= {(1, 1), (1, 3), (3, 1), (3, 3), (2, 5), (5, 5), (5, 7)} and any(r["launches"] == 2 for r in p13)
    assert any(r["H"] * r["W"] % 8 for r in p13)
    # stacked launches differ in their scale
    for r in gf.ROWS:
        if r["launches"] == 2:
            assert len(set(gf.build(r["name"]).sexp)) == 2, r["name"]
    # scale
    assert {r["sexp"] for r in rows("tn64", "scale")} == set(gf.SCALE_SEXPS) == {-40, 40, 63, 64, 74, 75, 78}
    for form in ("tn128", "pp64", "pp128", "pix13"):
        assert {r["sexp"] for r in rows(form, "scale")} & {63, 75}, form
    # what the CPU tier does not walk
    skipped = [r for r in gf.ROWS if not on_cpu(r)]
    assert 4 * len(skipped) <= len(gf.ROWS)
    for form in gf.FORMS:
        assert sum(on_cpu(r) for r in rows(form)) >= 3, form


def test_the_operands_are_what_the_docstring_says():
    o = gf.build("tn64-R513")
    assert np.abs(o.h.astype(np.float32)).max() == 8 and np.abs(o.l.astype(np.float32)).max() == 3 and o.sexp[0] in gf.SEXPS
    assert abs(np.corrcoef(o.h.astype(np.float64).ravel(), o.l.astype(np.float64).ravel())[0, 1]) < 0.05  # l is not a function of h
    o = gf.build("tn64-mant")
    back = (o.h.astype(np.float64) + o.l.astype(np.float64)) * 2.0 ** -o.sexp[0]
    assert o.sexp == [14] and (np.abs(back - o.x) <= 2.0 ** -22 * np.abs(o.x)).all() and (o.x.view(np.uint32) & 1).any()
    o = gf.build("tn64-scale75")
    assert np.float32(1.0) * np.float32(2.0 ** -75) * np.float32(2.0 ** -75) == 0 and (o.want >= 2.0 ** -126).all()


WORST = {}


@pytest.mark.parametrize("name", [r["name"] for r in gf.ROWS if on_cpu(r)])
def test_the_stand_in_is_exact_on_ints_and_scale_and_inside_the_bound_on_mant(name):
    row, o = gf.BY_NAME[name], gf.build(name)
    got = gf.emulate(row, o)
    assert not np.isnan(got).any()
    if row["kind"] == "mant":
        r = gf.ratio(row, got, o)
        WORST[row["form"]] = r
        print(f"{name}: stand-in error / bound = {r:.4f}  (R = {row['R']}: {r * (3 * row['R'] + 16):.2f} units of 2^-24 M)")
        assert r <= 1.0
        return
    want = o.want.astype(np.float32)
    if row["entry"] == "tn":
        up = gf.upper_tiles(row["C"])
        assert np.array_equal(got[up].view(np.int32), want[up].view(np.int32))
        assert np.array_equal(got[~up].view(np.int32), o.G0[~up].view(np.int32))  # below: untouched
    else:
        assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_print_the_worst_ratio_of_the_honest_stand_in():
    for form, r in sorted(WORST.items()):
        print(f"\n{form:6s} honest stand-in, error / bound {r:.4f}", end="")
    assert not WORST or max(WORST.values()) <= 1.0


def _differs(row, o, got):
    want = o.want.astype(np.float32)
    if row["entry"] == "tn":
        up = gf.upper_tiles(row["C"])
        return not np.array_equal(got[up].view(np.int32), want[up].view(np.int32))
    return not np.array_equal(got.view(np.int32), want.view(np.int32))


def _mutant_breaks(name, mutant):
    row, o = gf.BY_NAME[name], gf.build(name)
    return _differs(row, o, gf.emulate(row, o, mutant=mutant))


@pytest.mark.parametrize("name", ["tn64-R17", "tn128-c256-3pairs", "pp64-c192-1x3-B63", "pp128-c256-2x2-B32", "pix13-3x3-B17"])
@pytest.mark.parametrize("mutant", ["drop_ah_bl", "swap_b_planes"])
def test_mutants_of_the_three_products_break_ints_on_every_form(name, mutant):
    assert _mutant_breaks(name, mutant)


@pytest.mark.parametrize("name", ["tn64-R1", "tn64-R513", "tn128-R257", "tn128-c640-15pairs", "pp64-c64-1x3-B63", "pp128-c128-5x7-B33", "pix13-3x3-B17"])
def test_mutant_reading_the_ragged_last_stage_past_its_end_breaks_ints(name):
    assert _mutant_breaks(name, "overread_last_stage")


@pytest.mark.parametrize("name", ["pix13-1x1-B1", "pix13-1x3-B15", "pix13-5x7-B48"])
def test_mutant_not_skipping_an_out_of_map_shift_breaks_pix13(name):
    assert _mutant_breaks(name, "pix13_no_skip")


def test_an_interior_pixel_has_nothing_to_skip():
    """(what the mutant above cannot show on its own: 5 x 5 has a pixel with all 13 shifts inside the map)"""
    _, slots = gf.pixpair_tables(5, 5, 64)
    assert (slots >= 0).all(axis=1).sum() == 3 and (slots[2 * 5 + 2] >= 0).all()  # (pixels (0..2, 2))


@pytest.mark.parametrize("name,breaks", [("tn64-scale-40", False), ("tn64-scale40", False), ("tn64-scale63", False), ("tn64-scale75", True),
                                         ("tn64-scale78", True), ("tn128-scale75", True), ("pp64-scale63", False), ("pp64-scale75", True), ("pp128-scale75", True),
                                         ("pix13-scale75", True)])
def test_mutant_forming_the_unscale_factor_first_breaks_scale_from_75(name, breaks):
    """alpha 2^-sexp 2^-sexp as ONE fp32 factor is zero from sexp = 75: the scale rows see it (64 .. 74, where it is subnormal,
    depend on the denormal mode and are left to the device)"""
    assert _mutant_breaks(name, "unscale_factor_first") == breaks
