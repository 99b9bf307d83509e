"""The table of tests/gram_fixtures.py reaches EVERY launch form of the fp32 Gram engine (laplace_amd/csrc/lk_gram.hip), and its
bit-equality / bound hold for the kernels' arithmetic while three mutants of that arithmetic fail (CPU only:
``lk_gram_launch_variant`` is a host function of the built library; the kernels are stood in for by ``gram_fixtures.emulate``).

A rule that moves in the launchers (the tile choice, the split-K cost rule, the direct-epilogue rule, the NTB rule, the reduction
shapes) moves the query's answer with it — both call the same helpers — and fails here instead of silently un-covering a kernel
in tests/test_gpu_gram_instances.py."""
import os

import numpy as np
import pytest

from tests import gram_fixtures as gf


@pytest.fixture(scope="module")
def K():
    from laplace_amd._lib import LIB_PATH, HipKernels

    if not os.path.exists(LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return HipKernels()


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = gf.build(gf.BY_NAME[name])
        return cache[name]

    return get


def queried(K):
    for row in gf.ROWS:
        var = gf.variants(K, row)
        assert all(v is not None for v in var), row["name"]
        yield row, var


def test_every_row_reports_the_variant_it_claims(K):
    for row, var in queried(K):
        assert len(var) == len(row["expect"])
        for v, ex in zip(var, row["expect"]):
            assert {k: v[k] for k in ex} == ex, (row["name"], v)


def test_the_table_reaches_every_form(K):
    inst = {"ints": set(), "mant": set()}
    epilogues, sq_slabs, rpw_sq, rpw_rect, vec1_causes, wide_n = set(), set(), set(), set(), set(), set()
    persist, empty_split, ragged = set(), False, False
    for row, var in queried(K):
        for v in var:
            inst[row["kind"]].add((v["mode"], v["vec"], v["cfg"]))
            if row["kind"] != "ints":
                continue
            if v["mode"] == "XCORR":
                rpw_rect.add(v["rpw"])
            elif v["mode"] != "TNP":
                mirrored = not (row["flags"] & gf.UPPER)
                epilogues.add((v["epilogue"], mirrored) if v["epilogue"] == "slabs" else v["epilogue"])
                if v["epilogue"] == "direct":
                    epilogues.add(("direct", v["cfg"]))
                if v["epilogue"] == "slabs":
                    if mirrored:
                        rpw_sq.add(v["rpw"])
                    else:
                        assert v["nsplit"] > 1  # (upper-only with one split is the direct epilogue)
                    sq_slabs.add(1 if v["nsplit"] == 1 else ("2..32" if v["nsplit"] <= 32 else v["nsplit"]))
                    if v["nsplit"] > 1 and (v["nchunks"] % v["chunks_per_split"]) and (gf.rows_count(row) % v["BK"]) and row["entry"] == "tn":
                        ragged = True
                if v["epilogue"] == "persist":
                    persist.add(v["mode"])
                if v["cfg"] == "WIDE":
                    wide_n.add((v["mode"], row["n"]))
        v = var[0]
        if row["kind"] == "ints" and row["entry"] == "tn":
            if v["vec"] == 1:
                # (the single cause of the row: a row named for ldx or the offset has n % 4 == 0 and nothing else against it)
                vec1_causes.add("n" if row["n"] % 4 else ("ldx" if row["ldx"] % 4 else "offset"))
                assert row["n"] % 4 or (row["ldx"] % 4 != 0) + (row["off"] != 0) == 1, row["name"]
        if row["entry"] == "xcorr" and row["kind"] == "ints":
            vs = var[1]
            if vs["nsplit"] > 1 and -(-row["B"] // vs["BK"]) <= vs["chunks_per_split"]:  # a corner region: B rows
                empty_split = True
    assert inst["ints"] == gf.REQUIRED_INSTANCES, inst["ints"] ^ gf.REQUIRED_INSTANCES
    assert inst["mant"] == gf.REQUIRED_INSTANCES, inst["mant"] ^ gf.REQUIRED_INSTANCES
    assert epilogues == {("slabs", True), ("slabs", False), "direct", "persist", ("direct", "SMALL"), ("direct", "BIG"), ("direct", "WIDE")}
    assert persist == {"TN", "NTB"}
    assert sq_slabs == {1, "2..32", 33, 64}, sq_slabs
    assert rpw_sq == {4, 64} and rpw_rect == {4, 64}
    assert vec1_causes == {"n", "ldx", "offset"}
    assert {n for _, n in wide_n} == {576, 768} and {m for m, _ in wide_n} == {"TN", "NT", "NTB", "CONV"}
    assert empty_split and ragged
    assert {r["n"] for r in gf.ROWS if r["entry"] == "tn" and r["kind"] == "ints"} >= set(gf.N_EDGES)
    assert any(r["entry"] == "tn" and r["ldx"] > r["n"] and r["ldx"] % 4 == 0 for r in gf.ROWS)
    nts = [r for r in gf.ROWS if r["entry"] == "nt" and r["kind"] == "ints"]
    assert {r["L"] for r in nts} >= {1, 15, 16, 17, 100} and {r["nseg"] for r in nts} >= {1, 2, 16}
    assert any(r["mis"] is not None for r in nts) and any(r["nb"] == 0 for r in nts)
    assert {(r["H"], r["W"]) for r in gf.ROWS if r["entry"] == "xcorr"} >= {(2, 2), (2, 40), (17, 3), (2, 64)}
    cv = [r for r in gf.ROWS if r["entry"] == "conv" and r["kind"] == "ints"]
    assert any(r["k"] == (1, 1) for r in cv) and any(r["k"][0] > r["H"] for r in cv) and any(gf.conv_out_hw(r) == (1, 1) for r in cv)
    assert any(r["k"][0] != r["k"][1] and r["s"][0] != r["s"][1] and r["d"][0] != r["d"][1] for r in cv)


def test_k_edges_are_all_reached(K):
    """K in {0, 1, BK - 1, BK, BK + 1} for both chunk depths (64: the 64-tile, 16: the 128-tile) among the TN rows"""
    seen = {16: set(), 64: set()}
    for row, var in queried(K):
        if row["entry"] == "tn" and row["kind"] == "ints":
            seen[var[0]["BK"]].add(row["K"])
    for bk, ks in seen.items():
        assert {0, 1, bk - 1, bk, bk + 1} <= ks, (bk, sorted(ks))


def test_the_query_refuses_what_the_entry_points_refuse(K):
    q = K.gram_launch_variant
    assert q(gf.TN, 8, 16)["mode"] == "TN" and q(gf.TN, 8, 0) is not None
    assert q(gf.TN, 8, -1) is None and q(gf.TN, 1 << 30, 16) is None and q(gf.TN, 1 << 20, 16) is not None
    assert q(gf.TN, 0, 16) is None  # (accepted by the entry point, but nothing is launched)
    assert q(gf.NT, 8, 4, 0) is None and q(gf.NT, 8, 4, 1 << 30) is None and q(gf.NT, 8, 0, 4) is not None
    assert q(gf.CONV, 36, (1 << 31) - 64) is None and q(gf.CONV, 36, (1 << 31) - 65) is not None
    assert q(gf.XCORR_FULL, 8, 0) is None and q(gf.XCORR_STRIPS, 671089, 4) is None and q(gf.XCORR_STRIPS, 671088, 4) is not None
    assert q(5, 8, 16) is None and q(-1, 8, 16) is None
    # the rules the launchers share with it
    assert q(gf.TN, 8, 16, vec4_ok=False)["vec"] == 1 and q(gf.TN, 6, 16)["vec"] == 1
    assert q(gf.NT, 8, 4, 16)["mode"] == "NTB" and q(gf.NT, 8, 4, 16, vec4_ok=False)["mode"] == "NT" and q(gf.NT, 8, 4, 18)["mode"] == "NT"
    assert q(gf.TN, 576, 100, flags=1)["epilogue"] == "direct" and q(gf.TN, 576, 100, flags=3)["epilogue"] == "persist"
    assert [q(gf.TN, n, 64)["cfg"] for n in (64, 65, 384, 576, 768, 960, 1152)] == ["SMALL", "BIG", "BIG", "WIDE", "WIDE", "BIG", "BIG"]


WORST = {}


@pytest.mark.parametrize("name", [r["name"] for r in gf.ROWS])
def test_the_stand_in_is_exact_on_ints_and_inside_the_bound_on_mant(K, built, name):
    row, o = gf.BY_NAME[name], built(name)
    got = gf.emulate(row, o, gf.variants(K, row))
    if row["kind"] == "ints":
        want = o.want.astype(np.float32)
        if row["flags"] & gf.UPPER and got.ndim == 2:
            assert np.array_equal(np.triu(got), np.triu(want))
            low = np.tril(np.ones_like(got, bool), -1)
            assert ((got == want) | (got == o.C0))[low].all()
        else:
            assert np.array_equal(got, want)
    else:
        if row["flags"] & gf.UPPER and got.ndim == 2:
            got = np.triu(got) + np.triu(got, 1).T
        r = gf.ratio(got, o)
        fam = row["expect"][0].get("mode", "TNP")
        WORST[fam] = max(WORST.get(fam, 0.0), r)
        print(f"{name}: stand-in error / bound = {r:.4f}  (K = {o.K}: {r * (o.K + 10):.2f} units of 2^-24 M)")
        assert r <= 1.0


def test_print_the_worst_ratio_of_the_honest_stand_in():
    for fam, r in sorted(WORST.items()):
        print(f"\n{fam:6s} honest stand-in, worst error / bound {r:.4f}", end="")
    assert not WORST or max(WORST.values()) <= 1.0


def _differs(row, o, got):
    want = o.want.astype(np.float32)
    if row["flags"] & gf.UPPER and got.ndim == 2:
        return not np.array_equal(np.triu(got), np.triu(want))
    return not np.array_equal(got, want)


@pytest.mark.parametrize("name", ["tn-wide-768-upper", "tn-small-65rows", "tn-n191-K17", "tn-big-upper-13slabs", "conv-big-v1", "xcorr-2x40-c3", "tnp-small16"])
def test_mutant_dropping_the_last_ragged_chunk_breaks_ints(K, built, name):
    row, o = gf.BY_NAME[name], built(name)
    assert _differs(row, o, gf.emulate(row, o, gf.variants(K, row), mutant="drop_ragged_chunk"))


@pytest.mark.parametrize("name", ["tn-big-64slabs", "tn-wide-32slabs", "tn-n130-K16", "ntb-wide-768-L16", "conv-wide-v4", "tn-rpw64-1921"])
def test_mutant_mirroring_without_transposing_breaks_ints(K, built, name):
    row, o = gf.BY_NAME[name], built(name)
    assert _differs(row, o, gf.emulate(row, o, gf.variants(K, row), mutant="mirror_untransposed"))


@pytest.mark.parametrize("name", ["ntb-mant-small", "ntb-mant-big", "ntb-mant-wide"])
def test_mutant_ntb_without_the_l_h_term_exceeds_the_bound(K, built, name):
    row, o = gf.BY_NAME[name], built(name)
    r = gf.ratio(gf.emulate(row, o, gf.variants(K, row), mutant="ntb_drop_lh"), o)
    print(f"{name}: five-term product, error / bound = {r:.2f}")
    assert r > 1.0
