"""The table behind tests/test_gram16_fixtures.py (CPU) and tests/test_gpu_gram16_instances.py (GPU): one row per launch form of
the split-fp16 Gram engine (laplace_amd/csrc/lk_sweep16.hip) at an edge of its loops, each stating the form it claims, its
operands, its exact or fp64 reference, its bound, and a numpy stand-in for the launch.

Forms
  tn64   gram16_kernel<64, 64, 4, false>   lk_gram_tn_f16x2, C = 64: stages of 64 rows, four k-waves, + gram16_reduce4_kernel<64>
  tn128  gram16_kernel<128, 32, 1, false>  lk_gram_tn_f16x2, C % 128 == 0: stages of 32 rows, 2 x 2 waves, + gram16_reduce4_kernel<128>
  pp64   gram16_kernel<64, 64, 4, true>    lk_conv3x3_pixpair_accumulate_f16x2, Cin % 128 == 64 (tiles of 64 inside a Cin x Cin block)
  pp128  gram16_kernel<128, 32, 1, true>   lk_conv3x3_pixpair_accumulate_f16x2, Cin % 128 == 0
  pix13  pixpair13_kernel                  lk_conv3x3_pixpair_accumulate13_f16x2, Cin = 64: stages of 16 images, a ring of three
The claim of a ``tn*`` row (nbc, npairs, rows_per_split, nsplit) comes from ``plan_tn``, a replica of the launcher's plan; that of a
pixel-pair row (tile, n_tiles, n_blocks, stages) and its tile / slot tables from ``plan_pp`` / ``pixpair_tables``.  The CPU tier holds
every one of them against the library's own host functions.

Operand kinds (the result is  G0 + alpha 2^(-2 sexp) (H^T H' + H^T L' + L^T H'):  the product of the two l planes is never formed)
  ints   THE TEST builds the planes: h integer-valued in [-8, 8], l integer-valued in [-3, 3] and drawn INDEPENDENTLY of h (planes of
         a real split cannot tell the three terms apart, nor a swapped plane from a correct one), sexp in {-1, 0, 2}, alpha in
         {0.5, 1, 2}, G0 (or the initial blocks) integer-valued in [-64, 64].  Every product is an integer of at most 64 + 24 + 24 =
         112, so every partial sum in any order and the scaled result are exact in fp32 while 112 R 2^(2|sexp| + 1) < 2^24
         (``build`` asserts it; rows too long for that draw from the narrower ranges they name, with the same assertion on their own
         largest product) and the comparison is BIT EQUALITY with the fp64 value, which is exact as well.
  mant   entries uniform in [1, 2) with full 24-bit mantissas, split as lk_split_f16x2 splits them (one scale), G0 = 0, alpha = 1,
         R <= 128, against the fp64 Gram of the UNSPLIT fp32 values.  Element-wise, none exempt:
             |got - want| <= (3 R + 16) 2^-24 M_ij,   M the Gram of |x|
         because: the split keeps each factor to 2^-22 |x| (lk_split16.h), 4 units of 2^-24 each, 8 for the two factors of a product;
         the dropped l l' term is at most 2^-11 |x| 2^-11 |x'| = 2^-22 |x x'|, 4 more: 12 units; the running sum is rounded at
         most three times per row (three MFMAs per k16 step), each time by at most 2^-24 of a partial sum that M bounds: 3 R units;
         the remaining 4 cover the sums of the k-waves and of the partials (at most 1 + 3 roundings at R <= 128: one split) and the
         final scaling.
  scale  h = k 2^11 with integer k in [2, 8] (every Gram entry at least 4 R 2^22), l = 0, R = 1024, G0 = 0, alpha = 1 and a GIVEN
         sexp: the result is the integer Gram times 2^(-2 sexp), exact and normal in fp32 for every exponent used (``build`` asserts
         it), although 2^(-2 sexp) by itself is subnormal from sexp = 64 and zero from 75.  BIT EQUALITY.

The stand-in (``emulate``) walks the launch as the kernels do: splits of whole stages; stages of BKR rows, zero-filled past r1; the
k16 steps of a stage dealt to the four k-waves of the 64-tile, which are summed in wave order; three products per k16 step; the
32 x 32 tiles below the diagonal of a diagonal block never written (the workspace starts as NaN); the partials summed in
gram16_reduce4_kernel's order (wave g: p = g, g + 4, ...; then the four sums in order); the un-scaling alpha ((t 2^-sexp) 2^-sexp);
the read-modify-write of a pixel-pair block through the tile table; pixpair13_kernel's shift validity from the slot table.  Its
mutants are what the CPU tier must see fail."""
import functools
import zlib

import numpy as np

U = 2.0 ** -24
HALF = [(0, 0), (0, 1), (0, 2)] + [(dy, dx) for dy in (1, 2) for dx in range(-2, 3)]  # the 13 shifts, in slot order
SEXPS, ALPHAS = (-1, 0, 2), (0.5, 1.0, 2.0)
FORMS = ("tn64", "tn128", "pp64", "pp128", "pix13")
MUTANTS = ("drop_ah_bl", "swap_b_planes", "overread_last_stage", "pix13_no_skip", "unscale_factor_first")
CPU_MAX_ROWS = 40000  # rows longer than this are walked on the device only (tests/test_gram16_fixtures.py counts how many that is)

ROWS = []


# ---- the plans (replicas of the host code in lk_sweep16.hip / lk_gram.hip) -----------------------------------------------------
def plan_tn(R, C):
    """gram16_plan: two workgroups per CU, slices of whole stages, at least 8 stages per slice"""
    nb, bkr = (64, 64) if C == 64 else (128, 32)
    nbc = C // nb
    npairs = nbc * (nbc + 1) // 2
    want = -(-512 // npairs)
    stages = -(-R // bkr)
    per = max(-(-stages // want), 8)
    rps = per * bkr
    return dict(kernel="tn64" if C == 64 else "tn128", nb=nb, bkr=bkr, nbc=nbc, npairs=npairs, rows_per_split=rps,
                nsplit=max(-(-R // rps), 1))


def in_map(H, W, y, x, dy, dx):
    return 0 <= y + dy < H and 0 <= x + dx < W


def plan_pp(form, B, H, W, Cin):
    """lk_conv3x3_pixpair_plan and the stage count of the kernel the entry point picks"""
    n_blocks = sum(in_map(H, W, y, x, dy, dx) for y in range(H) for x in range(W) for dy, dx in HALF)
    tile = 128 if Cin % 128 == 0 else 64
    bkr = {"pp64": 64, "pp128": 32, "pix13": 16}[form]
    return dict(kernel=form, tile=tile, bkr=bkr, n_blocks=n_blocks, n_tiles=n_blocks * (Cin // tile) ** 2, stages=-(-B // bkr))


def pixpair_tables(H, W, Cin):
    """lk_conv3x3_pixpair_tables: tiles [n_tiles][3] = (column of the A panel, column of the B panel, output offset), slots [H W][13]"""
    T = 128 if Cin % 128 == 0 else 64
    tpp = Cin // T
    tiles, slots, slot = [], np.full((H * W, 13), -1, np.int32), 0
    for y in range(H):
        for x in range(W):
            for h, (dy, dx) in enumerate(HALF):
                if not in_map(H, W, y, x, dy, dx):
                    continue
                q, q2 = y * W + x, (y + dy) * W + x + dx
                slots[q, h] = slot
                for ta in range(tpp):
                    for tb in range(tpp):
                        tiles.append((q * Cin + ta * T, q2 * Cin + tb * T, slot * Cin * Cin + ta * T * Cin + tb * T))
                slot += 1
    return np.array(tiles, np.int32).reshape(-1, 3), slots


def reduce4_walk(nparts):
    """per wave of gram16_reduce4_kernel: (passes of the eight-deep loop, passes of the tail loop)"""
    out = []
    for g in range(4):
        p, deep, tail = g, 0, 0
        while p + 28 < nparts:
            p, deep = p + 32, deep + 1
        while p < nparts:
            p, tail = p + 4, tail + 1
        out.append((deep, tail))
    return tuple(out)


# ---- the table -----------------------------------------------------------------------------------------------------------------
def _row(name, **kw):
    assert all(r["name"] != name for r in ROWS), name
    ROWS.append(dict(name=name, **kw))


def tn(name, R, C, kind="ints", nsplit=None, **kw):
    claim = plan_tn(R, C)
    assert nsplit is None or claim["nsplit"] == nsplit, (name, claim)
    _row(name, entry="tn", form=claim["kernel"], kind=kind, R=R, C=C, launches=1, claim=claim, **kw)


def pp(name, form, B, H, W, Cin, kind="ints", launches=1, **kw):
    claim = plan_pp(form, B, H, W, Cin)
    assert (form == "pix13" and Cin == 64) or (form == "pp64" and Cin % 128 == 64) or (form == "pp128" and Cin % 128 == 0), name
    _row(name, entry="pp", form=form, kind=kind, B=B, H=H, W=W, Cin=Cin, R=B, launches=launches, claim=claim, **kw)


# tn64: R below one stage, at the k16 hand-over between the k-waves, at the stage and the split boundary
for _R in (1, 15, 16, 17, 63, 64, 65, 511, 512, 513):
    tn(f"tn64-R{_R}", _R, 64, nsplit=2 if _R == 513 else 1)
# ... the partial counts at the edges of reduce4's loops, the last split holding ONE row (rows_per_split = 512)
NSPLIT_EDGES = (3, 4, 5, 28, 29, 32, 33, 36, 64, 65)
for _n in NSPLIT_EDGES:
    tn(f"tn64-{_n}splits-last1", (_n - 1) * 512 + 1, 64, nsplit=_n)
for _n in (4, 32, 64):  # ... and holding a whole split
    tn(f"tn64-{_n}splits-whole", _n * 512, 64, nsplit=_n)
# 512 splits; more than 8 stages per split (4097 stages: 9 per split, 456 splits, the last with 128 rows) -- narrower integers
tn("tn64-512splits", 262144, 64, nsplit=512, hmax=2, lmax=1, sexp=0)
tn("tn64-9stages-per-split", 262208, 64, nsplit=456, hmax=2, lmax=1, sexp=0)
assert ROWS[-1]["claim"]["rows_per_split"] == 9 * 64
# tn128
for _R in (1, 31, 32, 33, 255, 256, 257):
    tn(f"tn128-R{_R}", _R, 128, nsplit=2 if _R == 257 else 1)
for _n in (4, 29, 33):
    tn(f"tn128-{_n}splits-last1", (_n - 1) * 256 + 1, 128, nsplit=_n)
tn("tn128-c256-3pairs", 296, 256, nsplit=2)    # the last split: 40 rows = a whole stage and 8 rows
tn("tn128-c384-6pairs", 300, 384, nsplit=2)    # 44 rows: 32 + 12
tn("tn128-c640-15pairs", 530, 640, nsplit=3)   # 18 rows: one ragged stage
tn("tn128-c1024-R40", 40, 1024, nsplit=1)      # 36 pairs, two stages, the second of 8 rows
# pp64: Cin in {64, 192, 320} (192, 320: 3 x 3 and 5 x 5 tiles of 64 inside a block, ldc = Cin), B at the edges of the 64-row stage
pp("pp64-c64-1x1-B1", "pp64", 1, 1, 1, 64)
pp("pp64-c64-1x3-B63", "pp64", 63, 1, 3, 64)
pp("pp64-c64-3x1-B64", "pp64", 64, 3, 1, 64)
pp("pp64-c64-5x7-B65", "pp64", 65, 5, 7, 64)
pp("pp64-c64-3x3-B129", "pp64", 129, 3, 3, 64)
pp("pp64-c192-1x3-B63", "pp64", 63, 1, 3, 192)    # 54 tiles
pp("pp64-c192-3x3-B64", "pp64", 64, 3, 3, 192)
pp("pp64-c192-2x2-B129", "pp64", 129, 2, 2, 192)  # 90 tiles
pp("pp64-c320-3x1-B65", "pp64", 65, 3, 1, 320)    # 150 tiles
pp("pp64-c320-2x2-B1", "pp64", 1, 2, 2, 320)      # 250 tiles
pp("pp64-c192-stacked", "pp64", 65, 3, 3, 192, launches=2)
# pp128: Cin in {128, 256, 384}, B at the edges of the 32-row stage
pp("pp128-c128-1x1-B1", "pp128", 1, 1, 1, 128)
pp("pp128-c128-3x1-B32", "pp128", 32, 3, 1, 128)
pp("pp128-c128-5x7-B33", "pp128", 33, 5, 7, 128)
pp("pp128-c128-3x3-B65", "pp128", 65, 3, 3, 128)
pp("pp128-c256-1x3-B31", "pp128", 31, 1, 3, 256)
pp("pp128-c256-2x2-B32", "pp128", 32, 2, 2, 256)
pp("pp128-c256-3x3-B33", "pp128", 33, 3, 3, 256)
pp("pp128-c384-3x1-B65", "pp128", 65, 3, 1, 384)  # 54 tiles
pp("pp128-c384-2x2-B1", "pp128", 1, 2, 2, 384)    # 90 tiles
pp("pp128-c256-stacked", "pp128", 33, 2, 2, 256, launches=2)
# pix13: 1, 2, 3, 4 stages of 16 images (the ring of three holds two in flight) and more; 5 x 5 has a pixel with all 13 shifts
pp("pix13-1x1-B1", "pix13", 1, 1, 1, 64)
pp("pix13-1x3-B15", "pix13", 15, 1, 3, 64)
pp("pix13-3x1-B16", "pix13", 16, 3, 1, 64)
pp("pix13-3x3-B17", "pix13", 17, 3, 3, 64)
pp("pix13-2x5-B32", "pix13", 32, 2, 5, 64)
pp("pix13-5x5-B33", "pix13", 33, 5, 5, 64)
pp("pix13-5x7-B48", "pix13", 48, 5, 7, 64)
pp("pix13-3x3-B49", "pix13", 49, 3, 3, 64)
pp("pix13-2x5-B64", "pix13", 64, 2, 5, 64)
pp("pix13-5x5-B100", "pix13", 100, 5, 5, 64)
pp("pix13-3x3-stacked", "pix13", 33, 3, 3, 64, launches=2)
# mant: one row per form
tn("tn64-mant", 128, 64, kind="mant")
tn("tn128-mant", 100, 256, kind="mant")
pp("pp64-mant", "pp64", 100, 2, 2, 192, kind="mant")
pp("pp128-mant", "pp128", 128, 2, 2, 128, kind="mant")
pp("pix13-mant", "pix13", 100, 3, 3, 64, kind="mant")
# scale: a tensor that is small (or large) as a whole
SCALE_SEXPS = (-40, 40, 63, 64, 74, 75, 78)
for _s in SCALE_SEXPS:
    tn(f"tn64-scale{_s}", 1024, 64, kind="scale", sexp=_s)
tn("tn128-scale75", 1024, 128, kind="scale", sexp=75)
pp("pp64-scale63", "pp64", 1024, 1, 3, 64, kind="scale", sexp=63)
pp("pp64-scale75", "pp64", 1024, 2, 2, 192, kind="scale", sexp=75)
pp("pp128-scale75", "pp128", 1024, 1, 3, 128, kind="scale", sexp=75)
pp("pix13-scale75", "pix13", 1024, 2, 2, 64, kind="scale", sexp=75)

BY_NAME = {r["name"]: r for r in ROWS}


# ---- operands and references ----------------------------------------------------------------------------------------------------
class Built:
    pass


def split_f16x2(x):
    """lk_split_f16x2 on the host: (h, l, sexp) with max|x| 2^sexp in [2^14, 2^15), h = fp16(xs), l = fp16(xs - h)"""
    amax = float(np.abs(x).max())
    sexp = min(14 - int(np.floor(np.log2(amax))), 120)
    xs = x.astype(np.float32) * np.float32(2.0 ** sexp)
    h = xs.astype(np.float16)
    l = (xs - h.astype(np.float32)).astype(np.float16)
    return h, l, sexp


def operand_shape(row):
    return (row["launches"], row["R"], row["C"]) if row["entry"] == "tn" else (row["launches"], row["B"], row["H"] * row["W"] * row["Cin"])


def product64(H, L, H2, L2):
    """what the three MFMAs of a step add up to, in fp64: H^T H' + H^T L' + L^T H'"""
    f = np.float64
    H, L, H2, L2 = H.astype(f), L.astype(f), H2.astype(f), L2.astype(f)
    return H.T @ (H2 + L2) + L.T @ H2


def reference(row, planes_of):
    """sum over the launches of ``scale(launch) * product`` -- [C][C] for ``tn``, [n_blocks][Cin][Cin] in slot order for pixel pairs;
    ``planes_of(launch)`` -> (H, L, scale), H and L as [rows][columns]"""
    out = None
    for la in range(row["launches"]):
        H, L, sc = planes_of(la)
        if row["entry"] == "tn":
            G = product64(H, L, H, L)
        else:
            Hh, Ww, C = row["H"], row["W"], row["Cin"]
            px = lambda P, q: P[:, q * C:(q + 1) * C]  # noqa: E731
            G = np.stack([product64(px(H, y * Ww + x), px(L, y * Ww + x), px(H, (y + dy) * Ww + x + dx), px(L, (y + dy) * Ww + x + dx))
                          for y in range(Hh) for x in range(Ww) for dy, dx in HALF if in_map(Hh, Ww, y, x, dy, dx)])
        out = sc * G if out is None else out + sc * G
    return out


@functools.lru_cache(maxsize=None)
def build(name):
    """``build_row`` of a row of the table, cached: the tests share one copy and leave it unchanged"""
    return build_row(BY_NAME[name])


def adhoc(name, **kw):
    """a row outside the table (the route-against-route comparisons): ``ints`` with l = 0, where the dropped term is zero"""
    row = dict(name=name, kind="ints", launches=1, lzero=True, sexp=0)
    row.update(kw)
    if row["entry"] == "tn":
        row.update(claim=plan_tn(row["R"], row["C"]))
        row.update(form=row["claim"]["kernel"])
    else:
        row.update(R=row["B"], claim=plan_pp(row["form"], row["B"], row["H"], row["W"], row["Cin"]))
    return row


def build_row(row):
    """operands (fp16 planes ``h``, ``l`` [launch][rows][columns], ``sexp`` per launch), alpha, G0, the fp64 reference ``want`` and,
    for ``mant``, the element-wise bound ``tol``"""
    name = row["name"]
    seed = zlib.crc32(name.encode())
    rng = np.random.default_rng(seed)
    o = Built()
    kind, shape, R = row["kind"], operand_shape(row), row["R"]
    f = np.float64
    if kind == "ints":
        hmax, lmax = row.get("hmax", 8), row.get("lmax", 3)
        o.h = rng.integers(-hmax, hmax + 1, size=shape).astype(np.float16)
        o.l = rng.integers(-lmax, lmax + 1, size=shape).astype(np.float16) * np.float16(0 if row.get("lzero") else 1)
        o.alpha = ALPHAS[seed % 3]
        P = hmax * hmax + 2 * hmax * lmax  # the largest |h h' + h l' + l h'|: 112 for the ranges of the docstring
        o.sexp = []
        for la in range(row["launches"]):  # the first exponent of the rotation that keeps the row exact (a given one has to)
            cands = [row["sexp"]] if "sexp" in row else [SEXPS[(seed // 3 + la + i) % 3] for i in range(3)]
            o.sexp.append(next(s for s in cands if P * R * 2 ** (2 * abs(s) + 1) < 1 << 24))
        # the sum of all launches on top of G0: from the finest bit any launch adds to the largest value, inside 24 bits
        lo = min([1.0] + [2.0 ** (-2 * s - 1) for s in o.sexp])
        hi = 64 + sum(P * R * 2.0 ** (-2 * s + 1) for s in o.sexp)
        assert P * R < 1 << 24 and hi / lo < 1 << 24, name
    elif kind == "mant":
        assert R <= 128 and row["launches"] == 1, name
        m = rng.integers(0, 1 << 23, size=shape, dtype=np.int64)  # 1.m with all 23 mantissa bits drawn
        o.x = (1.0 + m.astype(f) * 2.0 ** -23).astype(np.float32)
        o.h, o.l, s = split_f16x2(o.x)
        o.alpha, o.sexp = 1.0, [s]
    else:
        assert R == 1024 and row["launches"] == 1, name
        o.h = (rng.integers(2, 9, size=shape) * 2048).astype(np.float16)
        o.l = np.zeros(shape, np.float16)
        o.alpha, o.sexp = 1.0, [row["sexp"]]
    G = reference(row, lambda la: (o.h[la], o.l[la], 2.0 ** (-2 * o.sexp[la])))
    if kind == "ints":
        g0 = rng.integers(-64, 65, size=G.shape).astype(np.float32)
        o.G0 = g0 if G.ndim == 3 else np.triu(g0) + np.triu(g0, 1).T
    else:
        o.G0 = np.zeros(G.shape, np.float32)
    o.want = o.G0.astype(f) + o.alpha * G
    o.tol = None
    if kind == "mant":
        x64 = o.x.astype(f)
        o.want = reference(row, lambda la: (x64[la], np.zeros_like(x64[la]), 1.0))  # the Gram of the UNSPLIT values
        o.tol = (3 * R + 16) * U * o.want  # (M = the Gram of |x| = the Gram itself: every entry is positive)
    else:
        w32 = o.want.astype(np.float32)
        assert np.array_equal(w32.astype(f), o.want), name  # exact in fp32 ...
        if kind == "scale":
            assert (np.abs(w32) >= 2.0 ** -126).all() and np.isfinite(w32).all() and G.min() * 2.0 ** (2 * o.sexp[0]) >= 4 * R * 2 ** 22, name
    return o


def ratio(row, got, o):
    """worst |got - want| / bound over every element the launch computes (``mant`` rows): all of the blocks, every element of the
    upper 32 x 32 tiles of G -- the tiles below them have to stay G0 to the bit"""
    r = np.abs(np.asarray(got, np.float64) - o.want) / o.tol
    if row["entry"] == "tn":
        up = upper_tiles(row["C"])
        assert np.array_equal(np.asarray(got)[~up].view(np.int32), o.G0[~up].view(np.int32)), row["name"]
        r = r[up]
    return float(r.max())


def upper_tiles(n):
    """[n][n] bool: the elements of the 32 x 32 tiles (ti <= tj) -- what lk_gram_tn_f16x2 writes; everything else stays G0"""
    t = np.arange(n) // 32
    return t[:, None] <= t[None, :]


# ---- the stand-in ---------------------------------------------------------------------------------------------------------------
def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _mfma3(acc, ah, al, bh, bl, exact, mutant):
    """one k16 step of a tile: acc += al^T bh, += ah^T bl, += ah^T bh, the accumulator rounded to fp32 after each"""
    terms = [(al, bh), (ah, bl), (ah, bh)]
    if mutant == "drop_ah_bl":
        terms = [terms[0], terms[2]]
    elif mutant == "swap_b_planes":
        terms = [(al, bl), (ah, bh), (ah, bl)]
    for a, b in terms:
        if exact:
            acc = acc + a.T @ b  # (fp32 matmul of integers below 2^24: exact in any order)
        else:
            acc = (acc.astype(np.float64) + a.astype(np.float64).T @ b.astype(np.float64)).astype(np.float32)
    return acc


def _pad(plane, rows):
    """the plane as the device holds it: a band of NaN behind its last row (what a read past r1 would find)"""
    return np.concatenate([_f32(plane), np.full((rows, plane.shape[1]), np.nan, np.float32)])


def _tile_product(Hp, Lp, colA, colB, NB, BKR, r0, r1, exact, mutant):
    """gram16_kernel's K loop for one workgroup: rows r0 .. r1 of the column panels at colA / colB -> the [NB][NB] sum"""
    KW = 4 if NB == 64 else 1
    acc = [np.zeros((NB, NB), np.float32) for _ in range(KW)]
    nstage = -(-(r1 - r0) // BKR) if r1 > r0 else 0
    for s in range(nstage):
        rb = r0 + s * BKR
        stage = []
        for P, c in ((Hp, colA), (Lp, colA), (Hp, colB), (Lp, colB)):
            img = P[rb:rb + BKR, c:c + NB].copy()
            if mutant != "overread_last_stage":
                img[max(r1 - rb, 0):] = 0.0  # rows past r1 come from zero16
            stage.append(img)
        for k16 in range(BKR // 16):
            w = k16 if KW == 4 else 0  # the 64-tile deals its four k16 steps to its four waves
            ah, al, bh, bl = (p[k16 * 16:(k16 + 1) * 16] for p in stage)
            acc[w] = _mfma3(acc[w], ah, al, bh, bl, exact, mutant)
    return ((acc[0] + acc[1]) + acc[2]) + acc[3] if KW == 4 else acc[0]


def _unscale(old, t, alpha, sexp, mutant):
    """old + alpha ((t 2^-sexp) 2^-sexp), the products in fp32, the last multiply-add fused"""
    inv = np.float32(2.0 ** min(max(-sexp, -126), 127))
    with np.errstate(under="ignore", over="ignore"):
        if mutant == "unscale_factor_first":
            f = np.float32(np.float32(np.float32(alpha) * inv) * inv)  # (2^(-2 sexp) first: subnormal from 64, zero from 75)
            return (old.astype(np.float64) + np.float64(f) * t.astype(np.float64)).astype(np.float32)
        tt = (t * inv) * inv
    return (old.astype(np.float64) + np.float64(alpha) * tt.astype(np.float64)).astype(np.float32)


def _emulate_tn(row, o, mutant):
    c, R, C = row["claim"], row["R"], row["C"]
    NB, BKR, nbc, rps, nsplit = c["nb"], c["bkr"], c["nbc"], c["rows_per_split"], c["nsplit"]
    exact = row["kind"] != "mant"
    Hp, Lp = _pad(o.h[0], BKR), _pad(o.l[0], BKR)
    pairs = [(bi, bj) for bi in range(nbc) for bj in range(bi, nbc)]
    ws = np.full((nsplit, len(pairs), NB, NB), np.nan, np.float32)  # exactly the advertised workspace, NaN as the GPU tier fills it
    diag_live = upper_tiles(NB)
    for s in range(nsplit):
        r0, r1 = s * rps, min(R, (s + 1) * rps)
        for pi, (bi, bj) in enumerate(pairs):
            v = _tile_product(Hp, Lp, bi * NB, bj * NB, NB, BKR, r0, r1, exact, mutant)
            live = diag_live if bi == bj else np.ones((NB, NB), bool)
            ws[s, pi][live] = v[live]
    G = o.G0.copy()
    for pi, (bi, bj) in enumerate(pairs):  # gram16_reduce4_kernel
        live = diag_live if bi == bj else np.ones((NB, NB), bool)
        sums = []
        for g in range(4):
            acc = np.zeros((NB, NB), np.float32)
            for p in range(g, nsplit, 4):
                acc = acc + np.where(live, ws[p, pi], 0.0).astype(np.float32)
            sums.append(acc)
        t = ((sums[0] + sums[1]) + sums[2]) + sums[3]
        blk = G[bi * NB:(bi + 1) * NB, bj * NB:(bj + 1) * NB]
        blk[live] = _unscale(blk, t, o.alpha, o.sexp[0], mutant)[live]
    return G


def _emulate_pp(row, o, mutant):
    c, B, Hh, Ww, C = row["claim"], row["B"], row["H"], row["W"], row["Cin"]
    exact = row["kind"] != "mant"
    tiles, slots = pixpair_tables(Hh, Ww, C)
    nb = c["n_blocks"]
    # the blocks behind a guard block of -0.0 (slot -1): a write there poisons the result, as the GPU tier's band check fails
    buf = np.concatenate([np.full(C * C, -0.0, np.float32), o.G0.reshape(-1)])
    blocks = buf[C * C:]
    for la in range(row["launches"]):
        Hp, Lp = _pad(o.h[la], c["bkr"]), _pad(o.l[la], c["bkr"])
        if row["form"] == "pix13":
            zero = np.zeros((B + 16, 64), np.float32)
            for q in range(Hh * Ww):
                for h, (dy, dx) in enumerate(HALF):
                    slot = int(slots[q, h])
                    if slot < 0 and mutant != "pix13_no_skip":
                        continue
                    acc = np.zeros((64, 64), np.float32)
                    for s in range(c["stages"]):
                        rows = slice(s * 16, s * 16 + 16)
                        cut = lambda img: img if mutant == "overread_last_stage" else np.where(np.arange(s * 16, s * 16 + 16)[:, None] < B, img, 0.0).astype(np.float32)  # noqa: E731
                        ah, al = cut(Hp[rows, q * 64:q * 64 + 64]), cut(Lp[rows, q * 64:q * 64 + 64])
                        if slot >= 0:
                            q2 = q + dy * Ww + dx
                            bh, bl = cut(Hp[rows, q2 * 64:q2 * 64 + 64]), cut(Lp[rows, q2 * 64:q2 * 64 + 64])
                        else:
                            bh = bl = zero[rows]  # (a panel outside the map stages zeros)
                        acc = _mfma3(acc, ah, al, bh, bl, exact, mutant)
                    dst = buf[(slot + 1) * 4096:(slot + 2) * 4096].reshape(64, 64)
                    dst[...] = _unscale(dst, acc, o.alpha, o.sexp[la], mutant)
        else:
            T = c["tile"]
            for colA, colB, off in tiles:
                v = _tile_product(Hp, Lp, int(colA), int(colB), T, c["bkr"], 0, B, exact, mutant)
                idx = int(off) + np.arange(T)[:, None] * C + np.arange(T)[None, :]  # blocks[off + r * ldc + c], ldc = Cin
                blocks[idx] = _unscale(blocks[idx], v, o.alpha, o.sexp[la], mutant)
    guard = buf[:C * C]
    if not (np.signbit(guard) & (guard == 0)).all():
        return np.full((nb, C, C), np.nan, np.float32)
    return blocks.reshape(nb, C, C).copy()


def emulate(row, o, mutant=None):
    """the row as the kernels compute it, in numpy: G [C][C] or the blocks [n_blocks][Cin][Cin] after the launch(es)"""
    assert mutant is None or mutant in MUTANTS
    return _emulate_tn(row, o, mutant) if row["entry"] == "tn" else _emulate_pp(row, o, mutant)
