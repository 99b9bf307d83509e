"""The table behind tests/test_gram_fixtures.py (CPU) and tests/test_gpu_gram_instances.py (GPU): one row per launch form of the
fp32 Gram engine (laplace_amd/csrc/lk_gram.hip), each stating the variant it claims (``lk_gram_launch_variant`` must agree), with
its operands, its fp64 reference, its bound and a numpy stand-in for the kernel's arithmetic.

Operand kinds
  ints  entries are integers in [-8, 8], C0 integer-valued in [-64, 64] and symmetric, alpha in {0.5, 1, 2}.  Every product, every
        partial sum in any order, every bf16 piece (m = l = 0) and every strip correction is exact in fp32 while 64 K + 64 < 2^24
        (``build`` asserts it), so the expected result is the integer Gram (formed in fp64, where it is exact as well) and the
        comparison is BIT EQUALITY.
  mant  entries uniform in [1, 2) with full 24-bit mantissas, C0 = 0, alpha = 1, K <= 128.  Element-wise, for any summation order:
        |got - want64| <= (K + 10) 2^-24 M_ij, M the Gram of |x| (K roundings of the running sum; the 10 covers the three dropped
        split-bf16 terms, <= 8 * 2^-24 per product (tests/test_split_bf16.py), and the final scaling).  For the shift-correlation
        form K = B H W and M = R + Row + Col + Pix, the four terms taken absolutely.

The stand-in (``emulate``) walks the launch as the kernel does — tiles of T, chunks of BK rows, splits of K, slabs summed in fp32
in the order of gram_reduce_kernel (two-level beyond 32), mirror or upper-only, direct epilogue, persistent slabs, the NT rows
padded to whole chunks, the six-term split-bf16 product — with three mutants the CPU tests must see fail.  For ``ints`` a chunk is
summed by one fp32 matmul (any order is exact); for ``mant`` row by row with one rounding per row."""
import numpy as np

UPPER, PERSIST = 1, 2
U = 2.0 ** -24
TN, NT, CONV, XCORR_FULL, XCORR_STRIPS = range(5)  # ``entry`` of lk_gram_launch_variant

HALF = [(0, 0), (0, 1), (0, 2)] + [(dy, dx) for dy in (1, 2) for dx in range(-2, 3)]  # the 13 shifts of the full-grid launch
ALL25 = [(t // 5 - 2, t % 5 - 2) for t in range(25)]
HALF_INDEX = [-1] * 12 + list(range(13))  # (Dy + 2) * 5 + Dx + 2 -> index into HALF, -1: the transpose of -D

ROWS = []


def _row(name, entry, kind, expect, **kw):
    assert all(r["name"] != name for r in ROWS), name
    ROWS.append(dict(name=name, entry=entry, kind=kind, expect=expect, **kw))


def E(mode, vec, cfg, epilogue="slabs", **more):
    return dict(mode=mode, vec=vec, cfg=cfg, epilogue=epilogue, **more)


def tn(name, n, K, expect, kind="ints", ldx=None, off=0, flags=0, launches=1):
    _row(name, "tn", kind, [expect], n=n, K=K, ldx=n if ldx is None else ldx, off=off, flags=flags, launches=launches)


def nt(name, n, L, nb, nseg, expect, kind="ints", mis=None, flags=0, launches=1):
    _row(name, "nt", kind, [expect], n=n, L=L, nb=nb, nseg=nseg, mis=mis, flags=flags, launches=launches)


def conv(name, B, Cin, H, W, k, s, p, d, expect, kind="ints", off=0, flags=0):
    two = lambda v: tuple(v) if isinstance(v, tuple) else (v, v)  # noqa: E731
    _row(name, "conv", kind, [expect], B=B, Cin=Cin, H=H, W=W, k=two(k), s=two(s), p=two(p), d=two(d), off=off, flags=flags,
         n=Cin * two(k)[0] * two(k)[1])


def xcorr(name, B, Cin, H, W, full, strips, kind="ints", off=0):
    _row(name, "xcorr", kind, [full, strips], B=B, Cin=Cin, H=H, W=W, off=off, flags=0, n=9 * Cin)


def tnp(name, B, Cin, H, W, tile, kind="ints"):
    _row(name, "tnp", kind, [dict(tile=tile)], B=B, Cin=Cin, H=H, W=W, flags=UPPER)


# ---- TN ------------------------------------------------------------------------------------------------------------------------
# reductions: 33 slabs (SMALL and BIG), 64 slabs, 32 slabs (the last one-level count), rpw = 64 on the square form
tn("tn-small-33slabs", 64, 8448, E("TN", 4, "SMALL", nsplit=33, two_level=True, rpw=4))
tn("tn-big-33slabs", 128, 2112, E("TN", 4, "BIG", nsplit=33, two_level=True, rpw=4))
tn("tn-big-64slabs", 200, 4096, E("TN", 4, "BIG", nsplit=64, two_level=True, rpw=4))
tn("tn-wide-32slabs", 576, 2048, E("TN", 4, "WIDE", nsplit=32, two_level=False, rpw=4))
tn("tn-rpw64-1921", 1921, 16, E("TN", 1, "BIG", nsplit=1, rpw=64))
tn("tn-rpw64-1924", 1924, 16, E("TN", 4, "BIG", nsplit=1, rpw=64))
# WIDE: both sizes, VEC 1 from ldx % 4 != 0 and from an operand one float past a 16-byte boundary, no mirror with several splits
# (K = 130: nine chunks in two splits of five and four, the last chunk two rows), direct
tn("tn-wide-ldx577", 576, 130, E("TN", 1, "WIDE", nsplit=2), ldx=577)
tn("tn-wide-768-upper", 768, 130, E("TN", 4, "WIDE", nsplit=2, chunks_per_split=5, nchunks=9), flags=UPPER)
tn("tn-wide-768-off1-direct", 768, 17, E("TN", 1, "WIDE", "direct"), off=1, flags=UPPER)
tn("tn-wide-direct", 576, 100, E("TN", 4, "WIDE", "direct"), flags=UPPER)
tn("tn-big-direct", 200, 100, E("TN", 4, "BIG", "direct"), flags=UPPER)
tn("tn-small-direct", 64, 100, E("TN", 4, "SMALL", "direct"), flags=UPPER)
tn("tn-big-upper-13slabs", 130, 1000, E("TN", 1, "BIG", nsplit=13), flags=UPPER)
# ldx > n, operand offset
tn("tn-ldx72", 68, 40, E("TN", 4, "BIG"), ldx=72)
tn("tn-ldx71", 68, 40, E("TN", 1, "BIG"), ldx=71)
tn("tn-small-off1", 64, 130, E("TN", 1, "SMALL"), off=1)
tn("tn-small-65rows", 63, 65, E("TN", 1, "SMALL", nchunks=2))
# edges of n, each with an edge of K for its chunk depth (0, 1, BK - 1, BK, BK + 1), mirrored and upper-only in turn
N_EDGES = [1, 3, 63, 64, 65, 127, 128, 129, 130, 191, 193]
for _i, _n in enumerate(N_EDGES):
    _bk = 64 if _n <= 64 else 16
    _K = [0, 1, _bk - 1, _bk, _bk + 1][_i % 5]
    _up = _i % 2 == 1
    tn(f"tn-n{_n}-K{_K}", _n, _K, E("TN", 4 if _n % 4 == 0 else 1, "SMALL" if _n <= 64 else "BIG", "direct" if _up else "slabs", BK=_bk),
       flags=UPPER if _up else 0)
# persistent slabs over two launches, then lk_gram_slabs_reduce_f32
tn("tn-persist", 200, 300, E("TN", 4, "BIG", "persist", nsplit=4), flags=PERSIST, launches=2)
# mant
tn("tn-mant-small-v4", 64, 128, E("TN", 4, "SMALL"), kind="mant")
tn("tn-mant-small-v1", 63, 100, E("TN", 1, "SMALL"), kind="mant")
tn("tn-mant-big-v4", 132, 100, E("TN", 4, "BIG"), kind="mant")
tn("tn-mant-big-v1", 130, 100, E("TN", 1, "BIG", "direct"), kind="mant", flags=UPPER)
tn("tn-mant-wide-v4", 576, 128, E("TN", 4, "WIDE"), kind="mant")
tn("tn-mant-wide-v1", 576, 100, E("TN", 1, "WIDE"), kind="mant", ldx=577)

# ---- NT / NTB ------------------------------------------------------------------------------------------------------------------
nt("nt-small-L15", 64, 15, 2, 1, E("NT", 1, "SMALL"))
nt("nt-big-L17-2seg", 100, 17, 2, 2, E("NT", 1, "BIG"))
nt("nt-big-L1", 65, 1, 5, 1, E("NT", 1, "BIG"))
nt("nt-wide-L15-direct", 576, 15, 3, 1, E("NT", 1, "WIDE", "direct"), flags=UPPER)
nt("nt-small-misaligned-seg", 64, 16, 2, 2, E("NT", 1, "SMALL"), mis=1)
nt("ntb-small-L100-16seg", 64, 100, 2, 16, E("NTB", 4, "SMALL", nsplit=16))
nt("ntb-big-L16-2seg", 130, 16, 3, 2, E("NTB", 4, "BIG"))
nt("ntb-big-L100-upper", 193, 100, 2, 2, E("NTB", 4, "BIG", nsplit=7), flags=UPPER)
nt("ntb-wide-768-L16", 768, 16, 3, 1, E("NTB", 4, "WIDE"))
nt("ntb-wide-576-L100-upper", 576, 100, 4, 1, E("NTB", 4, "WIDE", nsplit=7), flags=UPPER)
nt("ntb-small-direct", 33, 16, 2, 1, E("NTB", 4, "SMALL", "direct"), flags=UPPER)
nt("ntb-big-nb0", 100, 16, 0, 1, E("NTB", 4, "BIG", nchunks=1))
nt("nt-persist", 64, 100, 2, 2, E("NTB", 4, "SMALL", "persist"), flags=PERSIST, launches=2)
nt("nt-mant-small", 64, 15, 4, 1, E("NT", 1, "SMALL"), kind="mant")
nt("nt-mant-big", 130, 17, 2, 2, E("NT", 1, "BIG"), kind="mant")
nt("nt-mant-wide", 576, 15, 4, 1, E("NT", 1, "WIDE"), kind="mant")
nt("ntb-mant-small", 64, 16, 1, 1, E("NTB", 4, "SMALL"), kind="mant")
nt("ntb-mant-big", 132, 16, 2, 1, E("NTB", 4, "BIG"), kind="mant")
nt("ntb-mant-wide", 768, 16, 2, 2, E("NTB", 4, "WIDE"), kind="mant")
nt("ntb-mant-L100", 65, 100, 1, 1, E("NTB", 4, "BIG", "direct"), kind="mant", flags=UPPER)

# ---- CONV (implicit im2col) ----------------------------------------------------------------------------------------------------
conv("conv-small-v4", 2, 4, 5, 5, 3, 1, 1, 1, E("CONV", 4, "SMALL"))
conv("conv-small-v1", 4, 3, 5, 5, 2, 2, 0, 1, E("CONV", 1, "SMALL"))
conv("conv-small-off1", 2, 4, 5, 5, 3, 2, 1, 1, E("CONV", 1, "SMALL"), off=1)
conv("conv-anisotropic", 2, 8, 9, 7, (3, 2), (2, 1), (1, 0), (1, 2), E("CONV", 4, "SMALL"))  # (the anisotropic case of CONV_CASES)
conv("conv-big-1x1-s2", 4, 128, 8, 8, 1, 2, 0, 1, E("CONV", 4, "BIG"))
conv("conv-big-v1", 2, 6, 14, 14, 5, 1, 0, 1, E("CONV", 1, "BIG"))
conv("conv-wide-v4", 4, 64, 8, 8, 3, 1, 1, 1, E("CONV", 4, "WIDE", nsplit=4))
conv("conv-wide-v1-direct", 3, 9, 9, 9, 8, 1, 0, 1, E("CONV", 1, "WIDE", "direct"), flags=UPPER)
conv("conv-kernel-larger-than-input", 3, 5, 2, 2, 3, 1, 1, 1, E("CONV", 1, "SMALL"))
conv("conv-one-output-pixel", 5, 8, 3, 3, 3, 1, 0, 1, E("CONV", 4, "BIG", "direct"), flags=UPPER)
conv("conv-mant-small-v4", 2, 4, 5, 5, 3, 1, 1, 1, E("CONV", 4, "SMALL"), kind="mant")
conv("conv-mant-small-v1", 4, 3, 5, 5, 2, 2, 0, 1, E("CONV", 1, "SMALL"), kind="mant")
conv("conv-mant-big-v4", 2, 8, 6, 6, 3, 1, 1, 1, E("CONV", 4, "BIG"), kind="mant")
conv("conv-mant-big-v1", 2, 6, 10, 10, 5, 1, 0, 1, E("CONV", 1, "BIG"), kind="mant")
conv("conv-mant-wide-v4", 2, 64, 8, 8, 3, 1, 1, 1, E("CONV", 4, "WIDE"), kind="mant")
conv("conv-mant-wide-v1", 3, 9, 9, 9, 8, 1, 0, 1, E("CONV", 1, "WIDE"), kind="mant")

# ---- shift-correlation: (full-grid launch, strips launch) -----------------------------------------------------------------------
xcorr("xcorr-2x2-c384-rpw64", 1, 384, 2, 2, E("XCORR", 4, "BIG", rpw=4), E("XCORR", 4, "BIG", rpw=64))
xcorr("xcorr-2x40-c3", 3, 3, 2, 40, E("XCORR", 1, "SMALL"), E("XCORR", 1, "SMALL"))
xcorr("xcorr-17x3-c12", 2, 12, 17, 3, E("XCORR", 4, "SMALL"), E("XCORR", 4, "SMALL"))
# the strips launch: Kmax = 128 rows are 8 chunks in 2 splits; the corner regions have one chunk, so their second split is empty
xcorr("xcorr-2x64-c68-empty-split", 2, 68, 2, 64, E("XCORR", 4, "BIG", nsplit=4), E("XCORR", 4, "BIG", nsplit=2, nchunks=8))
xcorr("xcorr-4x4-c65", 2, 65, 4, 4, E("XCORR", 1, "BIG"), E("XCORR", 1, "BIG"))
xcorr("xcorr-4x4-c8-off1", 2, 8, 4, 4, E("XCORR", 1, "SMALL"), E("XCORR", 1, "SMALL"), off=1)
xcorr("xcorr-mant-small-v1", 1, 3, 2, 40, E("XCORR", 1, "SMALL"), E("XCORR", 1, "SMALL"), kind="mant")
xcorr("xcorr-mant-small-v4", 2, 8, 4, 4, E("XCORR", 4, "SMALL"), E("XCORR", 4, "SMALL"), kind="mant")
xcorr("xcorr-mant-big-v1", 2, 65, 2, 2, E("XCORR", 1, "BIG"), E("XCORR", 1, "BIG"), kind="mant")
xcorr("xcorr-mant-big-v4", 2, 68, 4, 4, E("XCORR", 4, "BIG"), E("XCORR", 4, "BIG"), kind="mant")

# ---- pixel-pair blocks (MODE_TNP through lk_conv3x3_pixpair_accumulate_f32; the tile comes from lk_conv3x3_pixpair_plan) --------
tnp("tnp-small16", 20, 64, 3, 3, 64)
tnp("tnp-big", 17, 128, 2, 2, 128)
tnp("tnp-mant-small16", 20, 64, 2, 3, 64, kind="mant")
tnp("tnp-mant-big", 33, 128, 2, 2, 128, kind="mant")

BY_NAME = {r["name"]: r for r in ROWS}

# what the table has to reach (tests/test_gram_fixtures.py compares SETS)
REQUIRED_INSTANCES = (
    {("TN", v, c) for v in (1, 4) for c in ("SMALL", "BIG", "WIDE")} | {("NT", 1, c) for c in ("SMALL", "BIG", "WIDE")}
    | {("NTB", 4, c) for c in ("SMALL", "BIG", "WIDE")} | {("CONV", v, c) for v in (1, 4) for c in ("SMALL", "BIG", "WIDE")}
    | {("XCORR", v, c) for v in (1, 4) for c in ("SMALL", "BIG")} | {("TNP", 4, "SMALL16"), ("TNP", 4, "BIG")})
assert len(REQUIRED_INSTANCES) == 24


# ---- the query ------------------------------------------------------------------------------------------------------------------
def nt_vec4_ok(row):
    return row["mis"] is None


def variants(K, row):
    """what the built library says the row's launches run: a list parallel to ``row['expect']``"""
    e = row["entry"]
    if e == "tn":
        return [K.gram_launch_variant(TN, row["n"], row["K"], 0, row["ldx"] % 4 == 0 and row["off"] == 0, row["flags"])]
    if e == "nt":
        return [K.gram_launch_variant(NT, row["n"], row["nseg"] * row["nb"], row["L"], nt_vec4_ok(row), row["flags"])]
    if e == "conv":
        OH, OW = conv_out_hw(row)
        return [K.gram_launch_variant(CONV, row["n"], row["B"] * OH * OW, 0, row["Cin"] % 4 == 0 and row["off"] == 0, row["flags"])]
    if e == "xcorr":
        B, H, W = row["B"], row["H"], row["W"]
        return [K.gram_launch_variant(XCORR_FULL, row["Cin"], B * H * W, 0, row["off"] == 0, 0),
                K.gram_launch_variant(XCORR_STRIPS, row["Cin"], B * max(H, W), 0, row["off"] == 0, 0)]
    import ctypes

    out = (ctypes.c_int64 * 3)()
    a = ctypes.addressof(out)
    rc = K.lib.lk_conv3x3_pixpair_plan(row["H"], row["W"], row["Cin"], ctypes.c_void_p(a), ctypes.c_void_p(a + 8), ctypes.c_void_p(a + 16))
    assert rc == 0
    T = int(out[0])
    return [dict(tile=T, mode="TNP", vec=4, cfg="SMALL16" if T == 64 else "BIG", T=T, BK=16, epilogue="direct", nsplit=1, two_level=False,
                 n_tiles=int(out[1]), n_blocks=int(out[2]), nchunks=-(-row["B"] // 16), chunks_per_split=-(-row["B"] // 16))]


def conv_out_hw(row):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = row["k"], row["s"], row["p"], row["d"]
    return (row["H"] + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (row["W"] + 2 * pw - dw * (kw - 1) - 1) // sw + 1


# ---- operands and references ----------------------------------------------------------------------------------------------------
class Built:
    pass


def _values(kind, shape, rng):
    if kind == "ints":
        return rng.integers(-8, 9, size=shape).astype(np.float32)
    m = rng.integers(0, 1 << 23, size=shape, dtype=np.int64)  # 1.m with all 23 mantissa bits drawn
    return (1.0 + m.astype(np.float64) * 2.0 ** -23).astype(np.float32)


def operand_shape(row):
    e = row["entry"]
    if e == "tn":
        return (row["launches"], row["K"], row["n"])
    if e == "nt":
        return (row["launches"], row["nseg"], row["nb"], row["n"], row["L"])
    return (row["B"], row["H"], row["W"], row["Cin"])  # NHWC


def rows_count(row):
    """K of the bound: products summed per output element"""
    e = row["entry"]
    if e == "tn":
        return row["K"] * row["launches"]
    if e == "nt":
        return row["nseg"] * row["nb"] * row["L"] * row["launches"]
    if e == "conv":
        OH, OW = conv_out_hw(row)
        return row["B"] * OH * OW
    if e == "xcorr":
        return row["B"] * row["H"] * row["W"]
    return row["B"]


def unfold_native64(x, k, s, p, d):
    """fp64 patch matrix [B * OH * OW][(kh, kw, ci)] of NHWC ``x`` through torch's F.unfold (independent of ``patch_rows``)"""
    import torch
    import torch.nn.functional as F

    B, H, W, C = x.shape
    cols = F.unfold(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2), k, dilation=d, padding=p, stride=s)  # [B][(ci, kh, kw)][L]
    cols = cols.view(B, C, k[0] * k[1], -1).permute(0, 3, 2, 1)  # [B][L][(kh, kw)][ci]
    return cols.reshape(-1, k[0] * k[1] * C).numpy()


def build(row, seed=None):
    """operands, C0, alpha, the fp64 reference ``want`` of the whole of C (both triangles) and, for ``mant``, the bound"""
    import zlib

    seed = zlib.crc32(row["name"].encode()) if seed is None else seed
    rng = np.random.default_rng(seed)
    o = Built()
    kind, e = row["kind"], row["entry"]
    o.x = _values(kind, operand_shape(row), rng)
    o.K = rows_count(row)
    f = np.float64
    if e == "tn":
        X = o.x.reshape(-1, row["n"]).astype(f)
        G = X.T @ X
    elif e == "nt":
        X = o.x.astype(f).transpose(0, 1, 2, 4, 3).reshape(-1, row["n"])  # rows (launch, seg, b, l)
        G = X.T @ X
    elif e == "tnp":
        G = None
    else:
        c = row if e == "conv" else dict(k=(3, 3), s=(1, 1), p=(1, 1), d=(1, 1))
        X = unfold_native64(o.x, c["k"], c["s"], c["p"], c["d"])
        G = X.T @ X
    if e == "tnp":
        B, H, W, C = o.x.shape
        x = o.x.astype(f)
        blocks = []
        for y in range(H):
            for xx in range(W):
                for dy, dx in HALF:
                    if 0 <= y + dy < H and 0 <= xx + dx < W:
                        blocks.append(x[:, y, xx, :].T @ x[:, y + dy, xx + dx, :])
        G = np.stack(blocks)  # [n_blocks][Cin][Cin] in the slot order of lk_conv3x3_pixpair_tables
    if kind == "ints":
        assert 64 * o.K + 64 < 1 << 24, row["name"]
        o.alpha = [0.5, 1.0, 2.0][seed % 3]
        c0 = rng.integers(-64, 65, size=G.shape).astype(f)
        o.C0 = (np.triu(c0) + np.triu(c0, 1).T if G.ndim == 2 else c0).astype(np.float32)
        o.tol = None
    else:
        assert o.K <= 128, row["name"]
        o.alpha = 1.0
        o.C0 = np.zeros(G.shape, np.float32)
        M = G if e != "xcorr" else xcorr_assemble(o.x.astype(f), lambda A, Bm, which: A.T @ Bm, sign=+1.0, dtype=f)
        o.tol = (o.K + 10) * U * M
    o.want = o.C0.astype(f) + o.alpha * G
    return o


def ratio(got, o):
    """worst |got - want| / bound over every element (``mant`` rows)"""
    err = np.abs(np.asarray(got, np.float64) - o.want)
    with np.errstate(divide="ignore", invalid="ignore"):  # (a block no pixel pair reaches has M = 0: it has to be exactly 0)
        return float(np.where(err == 0, 0.0, err / o.tol).max())


# ---- the stand-in ---------------------------------------------------------------------------------------------------------------
def split3(x):
    xi = x.view(np.uint32)
    h = (xi & np.uint32(0xFFFF0000)).view(np.float32)
    r1 = x - h
    m = (r1.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    return h, m, r1 - m


def _chunk_product(acc, A, Bm, mode, exact, mutant):
    """acc (fp32) += A^T B over the rows of one chunk, as one workgroup accumulates them"""
    f = np.float64
    if mode == "NTB":
        pa, pb = split3(np.ascontiguousarray(A)), split3(np.ascontiguousarray(Bm))
        terms = [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)]  # small terms first: l h', h l', m m', m h', h m', h h'
        if mutant == "ntb_drop_lh":
            terms = terms[1:]
        for r0 in range(0, A.shape[0], 16):  # one MFMA sums 16 rows, one rounding into the accumulator
            for p, q in terms:
                acc = (acc.astype(f) + pa[p][r0:r0 + 16].astype(f).T @ pb[q][r0:r0 + 16].astype(f)).astype(np.float32)
        return acc
    if exact:
        return acc + A.T @ Bm  # (fp32 matmul: integers, exact in any order)
    for r in range(A.shape[0]):
        acc = (acc.astype(f) + np.outer(A[r].astype(f), Bm[r].astype(f))).astype(np.float32)
    return acc


def split_partials(A, Bm, var, exact, mutant=None):
    """the slabs of one launch: [nsplit][nA][nB] fp32 partial products (A, Bm: virtual rows [K][nA], [K][nB])"""
    BK, cps, nsplit = var["BK"], var["chunks_per_split"], var["nsplit"]
    Kv = A.shape[0]
    my_chunks = max(-(-Kv // BK), 1)
    slabs = np.zeros((nsplit, A.shape[1], Bm.shape[1]), np.float32)
    for s in range(nsplit):
        for c in range(s * cps, min(my_chunks, (s + 1) * cps)):
            r0, r1 = c * BK, min(Kv, (c + 1) * BK)
            if mutant == "drop_ragged_chunk" and r1 - r0 < BK and c == my_chunks - 1:
                continue
            if r1 > r0:
                slabs[s] = _chunk_product(slabs[s], A[r0:r1], Bm[r0:r1], var["mode"], exact, mutant)
    return slabs


def reduce_slabs(slabs, two_level):
    """gram_reduce_kernel's sum: slab after slab in fp32, groups of 32 first beyond 32 slabs"""
    if two_level:
        groups = []
        for g0 in range(0, len(slabs), 32):
            s = slabs[g0].copy()
            for k in range(g0 + 1, min(len(slabs), g0 + 32)):
                s = s + slabs[k]
            groups.append(s)
        slabs = groups
    s = np.zeros_like(slabs[0])
    for k in range(len(slabs)):
        s = s + slabs[k]
    return s


def place_tiles(C, S, T, upper_only, mutant=None):
    """C += S by tile pairs bi <= bj (diagonal tiles whole), the off-diagonal ones mirrored unless ``upper_only``"""
    n = C.shape[0]
    nbt = -(-n // T)
    P = np.zeros((nbt * T, nbt * T), np.float32)
    P[:n, :n] = S
    out = np.zeros_like(P)
    out[:n, :n] = C
    for bi in range(nbt):
        for bj in range(bi, nbt):
            t = P[bi * T:(bi + 1) * T, bj * T:(bj + 1) * T]
            out[bi * T:(bi + 1) * T, bj * T:(bj + 1) * T] += t
            if bi != bj and not upper_only:
                out[bj * T:(bj + 1) * T, bi * T:(bi + 1) * T] += t if mutant == "mirror_untransposed" else t.T
    return out[:n, :n].copy()


def patch_rows(x, row):
    """the virtual rows of MODE_CONV: [B * OH * OW][(kh, kw, ci)] by index arithmetic, zero outside the image"""
    B, H, W, C = x.shape
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = row["k"], row["s"], row["p"], row["d"]
    OH, OW = conv_out_hw(row)
    X = np.zeros((B, OH, OW, kh * kw, C), x.dtype)
    for oh in range(OH):
        for ow in range(OW):
            for dy in range(kh):
                for dx in range(kw):
                    ih, iw = oh * sh + dy * dh - ph, ow * sw + dx * dw - pw
                    if 0 <= ih < H and 0 <= iw < W:
                        X[:, oh, ow, dy * kw + dx, :] = x[:, ih, iw, :]
    return X.reshape(B * OH * OW, kh * kw * C)


def nt_rows(x, BK):
    """the virtual rows of MODE_NT: (seg, b, l) with every image padded to a whole number of chunks"""
    nseg, nb, n, L = x.shape
    Lp = -(-L // BK) * BK
    X = np.zeros((nseg * nb, Lp, n), x.dtype)
    X[:, :L, :] = x.reshape(nseg * nb, n, L).transpose(0, 2, 1)
    return X.reshape(nseg * nb * Lp, n)


def shifted_rows(x, region, shifts):
    """A [K_r][Cin] = x over the region, B [K_r][nshift * Cin] = the zero-extended x at q + shift"""
    B, H, W, C = x.shape
    h0, w0, h, w = region
    A = x[:, h0:h0 + h, w0:w0 + w, :].reshape(-1, C)
    xp = np.zeros((B, H + 4, W + 4, C), x.dtype)
    xp[:, 2:H + 2, 2:W + 2, :] = x
    Bs = [xp[:, h0 + 2 + dy:h0 + 2 + dy + h, w0 + 2 + dx:w0 + 2 + dx + w, :].reshape(-1, C) for dy, dx in shifts]
    return A, np.concatenate(Bs, axis=1)


def xcorr_regions(H, W):
    return [(0, 0, 1, W), (H - 1, 0, 1, W), (0, 0, H, 1), (0, W - 1, H, 1), (0, 0, 1, 1), (0, W - 1, 1, 1), (H - 1, 0, 1, 1), (H - 1, W - 1, 1, 1)]


def xcorr_assemble(x, product, sign=-1.0, dtype=np.float32):
    """shiftcorr_assemble_kernel: A[(d,ci),(e,cj)] = R[e-d] - Row - Col + Pix (``sign`` = +1: the four terms added, for the bound);
    ``product(A, B, which)`` forms one region's correlation, which = 'full' or the region index of the strips launch"""
    B, H, W, C = x.shape
    Rf = product(*shifted_rows(x, (0, 0, H, W), HALF), "full")
    regs = [product(*shifted_rows(x, reg, ALL25), i) for i, reg in enumerate(xcorr_regions(H, W))]
    out = np.zeros((9 * C, 9 * C), dtype)
    blk = lambda M, t: M[:, t * C:(t + 1) * C]  # noqa: E731
    for d in range(9):
        for e in range(9):
            dy, dx = d // 3 - 1, d % 3 - 1
            t = ((e // 3 - 1) - dy + 2) * 5 + ((e % 3 - 1) - dx + 2)
            v = blk(Rf, HALF_INDEX[t]) if HALF_INDEX[t] >= 0 else blk(Rf, HALF_INDEX[24 - t]).T
            v = v.astype(dtype)
            sr = {1: 0, -1: 1}.get(dy, -1)
            sc = {1: 2, -1: 3}.get(dx, -1)
            if sr >= 0:
                v = v + dtype(sign) * blk(regs[sr], t)
            if sc >= 0:
                v = v + dtype(sign) * blk(regs[sc], t)
            if sr >= 0 and sc >= 0:
                v = v + blk(regs[4 + sr * 2 + (sc - 2)], t)
            out[d * C:(d + 1) * C, e * C:(e + 1) * C] = v
    return out


def emulate(row, o, var, mutant=None):
    """the row as the kernels compute it, in numpy: fp32 C after the launch(es) -- ``var``: the list ``variants`` returned"""
    exact = row["kind"] == "ints"
    e = row["entry"]
    alpha = np.float32(o.alpha)
    if e == "xcorr":
        vf, vs = var

        def product(A, Bm, which):  # (a region runs its own chunks in the split geometry of the launch's longest one)
            v = vf if which == "full" else vs
            return reduce_slabs(split_partials(A, Bm, v, exact, mutant), v["two_level"])

        return o.C0 + alpha * xcorr_assemble(o.x, product)
    v = var[0]
    if e == "tnp":
        B, H, W, C = o.x.shape
        out, i = o.C0.copy(), 0
        for y in range(H):
            for xx in range(W):
                for dy, dx in HALF:
                    if 0 <= y + dy < H and 0 <= xx + dx < W:
                        acc = split_partials(o.x[:, y, xx, :], o.x[:, y + dy, xx + dx, :], v, exact, mutant)[0]
                        out[i] = out[i] + alpha * acc
                        i += 1
        return out
    upper = bool(row["flags"] & UPPER)
    launches = []
    for la in range(row["launches"] if "launches" in row else 1):
        if e == "tn":
            X = o.x[la]
        elif e == "nt":
            X = nt_rows(o.x[la], v["BK"])
        else:
            X = patch_rows(o.x, row)
        launches.append(split_partials(X, X, v, exact, mutant))
    if v["epilogue"] == "direct":
        return place_tiles(o.C0, alpha * launches[0][0], v["T"], True, mutant)
    slabs = launches[0]
    for more in launches[1:]:  # persistent slabs: slab += partial
        slabs = slabs + more
    S = reduce_slabs(slabs, v["two_level"]) * alpha
    return place_tiles(o.C0, S, v["T"], upper, mutant)
