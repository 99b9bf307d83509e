"""Seeded operands, the fp64 reference, the element-wise tolerance and the table of launches for the split-fp16 convolution
engine (laplace_amd/csrc/lk_conv.hip: ``conv_f16x2_kernel`` in five tile shapes with its plain / split-planes / VJP / forward
epilogues, ``conv_winp_f16x2_kernel`` in two configurations, ``conv_strided_f16x2_kernel`` in two tile shapes).
tests/test_conv_fixtures.py pins, on the CPU, that the table reaches every instantiation and every structural edge (through
``lk_conv_launch_variant``: the launchers decide with the same helpers) and that the tolerance holds for the arithmetic and is
sharp against three mutants of it; tests/test_gpu_conv_instances.py holds the kernels to it on the device.

TEST INFRASTRUCTURE (touches no device), in the style of tests/quad_fixtures.py.

Operands (``build``): NOT i.i.d. unit normals.
  * inputs / cotangents ``x [N, Hi, Wi, K]``: flavour ``relu`` (about half exact zeros) or ``dense`` (no zeros: |v| >= 0.25, so a
    read across an image boundary or of an out-of-image tap always changes the result), times one factor per image
    10^U(-3, 0) (image 0: 1, image 1: 1e-3 — both extremes present) and one per channel 10^U(-1, 0)
  * weights: normal times one factor per output channel 10^U(-2, 0)
  * addend: 0.3 of the convolution's rms (per image); byte mask: about 60 % ones; fp32 multiplier in [-0.5, 1.5]; channel
    scale in [0.25, 1.75]

Reference (``build``): the same operation in fp64 from the fp32 operands — ``F.conv2d`` / ``conv2d_input`` in double, then add,
multiply, scale — and the absolute convolution A = |x| (*) |W| with the same taps.

Tolerance (element-wise, from the contract at the head of lk_conv.hip; not tuned):
  plain fp32 output   tol = 2^-20 A + 2^-38 (max|x_n| sum|W[n]| + max|W| sum_window|x|)
                      three relative terms of 2^-22 (the split of each operand, the dropped l l') with margin, and the 2^-39
                      fixed-point floor of each operand, doubled; max|x_n|: of the image with per-image scales, else the tensor's
  VJP epilogue        o = (conv + add) m s:  (tol + 2^-22 |add|) |m s| + 2^-21 |o| + 2^-38 B_out
                      B_out = (max|in| l1(W) [+ 2^(15 - add.sexp)]) max|m| max|s|, the guaranteed bound the launch scales its
                      planes from (summed over both sources of the strided form); ``out_sexp`` must be the exponent it gives
  forward epilogue    y = act(conv s + t + addend) in fp32: tol |s| + 2^-22 (|conv s| + |t| + |addend|)  (two fp32 roundings of
                      partial results no larger than the sum of the terms, with margin; ReLU is 1-Lipschitz); its planes
                      add 2^-21 |y| + 2^-38 B_out[n],  B_out[n] = max|x_n| l1(W) max|s| + max|t| + bound(addend)[n]
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from laplace_amd.conv import _backward_plan

#: (BM, BN) of config bits 12..14
TILES = {1: (64, 64), 2: (128, 64), 3: (64, 128), 4: (128, 128), 5: (256, 64)}
BIT_NCHW, BIT_NO_PMAJOR, BIT_PM_LIMIT, BIT_ONE_WG, BIT_SPLIT, BIT_WIN512, BIT_NO_WIN, BIT_COLOC, BIT_HALO = (
    1 << 4, 1 << 15, 1 << 16, 1 << 19, 1 << 25, 1 << 26, 1 << 27, 1 << 28, 1 << 30)
VJP_VARIANTS = {"none": (), "add": ("add",), "mask": ("mask",), "fmult": ("fmult",), "scale": ("scale",),
                "all": ("add", "mask", "scale"), "allf": ("add", "fmult", "scale")}


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def R(name, entry, Kc, Nc, H, W, N, k=3, s=1, p=1, dir=None, tile=0, cfg=0, flavour="dense", expect=None, **opts):
    """one row.  ``entry``: plain / planes / forward / vjp / strided; ``Kc`` / ``Nc``: channels of the GEMM's K and N side (forward:
    cin / cout, backward-data: cout / cin); ``H x W``: the convolution's INPUT map (what backward-data writes); ``opts``: per_image,
    accumulate, vjp (a key of VJP_VARIANTS), seeds, amax (in_amax given), act, addend (0 / 1 / 'N' bounds), namax ('N' or 1),
    mask, planes, pair, os, x2_scale; ``expect``: the items of the launch variant the row exists for"""
    if dir is None:
        dir = "bwd" if entry in ("vjp", "strided") else "fwd"
    row = dict(name=name, entry=entry, dir=dir, Kc=Kc, Nc=Nc, H=H, W=W, N=N, k=_pair(k), s=s, p=_pair(p), config=2 | (tile << 12) | cfg,
               flavour=flavour, expect=dict(expect or {}), family="strided" if entry == "strided" else "generic")
    row.update(opts)
    if tile:
        row["expect"].setdefault("bm", TILES[tile][0]), row["expect"].setdefault("bn", TILES[tile][1])
    return row


def _table():
    rows = []
    # ---- generic kernel: every tile shape with every epilogue (4 x 4 maps: Ho Wo % 16 == 0 for the planes; 9 images: 144 rows,
    #      tiles that span images, a ragged one; 72 columns: BN + 8 of the narrow tiles, a ragged half tile of the wide ones)
    for t in TILES:
        for e in ("plain", "planes", "forward", "vjp"):
            rows.append(R(f"tile{t}-{e}", e, 64, 72, 4, 4, 9, tile=t, vjp="all", seeds=3, act=1, addend="N", namax="N",
                          per_image=e != "vjp", expect={"kernel": "generic", "epilogue": e}))
    # ---- M against BM (1 x 1 taps on 1 x M maps, one 32-channel chunk: nstage = 1), Co = 8
    for t, bm in ((1, 64), (2, 128), (5, 256), (4, 128)):
        for M in (bm - 1, 2 * bm - 1, 2 * bm + 1):
            rows.append(R(f"tile{t}-M{M}", "plain" if t != 4 else "vjp", 32, 8, 1, M, 1, k=1, p=0, tile=t, vjp="add", expect={"nb_m": -(-M // bm)}))
    # ---- column edges: 8, BN + 8, and on the plain epilogue 1 and 3
    for t, co in ((1, 72), (3, 136), (4, 136), (5, 72), (2, 8), (3, 8)):
        for e in ("plain", "vjp", "forward"):
            rows.append(R(f"tile{t}-{e}-co{co}", e, 32, co, 3, 5, 5, tile=t, vjp="scale", act=0, expect={"nb_n": -(-co // TILES[t][1])}))
    for co in (1, 3):
        for t in (1, 4):
            rows.append(R(f"tile{t}-plain-co{co}", "plain", 32, co, 3, 5, 5, tile=t))
    # ---- K stages: the ring is two deep (1: prologue only, 2: no steady state, 3: one steady step), odd chunk counts
    for Kc, ns in ((32, 1), (64, 2), (96, 3)):
        for e in ("plain", "vjp", "forward", "planes"):
            rows.append(R(f"nstage{ns}-{e}", e, Kc, 64, 4, 4, 5, k=1, p=0, tile=1, vjp="mask", act=1, nstage=ns))
    rows.append(R("ci96-3x3-plain", "plain", 96, 40, 5, 6, 3))
    rows.append(R("ci96-3x3-vjp", "vjp", 96, 40, 5, 6, 3, vjp="add"))
    # ---- tap sets, strides that do not divide the size
    for name, k, p in (("1x1", 1, 0), ("3x3p1", 3, 1), ("3x3p0", 3, 0), ("2x2p0", 2, 0), ("1x3p01", (1, 3), (0, 1))):
        rows.append(R(f"taps-{name}-fwd", "plain", 32, 40, 5, 7, 3, k=k, p=p))
        rows.append(R(f"taps-{name}-bwd", "plain", 32, 40, 5, 7, 3, k=k, p=p, dir="bwd", flavour="relu"))
    rows.append(R("fwd-stride2", "plain", 32, 40, 7, 6, 3, s=2))
    rows.append(R("fwd-stride3", "plain", 32, 40, 11, 8, 3, s=3))
    rows.append(R("fwd-stride2-forward", "forward", 32, 40, 7, 6, 3, s=2, act=1, addend=1))
    # ---- backward class launches (out_step = 2): every (oh0, ow0) on odd and even sizes, the other classes left alone
    for H, W in ((6, 6), (7, 7), (7, 6), (6, 7)):
        rows.append(R(f"classes-3x3s2-{H}x{W}", "plain", 32, 40, H, W, 3, s=2, dir="bwd", expect={"dense": False}))
    rows.append(R("classes-1x1s2-7x6", "plain", 32, 40, 7, 6, 3, k=1, s=2, p=0, dir="bwd", expect={"dense": False}))
    rows.append(R("classes-3x3s2-acc", "plain", 32, 40, 6, 7, 3, s=2, dir="bwd", accumulate=True, flavour="relu"))
    # ---- maps
    for H, W in ((1, 1), (1, 9), (9, 1), (3, 5), (7, 7)):
        rows.append(R(f"map-{H}x{W}-plain", "plain", 32, 40, H, W, 5))
        rows.append(R(f"map-{H}x{W}-vjp", "vjp", 32, 40, H, W, 6, vjp="all", seeds=2))
    rows.append(R("image-over-tiles-17x17", "plain", 32, 40, 17, 17, 2, tile=5, expect={"nb_m": 3}))
    rows.append(R("image-over-tiles-17x17-vjp", "vjp", 32, 40, 17, 17, 2, tile=5, vjp="all"))
    rows.append(R("image-over-tiles-17x17-forward", "forward", 32, 40, 17, 17, 2, tile=2, act=1, addend="N", namax="N", per_image=True))
    # ---- position-major rows
    for e in ("plain", "vjp", "forward"):
        kw = dict(vjp="all", seeds=2, act=1, addend="N", namax="N", per_image=e != "vjp")
        rows.append(R(f"pmajor-n64-{e}", e, 32, 40, 2, 2, 64, expect={"pmajor": True}, **kw))
        rows.append(R(f"pmajor-n63-{e}", e, 32, 40, 2, 2, 63, expect={"pmajor": False}, **dict(kw, seeds=3)))
        rows.append(R(f"pmajor-hw64-{e}", e, 32, 40, 8, 8, 64, expect={"pmajor": True}, **kw))
        rows.append(R(f"pmajor-hw65-{e}", e, 32, 40, 5, 13, 64, expect={"pmajor": False}, **kw))
        rows.append(R(f"pmajor-9x9-lifted-{e}", e, 32, 40, 9, 9, 64, cfg=BIT_PM_LIMIT, expect={"pmajor": True}, **kw))
        rows.append(R(f"pmajor-n70-{e}", e, 32, 40, 3, 3, 70, tile=2, expect={"pmajor": True}, **kw))
        rows.append(R(f"pmajor-corner-tile-{e}", e, 32, 40, 4, 4, 64, tile=1, expect={"pmajor": True, "nb_m": 16}, **kw))
        rows.append(R(f"pmajor-off-{e}", e, 32, 40, 4, 4, 64, tile=1, cfg=BIT_NO_PMAJOR, expect={"pmajor": False}, **kw))
    # ---- accumulate, position-contiguous fp32 output, one scale per image
    rows.append(R("accumulate", "plain", 64, 40, 5, 6, 3, accumulate=True))
    rows.append(R("accumulate-bwd", "plain", 64, 40, 5, 6, 3, dir="bwd", accumulate=True))
    for t in (1, 4, 5):
        rows.append(R(f"nchw-tile{t}", "plain", 32, 40, 6, 6, 5, tile=t, cfg=BIT_NCHW, expect={"out_nchw": True}))
    rows.append(R("nchw-per-image", "plain", 32, 40, 2, 2, 7, cfg=BIT_NCHW, per_image=True, expect={"out_nchw": True}))
    rows.append(R("per-image-plain", "plain", 32, 40, 5, 6, 7, per_image=True))
    rows.append(R("per-image-planes", "planes", 32, 40, 4, 8, 7, per_image=True, amax=True))
    rows.append(R("planes-one-scale", "planes", 32, 40, 4, 8, 7))
    rows.append(R("planes-hw16-odd-m", "planes", 32, 72, 4, 4, 3, tile=1))
    # ---- VJP variants, the mask shared by 1 / 2 / 3 seeds (mask_rows wraps inside a tile), in_amax given and NULL
    for v in VJP_VARIANTS:
        for seeds in (1, 2, 3):
            rows.append(R(f"vjp-{v}-s{seeds}", "vjp", 32, 40, 3, 5, 6, vjp=v, seeds=seeds, amax=seeds == 2, tile=2 if seeds == 3 else 0))
    # ---- forward variants
    for act in (0, 1):
        for addend, namax in ((0, 1), (1, "N"), ("N", 1), ("N", "N")):
            rows.append(R(f"forward-act{act}-add{addend}-namax{namax}", "forward", 32, 40, 5, 6, 5, act=act, addend=addend, namax=namax,
                          per_image=namax == "N"))
    rows.append(R("forward-no-mask", "forward", 32, 40, 5, 6, 5, act=1, addend=1, mask=False))
    rows.append(R("forward-no-planes", "forward", 32, 40, 5, 6, 5, act=1, addend=1, planes=False))

    # ---- persistent window form: both configurations of every row (bit 26: the 512-row one)
    def Wn(name, Kc, Nc, H, W, N, cfg=0, expect=None, **opts):
        for bm, bit in ((256, 0), (512, BIT_WIN512)):
            ex = dict(kernel=f"window-{bm}", bm=bm, bn=64, epilogue="vjp")
            ex.update(expect or {})
            r = R(f"win{bm}-{name}", "vjp", Kc, Nc, H, W, N, cfg=cfg | bit, expect=ex, wc=True, **opts)
            r["family"] = "window"
            rows.append(r)

    for i, (N, H, W) in enumerate(((32, 4, 4), (32, 2, 8), (32, 1, 16), (32, 16, 1))):
        Wn(f"512px-{H}x{W}", 32, 64, H, W, N, vjp=("none", "add", "mask", "scale")[i], seeds=2)
    Wn("wi47-1x47", 32, 64, 1, 47, 11, vjp="all")
    Wn("wi47-2x47", 32, 64, 2, 47, 6, vjp="mask", seeds=2)
    Wn("5x5x21", 32, 64, 5, 5, 21, vjp="all", seeds=3)
    Wn("20x20", 32, 64, 20, 20, 2, vjp="add")
    Wn("17x17", 96, 64, 17, 17, 2, vjp="all", seeds=2)
    Wn("24x24", 32, 64, 24, 24, 1, vjp="scale")
    for co in (128, 192, 256):
        Wn(f"co{co}", 32, co, 6, 6, 15, vjp="all", seeds=3, flavour="relu")
    Wn("ci96-co128", 96, 128, 6, 6, 15, vjp="none")
    # co-located columns: 1 / 2 / 4 by default, and by bits 28-29 (eight pixel tiles: the grid is a multiple of 8 c)
    Wn("coloc1-default", 32, 128, 8, 8, 12, vjp="mask", expect={"coloc": 1})
    Wn("coloc2-default", 32, 128, 16, 16, 16, vjp="mask", expect={"coloc": 2})
    Wn("coloc4-default", 32, 256, 16, 16, 16, vjp="add", expect={"coloc": 4})
    Wn("coloc2-forced", 32, 256, 16, 16, 16, cfg=BIT_COLOC, vjp="none", expect={"coloc": 2})
    Wn("coloc4-forced", 32, 256, 16, 16, 16, cfg=2 * BIT_COLOC, vjp="scale", expect={"coloc": 4})
    Wn("coloc4-refused", 32, 128, 16, 16, 16, cfg=2 * BIT_COLOC, vjp="none", expect={"coloc": 1})
    Wn("halo-all", 32, 64, 5, 7, 20, cfg=BIT_HALO, vjp="all", seeds=2)
    Wn("one-wg-per-cu", 32, 64, 5, 7, 20, cfg=BIT_ONE_WG, vjp="all", seeds=2, expect={"wg_per_cu": 1})
    # walks over several tiles per workgroup and the split tail: the image count follows the grid the query reports
    Wn("walk", 32, 256, 8, 8, "walk", vjp="mask", flavour="relu", expect={"walk": True})
    Wn("split2", 64, 256, 8, 8, "walk", cfg=BIT_SPLIT, vjp="all", flavour="relu", expect={"split_S": 2})
    Wn("split4", 128, 256, 8, 8, "walk", cfg=BIT_SPLIT, vjp="add", flavour="relu", expect={"split_S": 4})
    r = R("float-mult-leaves-the-window", "vjp", 32, 64, 4, 4, 32, vjp="fmult", wc=True, expect={"kernel": "generic"})
    r["family"] = "window"
    rows.append(r)

    # ---- strided form
    for co, bm, bn in ((8, 256, 64), (64, 256, 64), (72, 128, 128), (136, 128, 128)):
        for pair in (False, True):
            rows.append(R(f"strided-co{co}-{'pair' if pair else 'single'}", "strided", 32, co, 6, 6, 5, s=2, pair=pair, vjp="all" if pair else "mask",
                          expect={"kernel": "strided", "bm": bm, "bn": bn, "ncls": 4}))
    for H, W in ((2, 2), (2, 6), (6, 2)):
        rows.append(R(f"strided-map-{H}x{W}", "strided", 32, 40, H, W, 6, s=2, pair=True, vjp="add", seeds=2, expect={"kernel": "strided"}))
    rows.append(R("strided-os1", "strided", 32, 40, 3, 5, 5, s=1, pair=True, vjp="all", expect={"kernel": "strided", "ncls": 1, "dense": True}))
    rows.append(R("strided-ragged-tile", "strided", 32, 72, 6, 6, 15, s=2, pair=True, vjp="scale", seeds=3,
                  expect={"kernel": "strided", "nb_m": 2}))
    rows.append(R("strided-units-2^30", "strided", 64, 40, 4, 4, 5, s=2, pair=True, vjp="add", x_scale=1e-6, x2_scale=1e3,
                  expect={"kernel": "strided"}))
    for v in ("none", "add", "mask", "fmult", "allf"):
        rows.append(R(f"strided-vjp-{v}", "strided", 32, 40, 4, 6, 6, s=2, pair=True, vjp=v, seeds=2, amax=v == "add", expect={"kernel": "strided"}))
    names = [r["name"] for r in rows]
    assert len(set(names)) == len(names)
    return rows


ROWS = _table()
BY_NAME = {r["name"]: r for r in ROWS}
#: rows whose CPU emulation runs on their first images only (the device runs them in full)
EMULATED_IMAGES = 48


# ---- geometry ----------------------------------------------------------------------------------------------------------------
def out_hw(row):
    (KH, KW), (ph, pw), s = row["k"], row["p"], row["s"]
    return (row["H"] + 2 * ph - KH) // s + 1, (row["W"] + 2 * pw - KW) // s + 1


def resolve(row, K):
    """the row with its image count: 'walk' rows take it from the grid the query reports for the device (or 256 CUs), so that
    the walk has between grid + 1 and 1.5 grid tiles: 17 / 16 of the grid, in whole groups of eight pixel tiles"""
    if row["N"] != "walk":
        return row
    probe = dict(row, N=1 << 14)
    grid = variant(K, probe, launches(probe)[0])["grid"]
    bm = row["expect"]["bm"]
    nb_n = row["Nc"] // 64
    nb_m = -(-(grid + grid // 16) // nb_n // 8) * 8
    return dict(row, N=nb_m * bm // (row["H"] * row["W"]))


def gemm_in_hw(row):
    return (row["H"], row["W"]) if row["dir"] == "fwd" else out_hw(row)


def gemm_out_hw(row):
    return out_hw(row) if row["dir"] == "fwd" else (row["H"], row["W"])


def launches(row):
    """the launches of a row: dicts ``Hc, Wc, in_mul, out_step, oh0, ow0, taps`` (forward: one dense launch; backward-data: one
    per residue class that owns a tap; strided: one launch, ``taps`` in rows of six)"""
    (KH, KW), (ph, pw), s = row["k"], row["p"], row["s"]
    if row["entry"] == "strided":
        taps = []
        for src, (k, p) in enumerate(((row["k"], row["p"]), ((1, 1), (0, 0)))[: 2 if row.get("pair") else 1]):
            for Hc, Wc, oh0, ow0, tp in _backward_plan(s, p, k, row["H"], row["W"]):
                taps += [(dh, dw, sl, src, oh0, ow0) for dh, dw, sl in tp]
        return [dict(Hc=row["H"] // s, Wc=row["W"] // s, in_mul=1, out_step=s, oh0=0, ow0=0, taps=taps)]
    if row["dir"] == "fwd":
        Ho, Wo = out_hw(row)
        return [dict(Hc=Ho, Wc=Wo, in_mul=s, out_step=1, oh0=0, ow0=0, taps=[(kh - ph, kw - pw, kh * KW + kw) for kh in range(KH) for kw in range(KW)])]
    return [dict(Hc=Hc, Wc=Wc, in_mul=1, out_step=s, oh0=oh0, ow0=ow0, taps=list(taps))
            for Hc, Wc, oh0, ow0, taps in _backward_plan(s, row["p"], row["k"], row["H"], row["W"]) if taps and Hc and Wc]


def variant(K, row, launch):
    """what ``lk_conv_launch_variant`` says the launch runs"""
    Hi, Wi = gemm_in_hw(row)
    Ho, Wo = gemm_out_hw(row)
    if row["entry"] == "strided":
        return K.conv_strided_launch_variant(row["N"], Hi, Wi, row["Kc"], row["Nc"], Ho, Wo, row["s"], launch["taps"], bool(row.get("pair")))
    entry = {"plain": K.CONV_PLAIN, "planes": K.CONV_PLANES, "forward": K.CONV_BN_ACT, "vjp": K.CONV_VJP}[row["entry"]]
    return K.conv_launch_variant(entry, row["N"], Hi, Wi, row["Kc"], row["Nc"], Ho, Wo, launch["taps"], Hc=launch["Hc"], Wc=launch["Wc"],
                                 in_mul=launch["in_mul"], out_step=launch["out_step"], oh0=launch["oh0"], ow0=launch["ow0"],
                                 in_nsexp=row["N"] if row.get("per_image") else 1, have_wc=bool(row.get("wc")),
                                 mask_is_float="fmult" in VJP_VARIANTS.get(row.get("vjp"), ()) and row["entry"] == "vjp", config=row["config"])


# ---- operands ------------------------------------------------------------------------------------------------------------------
def _field(g, shape, flavour, scale=1.0):
    N, C = shape[0], shape[-1]
    v = torch.randn(shape, generator=g)
    v = v.relu() if flavour == "relu" else torch.sign(v) * (0.25 + v.abs())
    img = 10.0 ** (-3.0 * torch.rand(N, generator=g))
    img[0] = 1.0
    if N > 1:
        img[1] = 1e-3
    ch = 10.0 ** (-torch.rand(C, generator=g))
    return (v * img.reshape(N, 1, 1, 1) * ch * scale).contiguous()


def _weights(g, row, k):
    cout, cin = (row["Nc"], row["Kc"]) if row["dir"] == "fwd" else (row["Kc"], row["Nc"])
    return (torch.randn(cout, cin, *k, generator=g) * (10.0 ** (-2.0 * torch.rand(cout, generator=g))).reshape(-1, 1, 1, 1)).contiguous()


def conv(row, x, W, k=None, p=None):
    """the row's convolution of NHWC ``x`` (any float dtype) -> NHWC: ``F.conv2d`` (forward) or ``conv2d_input`` (backward-data)"""
    k, p = k or row["k"], p if p is not None else row["p"]
    xn = x.permute(0, 3, 1, 2)
    if row["dir"] == "fwd":
        y = F.conv2d(xn, W, None, row["s"], p)
    else:
        y = torch.nn.grad.conv2d_input((x.shape[0], W.shape[1], row["H"], row["W"]), W, xn, stride=row["s"], padding=p)
    return y.permute(0, 2, 3, 1).contiguous()


def l1_of(row, W):
    """l1(W) as conv.PreparedConv builds it: max over the GEMM's output channels of the summed |W|"""
    return W.abs().double().sum(dim=(1, 2, 3) if row["dir"] == "fwd" else (0, 2, 3)).max().item()


def pow2_above(a):
    """2^(15 - sexp) of a tensor split with its own max|.| = a: the next power of two above it"""
    return 2.0 ** (math.floor(math.log2(a)) + 1) if a > 0 else 2.0 ** -125


def sexp_of(bound):
    return min(120, 14 - math.floor(math.log2(bound))) if bound > 2.0 ** -126 else 120


def _sources(row, o):
    return [(o.x, o.W, row["k"], row["p"])] + ([(o.x2, o.W2, (1, 1), (0, 0))] if row.get("pair") else [])


@functools.lru_cache(maxsize=4)
def _build(name, N):
    row = dict(BY_NAME[name], N=N)
    g = torch.Generator().manual_seed(sum(ord(c) * (i + 1) for i, c in enumerate(name)) % (1 << 31))
    Hi, Wi = gemm_in_hw(row)
    Ho, Wo = gemm_out_hw(row)
    Nc = row["Nc"]
    o = SimpleNamespace(row=row)
    o.x = _field(g, (N, Hi, Wi, row["Kc"]), row["flavour"], row.get("x_scale", 1.0))
    o.W = _weights(g, row, row["k"])
    if row.get("pair"):
        o.x2 = _field(g, (N, Hi, Wi, row["Kc"]), row["flavour"], row.get("x2_scale", 3.0))
        o.W2 = _weights(g, row, (1, 1))
    per_image = bool(row.get("per_image"))
    # fp64 convolution, its absolute companion and the fixed-point floor
    want = torch.zeros(N, Ho, Wo, Nc, dtype=torch.float64)
    tol = torch.zeros_like(want)
    o.bound_in = 0.0   # sum over the sources of max|in| l1(W), with the measured max or the power of two above it
    o.bound_in_n = None
    for x, W, k, p in _sources(row, o):
        xd, Wd = x.double(), W.double()
        want += conv(row, xd, Wd, k, p)
        xmax = xd.abs().amax(dim=(1, 2, 3), keepdim=True) if per_image else xd.abs().max().reshape(1, 1, 1, 1)
        ones_x, ones_w = torch.ones_like(xd), torch.ones_like(Wd)
        tol += 2.0 ** -20 * conv(row, xd.abs(), Wd.abs(), k, p)
        tol += 2.0 ** -38 * (conv(row, ones_x * xmax, Wd.abs(), k, p) + Wd.abs().max() * conv(row, xd.abs(), ones_w, k, p))
        amax = xd.abs().max().item()
        o.bound_in += (amax if row.get("amax") else pow2_above(amax)) * l1_of(row, W)
    o.conv, o.tol_conv = want, tol
    o.l1 = l1_of(row, o.W)
    if row["entry"] == "plain":
        if row.get("accumulate"):
            o.base = _field(g, (N, Ho, Wo, Nc), "dense", 0.5)
            want = want + o.base.double()
            tol = tol + 2.0 ** -23 * want.abs()  # (one fp32 rounding of the sum)
        o.want, o.tol = want, tol
    elif row["entry"] == "planes":
        xa = o.x.double().abs()
        bound = xa.amax(dim=(1, 2, 3)) if per_image else xa.max().reshape(1)
        if not row.get("amax"):
            bound = torch.tensor([pow2_above(b) for b in bound.tolist()], dtype=torch.float64)
        o.bound_out = bound * o.l1
        o.want, o.tol = want, tol + 2.0 ** -21 * want.abs() + 2.0 ** -38 * o.bound_out.reshape(-1, 1, 1, 1)
    elif row["entry"] in ("vjp", "strided"):
        parts = VJP_VARIANTS[row["vjp"]]
        S = row.get("seeds", 1)
        assert N % S == 0, name
        B = N // S
        o.S, o.B = S, B
        fac = torch.ones(1, 1, 1, 1, dtype=torch.float64)
        B_out, tol_add = o.bound_in, 0.0
        if "add" in parts:
            rms = want.pow(2).mean(dim=(1, 2, 3), keepdim=True).sqrt().float()
            o.add = (torch.randn(N, Ho, Wo, Nc, generator=g) * 0.3 * rms).contiguous()
            want = want + o.add.double()
            tol_add = 2.0 ** -22 * o.add.double().abs()
            B_out += pow2_above(o.add.abs().max().item())
        if "mask" in parts:
            o.mask = (torch.rand(B, Ho, Wo, Nc, generator=g) < 0.6).to(torch.uint8)
            fac = fac * o.mask.double().repeat(S, 1, 1, 1)
        if "fmult" in parts:
            o.fmult = (torch.rand(B, Ho, Wo, Nc, generator=g) * 2.0 - 0.5).contiguous()
            fac = fac * o.fmult.double().repeat(S, 1, 1, 1)
            B_out *= o.fmult.abs().max().item()
        if "scale" in parts:
            o.scale = (torch.rand(Nc, generator=g) * 1.5 + 0.25).contiguous()
            fac = fac * o.scale.double()
            B_out *= o.scale.abs().max().item()
        o.factor = fac
        o.want = want * fac
        o.bound_out = B_out
        o.tol = (tol + tol_add) * fac.abs() + 2.0 ** -21 * o.want.abs() + 2.0 ** -38 * B_out
    else:  # forward
        o.bn_scale = ((torch.rand(Nc, generator=g) * 1.5 + 0.25) * torch.where(torch.rand(Nc, generator=g) < 0.25, -1.0, 1.0)).contiguous()
        rms = want.pow(2).mean(dim=(1, 2, 3), keepdim=True).sqrt().float()
        o.bn_shift = (torch.randn(Nc, generator=g) * 0.2 * rms.min()).contiguous()
        pre = want * o.bn_scale.double() + o.bn_shift.double()
        mag = pre.abs() * 0 + (want * o.bn_scale.double()).abs() + o.bn_shift.double().abs()
        xa = o.x.double().abs()
        in_amax = xa.amax(dim=(1, 2, 3)) if row.get("namax") == "N" else xa.max().reshape(1)
        o.in_amax = in_amax.float()
        bound = in_amax.expand(N) * o.l1 * o.bn_scale.abs().max().item() + o.bn_shift.abs().max().item()
        if row.get("addend"):
            o.addend = (torch.randn(N, Ho, Wo, Nc, generator=g) * 0.3 * rms).contiguous()
            ab = o.addend.abs().amax(dim=(1, 2, 3)) if row["addend"] == "N" else o.addend.abs().max().reshape(1)
            o.addend_bound = ab.contiguous()
            pre = pre + o.addend.double()
            mag = mag + o.addend.double().abs()
            bound = bound + ab.double().expand(N)
        o.want = pre.relu() if row["act"] == 1 else pre
        o.bound_out = bound
        o.tol = tol * o.bn_scale.double().abs() + 2.0 ** -22 * mag
        o.tol_planes = o.tol + 2.0 ** -21 * o.want.abs() + 2.0 ** -38 * bound.reshape(-1, 1, 1, 1)
    return o


def build(row):
    """operands, fp64 reference and tolerance of a (resolved) row — CPU tensors, computed once and shared: do not modify"""
    return _build(row["name"], row["N"])


def ratio(got, want, tol):
    """worst |got - want| / tol over the elements (0 / 0 counts as 0: both exactly zero)"""
    err = (got.double().cpu() - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / tol)
    return float(torch.nan_to_num(r, nan=math.inf).max()) if r.numel() else 0.0  # (a NaN is outside every tolerance)


def class_mask(row, launch_list):
    """bool ``[Ho, Wo]``: the output pixels the row's launches write"""
    Ho, Wo = gemm_out_hw(row)
    m = torch.zeros(Ho, Wo, dtype=torch.bool)
    for la in launch_list:
        if row["entry"] == "strided":
            m[:] = True
        else:
            m[la["oh0"]::la["out_step"], la["ow0"]::la["out_step"]][: la["Hc"], : la["Wc"]] = True
    return m


# ---- the arithmetic of the kernels, emulated: fp16 pieces, l h' + h l' + h h', fp32 accumulation ------------------------------------
def split16(x, amax):
    """(h, l, 2^s) of fp32 ``x`` scaled so that ``amax`` (a tensor broadcastable to x) lands in [2^14, 2^15)"""
    e = torch.floor(torch.log2(amax.double().clamp_min(2.0 ** -126)))
    sc = torch.exp2(14 - e).clamp_max(2.0 ** 120).float()
    xs = x * sc
    h = xs.half().float()
    return h, (xs - h).half().float(), sc


def quantise(x, bound):
    """x as the two planes scaled from ``bound`` hold it"""
    h, l, sc = split16(x.float(), torch.as_tensor(bound, dtype=torch.float64).reshape(-1, *([1] * (x.dim() - 1))))
    return (h.double() + l.double()) / sc.double()


def emulate(row, o, keep=None, mutant=None):
    """the row's outputs as the kernels' arithmetic gives them, on the first ``keep`` images.  ``mutant``: 'cross' (l h' dropped),
    'tap' (one out-of-image tap read from the neighbouring row / image instead of zero), 'mask' (mask row off by one sample);
    returns None where the mutant does not apply to the row"""
    N = row["N"] if keep is None else min(keep, row["N"])
    per_image = bool(row.get("per_image"))
    acc = None
    for i, (x, W, k, p) in enumerate(_sources(row, o)):
        amax = x.abs().amax(dim=(1, 2, 3), keepdim=True)[:N] if per_image else x.abs().max().reshape(1, 1, 1, 1)
        xh, xl, sx = split16(x[:N], amax)
        wh, wl, sw = split16(W, W.abs().max().reshape(1, 1, 1, 1))
        c = conv(row, xh, wl, k, p) + conv(row, xh, wh, k, p)
        if mutant != "cross":
            c = c + conv(row, xl, wh, k, p)
        c = c.double() / (sx.double() * sw.double())
        acc = c if acc is None else acc + c
    if mutant == "tap":
        stray = _stray_tap(row, o, N)
        if stray is None:
            return None
        n, oh, ow, v = stray
        acc[n, oh, ow] += v
    acc = acc.float()
    e = row["entry"]
    if e == "plain":
        if mutant == "mask":
            return None
        return (acc + o.base[:N]) if row.get("accumulate") else acc
    if e == "planes":
        if mutant == "mask":
            return None
        b = o.bound_out if per_image else o.bound_out.expand(row["N"])
        return quantise(acc, b[:N])
    if e in ("vjp", "strided"):
        parts = VJP_VARIANTS[row["vjp"]]
        if mutant == "mask" and not ({"mask", "fmult"} & set(parts) and o.B > 1):
            return None
        v = acc
        if "add" in parts:
            v = v + quantise(o.add, o.add.abs().max().reshape(1).expand(row["N"]))[:N].float()
        f = torch.ones(1, dtype=torch.float32)
        for key in ("mask", "fmult"):
            if key in parts:
                m = getattr(o, key).float().repeat(o.S, 1, 1, 1)
                f = f * (m.roll(1, 0) if mutant == "mask" else m)[:N]
        if "scale" in parts:
            f = f * o.scale
        return quantise(v * f, torch.full((N,), o.bound_out))
    if mutant == "mask":
        return None
    y = acc * o.bn_scale + o.bn_shift
    if row.get("addend"):
        y = y + o.addend[:N]
    return y.relu() if row["act"] == 1 else y


def _stray_tap(row, o, N):
    """(n, oh, ow, values [Nc]) of ONE out-of-image tap of a launch read at its flat address — the neighbouring row or image
    of the NHWC tensor — or None when no tap of the row leaves the image over valid memory"""
    Hi, Wi = gemm_in_hw(row)
    x = o.x[:N].double().reshape(-1, row["Kc"])
    KH, KW = row["k"]
    for n, la in ((n, la) for n in (1, 0) for la in launches(row)):
        if n >= N:
            continue
        for i in range(la["Hc"]):
            for j in range(la["Wc"]):
                for tp in la["taps"]:
                    dh, dw, sl = tp[:3]
                    if len(tp) == 6 and (tp[3] != 0 or (tp[4], tp[5]) != (0, 0)):
                        continue
                    h, w = i * la["in_mul"] + dh, j * la["in_mul"] + dw
                    if 0 <= h < Hi and 0 <= w < Wi:
                        continue
                    flat = (n * Hi + h) * Wi + w
                    if not 0 <= flat < x.shape[0]:
                        continue
                    Wt = o.W.double()[:, :, sl // KW, sl % KW]          # [cout, cin]
                    v = Wt @ x[flat] if row["dir"] == "fwd" else Wt.T @ x[flat]
                    oh, ow = i * la["out_step"] + la["oh0"], j * la["out_step"] + la["ow0"]
                    if len(tp) == 6:
                        oh, ow = i * la["out_step"] + tp[4], j * la["out_step"] + tp[5]
                    return n, oh, ow, v
    return None
