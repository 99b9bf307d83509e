"""Every launch form of the split-fp16 Gram engine (laplace_amd/csrc/lk_sweep16.hip) at the edges of its loops, through the C ABI
itself (so that the workspace, zero16, the scale word and every pointer are the test's own): gram16_kernel in its four
instantiations, pixpair13_kernel, gram16_reduce4_kernel<64 | 128>.

Per row of the table (tests/test_gram16_fixtures.py proves on the CPU that the table reaches every form and that each row's claim
is what the library's host functions plan):
  * both planes sit inside bands of fp16 NaN one stage deep (a read of rows past the end shows up as NaN in the result, not as a
    fault), zero16 is EXACTLY 16 zero bytes inside NaN bands, the workspace EXACTLY the advertised byte count, filled with NaN,
    inside bands of -0.0, G / the blocks inside bands of -0.0; every band intact afterwards, no NaN in the result
  * ``ints`` and ``scale``: bit equality -- on every element of the upper 32 x 32 tiles of G, every element of the tiles below
    them bit-equal to G0; on every element of every pixel-pair block (a block exists exactly for the in-map shifts: the slot table)
  * ``mant``: planes from lk_split_f16x2 on the device, every element inside (3 R + 16) 2^-24 M, none exempt
  * a second identical launch into a fresh copy is bit-identical
and R = 0 / B = 0 leave the output bit-unchanged, and route against route on ``ints`` operands with l = 0, exactly:
pixpair13 == one workgroup per block == the fp32 pixel-pair engine; lk_gram_tn_f16x2 == lk_gram_tn_f32 (upper only).
Worst error / bound per form: profiles/gram16_instances.md.  -m gpu only."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import gram16_fixtures as gf

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 1024  # floats in front of and behind G, the blocks and the workspace
WORST = {}
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def K():
    from laplace_amd._lib import get_kernels

    return get_kernels()


@pytest.fixture(scope="module", autouse=True)
def _report():
    """the worst error / bound per form, printed when the module is done (pytest -s): what profiles/gram16_instances.md records"""
    yield
    for form, (r, name, units) in sorted(WORST.items()):
        print(f"\n{form:6s} worst error / bound {r:.4f}  = {units:.2f} units of 2^-24 M  ({name})", end="")


class Guards:
    """fp32 buffers with a band of -0.0 on both sides (a stray `+= 0` flips the sign bit, a stray store changes the value)"""

    def __init__(self):
        self.items = []

    def new(self, shape, fill):
        n = math.prod(shape)
        buf = torch.full((n + 2 * GUARD,), -0.0, dtype=torch.float32, device=DEV)
        v = buf[GUARD:GUARD + n].view(shape)
        if isinstance(fill, np.ndarray):
            v.copy_(torch.from_numpy(fill))
        else:
            v.fill_(fill)
        self.items.append((buf, n))
        return v

    def check(self, what):
        torch.cuda.synchronize()
        for buf, n in self.items:
            band = torch.cat([buf[:GUARD], buf[GUARD + n:]])
            assert bool((torch.signbit(band) & (band == 0)).all()), f"{what}: wrote outside a buffer of {n} floats"


class Banded16:
    """an fp16 array [rows][cols] inside bands of fp16 NaN ``band_rows`` rows deep"""

    def __init__(self, arr, band_rows):
        arr = arr if torch.is_tensor(arr) else torch.from_numpy(np.ascontiguousarray(arr))
        self.n = arr.numel()
        self.band = -(-band_rows * arr.shape[1] // 8) * 8  # (whole 16-byte units: the payload stays aligned)
        self.buf = torch.full((self.n + 2 * self.band,), float("nan"), dtype=torch.float16, device=DEV)
        self.buf[self.band:self.band + self.n].copy_(arr.reshape(-1))
        self.ptr = self.buf.data_ptr() + 2 * self.band
        assert self.ptr % 16 == 0
        self.before = self.buf[self.band:self.band + self.n].clone()

    def check(self, what):
        b = self.buf
        assert bool(torch.isnan(torch.cat([b[:self.band], b[self.band + self.n:]])).all()), f"{what}: a NaN band of an operand was written"
        assert torch.equal(b[self.band:self.band + self.n].view(torch.int16), self.before.view(torch.int16)), f"{what}: an operand was written"


def bits(t):
    return t.contiguous().view(torch.int32)


class Operands:
    """the device side of a row's inputs: planes per launch, the scale words, zero16, the pixel-pair tables"""

    def __init__(self, K, row, o):
        c = row["claim"]
        cols = row["C"] if row["entry"] == "tn" else row["H"] * row["W"] * row["Cin"]
        self.planes, self.sexp = [], []
        for la in range(row["launches"]):
            if row["kind"] == "mant":  # the planes come from lk_split_f16x2 -- and are the ones the stand-in was given
                st = K.split_f16x2(torch.from_numpy(o.x[la]).to(DEV))
                torch.cuda.synchronize()
                assert int(st.sexp.item()) == o.sexp[la]
                for plane, mine in zip(st.planes, (o.h[la], o.l[la])):
                    assert torch.equal(plane.cpu().view(torch.int16), torch.from_numpy(mine).view(torch.int16)), row["name"]
                h, l, s = st.planes[0].reshape(-1, cols), st.planes[1].reshape(-1, cols), st.sexp.clone()
            else:
                h, l, s = o.h[la], o.l[la], torch.tensor([o.sexp[la]], dtype=torch.int32, device=DEV)
            self.planes.append((Banded16(h, c["bkr"]), Banded16(l, c["bkr"])))
            self.sexp.append(s)
        self.zero = Banded16(np.zeros((1, 8), np.float16), 8)  # exactly 16 zero bytes
        if row["entry"] == "pp":
            tiles = torch.zeros(max(c["n_tiles"], 1) * 3, dtype=torch.int32)
            slots = torch.zeros(row["H"] * row["W"] * 13, dtype=torch.int32)
            rc = K.lib.lk_conv3x3_pixpair_tables(row["H"], row["W"], row["Cin"], vp(tiles.data_ptr()), vp(slots.data_ptr()))
            assert rc == 0
            self.tiles, self.slots = tiles.to(DEV), slots.to(DEV)

    def check(self, what):
        for h, l in self.planes:
            h.check(what), l.check(what)
        self.zero.check(what)


def launch(K, row, o, ops, out, ws, nbytes, la, R=None):
    """launch ``la`` of the row through the C ABI (``R``: another row / image count over the same buffers)"""
    st = K._stream(torch.device(DEV))
    R = row["R"] if R is None else R
    (h, l), s, z, a = ops.planes[la], ops.sexp[la], ops.zero, float(o.alpha)
    if row["entry"] == "tn":
        K._rc(K.lib.lk_gram_tn_f16x2(vp(h.ptr), vp(l.ptr), vp(s.data_ptr()), R, row["C"], a, vp(out.data_ptr()), vp(z.ptr), vp(ws.data_ptr()),
                                     nbytes, st), "lk_gram_tn_f16x2")
    elif row["form"] == "pix13":
        K._rc(K.lib.lk_conv3x3_pixpair_accumulate13_f16x2(vp(h.ptr), vp(l.ptr), vp(s.data_ptr()), R, row["H"], row["W"], row["Cin"], a,
                                                          vp(out.data_ptr()), vp(ops.slots.data_ptr()), vp(z.ptr), st),
              "lk_conv3x3_pixpair_accumulate13_f16x2")
    else:
        K._rc(K.lib.lk_conv3x3_pixpair_accumulate_f16x2(vp(h.ptr), vp(l.ptr), vp(s.data_ptr()), R, row["H"], row["W"], row["Cin"], a,
                                                        vp(out.data_ptr()), vp(ops.tiles.data_ptr()), row["claim"]["n_tiles"], vp(z.ptr), st),
              "lk_conv3x3_pixpair_accumulate_f16x2")


def run(K, row, o, ops, R=None):
    """all launches of the row into guarded buffers -> G or the blocks on the host"""
    G = Guards()
    out = G.new(o.G0.shape, o.G0)
    nbytes = int(K.lib.lk_gram_tn_f16x2_workspace_bytes(row["R"], row["C"])) if row["entry"] == "tn" else 0
    assert nbytes % 4 == 0 and (nbytes > 0) == (row["entry"] == "tn")
    ws = G.new((max(nbytes // 4, 1),), float("nan"))
    for la in range(row["launches"]):
        launch(K, row, o, ops, out, ws, nbytes, la, R)
    G.check(row["name"])
    ops.check(row["name"])
    if R == 0:
        assert bool(torch.isnan(ws).all()), f"{row['name']}: an empty launch wrote the workspace"
    return out.cpu()


def check_exact(row, o, got):
    want = o.want.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), o.want)
    g, g0 = got.numpy(), o.G0
    if row["entry"] == "tn":
        up = gf.upper_tiles(row["C"])
        bad = (g.view(np.int32) != want.view(np.int32)) & up
        assert not bad.any(), f"{row['name']}: {bad.sum()} elements of the upper tiles differ, first at {np.argwhere(bad)[0].tolist()}: " \
                              f"{g[tuple(np.argwhere(bad)[0])]!r} for {want[tuple(np.argwhere(bad)[0])]!r}"
        assert np.array_equal(g[~up].view(np.int32), g0[~up].view(np.int32)), f"{row['name']}: a tile below the diagonal was written"
    else:
        bad = g.view(np.int32) != want.view(np.int32)
        assert not bad.any(), f"{row['name']}: {bad.sum()} block elements differ, first at {np.argwhere(bad)[0].tolist()}: " \
                              f"{g[tuple(np.argwhere(bad)[0])]!r} for {want[tuple(np.argwhere(bad)[0])]!r}"


@pytest.mark.parametrize("name", [r["name"] for r in gf.ROWS])
def test_row_is_exact_or_within_its_bound_inside_its_buffers_and_reproducible(K, name):
    row, o = gf.BY_NAME[name], gf.build(name)
    ops = Operands(K, row, o)
    got = run(K, row, o, ops)
    assert got.shape == o.want.shape  # (pixel pairs: one block per in-map shift, none for the others)
    assert not torch.isnan(got).any(), f"{name}: NaN in the result (rows past the end, or workspace nobody wrote, were read)"
    if row["kind"] == "mant":
        r = gf.ratio(row, got.numpy(), o)
        units = r * (3 * row["R"] + 16)
        print(f"{name}: error / bound = {r:.4f}  (R = {row['R']}: {units:.2f} units of 2^-24 M)")
        if r > WORST.get(row["form"], (-1.0,))[0]:
            WORST[row["form"]] = (r, name, units)
        assert r <= 1.0, (name, r)
    else:
        check_exact(row, o, got)
    again = run(K, row, o, ops)
    assert torch.equal(bits(again), bits(got)), f"{name}: a second identical launch differs"


@pytest.mark.parametrize("name", ["tn64-R65", "tn128-c256-3pairs", "pp64-c192-1x3-B63", "pp128-c256-2x2-B32", "pix13-3x3-B17"])
def test_an_empty_launch_leaves_the_output_bit_unchanged(K, name):
    row, o = gf.BY_NAME[name], gf.build(name)
    got = run(K, row, o, Operands(K, row, o), R=0)
    assert torch.equal(bits(got), bits(torch.from_numpy(o.G0))), f"{name}: R = 0 changed the output"


# ---- route against route, exactly (l = 0: the term the split engine drops is zero) ----------------------------------------------
def test_pixpair13_one_workgroup_per_block_and_the_fp32_engine_agree_exactly(K):
    geo = dict(entry="pp", B=33, H=3, W=3, Cin=64)
    r13, r64 = gf.adhoc("route-pixel-pairs", form="pix13", **geo), gf.adhoc("route-pixel-pairs", form="pp64", **geo)
    o = gf.build_row(r13)
    assert not o.l.any() and o.sexp == [0]
    a = run(K, r13, o, Operands(K, r13, o))
    ops = Operands(K, r64, o)
    b = run(K, r64, o, ops)
    G = Guards()
    blocks = G.new(o.G0.shape, o.G0)
    x = torch.from_numpy(o.h[0].astype(np.float32)).to(DEV)
    assert x.data_ptr() % 16 == 0
    K._rc(K.lib.lk_conv3x3_pixpair_accumulate_f32(vp(x.data_ptr()), 33, 3, 3, 64, float(o.alpha), vp(blocks.data_ptr()), vp(ops.tiles.data_ptr()),
                                                  r64["claim"]["n_tiles"], K._stream(torch.device(DEV))), "lk_conv3x3_pixpair_accumulate_f32")
    G.check("fp32 pixel pairs")
    want = torch.from_numpy(o.want.astype(np.float32))
    for what, g in (("pixpair13", a), ("one workgroup per block", b), ("fp32 engine", blocks.cpu())):
        assert torch.equal(bits(g), bits(want)), what


@pytest.mark.parametrize("R,C", [(300, 64), (300, 256)])
def test_the_split_gram_and_the_fp32_gram_agree_exactly_on_the_upper_triangle(K, R, C):
    row = gf.adhoc(f"route-tn-{C}", entry="tn", R=R, C=C)
    o = gf.build_row(row)
    a = run(K, row, o, Operands(K, row, o))
    G = Guards()
    Gm = G.new(o.G0.shape, o.G0)
    nbytes = int(K.lib.lk_gram_workspace_bytes(C, R))
    ws = G.new((max(nbytes // 4, 1),), float("nan"))
    x = torch.from_numpy(o.h[0].astype(np.float32)).to(DEV)
    K._rc(K.lib.lk_gram_tn_f32(vp(x.data_ptr()), R, C, C, float(o.alpha), vp(Gm.data_ptr()), 1, vp(ws.data_ptr()), nbytes,
                               K._stream(torch.device(DEV))), "lk_gram_tn_f32")
    G.check("fp32 Gram")
    tri = torch.from_numpy(np.triu(np.ones((C, C), bool)))
    want = torch.from_numpy(o.want.astype(np.float32))
    assert torch.equal(bits(a)[tri], bits(want)[tri]) and torch.equal(bits(Gm.cpu())[tri], bits(want)[tri])
