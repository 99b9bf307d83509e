"""Every launch form of the fp32 Gram engine (laplace_amd/csrc/lk_gram.hip) at its edges, through the C ABI itself (so that ldx,
flags, the workspace and the pointer offsets are the test's own): gram_kernel<MODE, VEC, CFG> in its 24 reachable instantiations,
the three epilogues, the slab reduction in its four shapes.

Per row of the table (tests/test_gram_fixtures.py proves on the CPU that the table reaches every form):
  * the launch takes the form the row claims (``lk_gram_launch_variant``, asked on THIS device)
  * C sits inside bands of -0.0; the workspace is EXACTLY the advertised byte count, filled with NaN beforehand (zero for
    persistent slabs), inside bands of its own; both sets of bands intact afterwards, no NaN in C
  * ``ints``: bit equality with the integer Gram over all of C; under LK_GRAM_UPPER_ONLY every (i <= j) exact, every (i > j)
    equal to C0 or to the reference and to nothing else, whole T x T tiles strictly below the diagonal bit-equal to C0
  * ``mant``: every element inside (K + 10) 2^-24 M, none exempt
  * a second identical launch is bit-identical; K = 0 and nb = 0 leave C bit-unchanged
and route against route on the same ``ints`` operands, exactly: shift-correlation == implicit im2col == pixel-pair assemble,
segments == the stacked tensor, two persistent launches == one launch of the concatenation.  Worst error / bound per family:
profiles/gram_instances.md.  -m gpu only."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import gram_fixtures as gf

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 1024  # elements in front of and behind C and the workspace
WORST = {}


@pytest.fixture(scope="module")
def K():
    from laplace_amd._lib import get_kernels

    return get_kernels()


@pytest.fixture(scope="module", autouse=True)
def _report():
    """the worst error / bound per family, printed when the module is done (pytest -s): what profiles/gram_instances.md records"""
    yield
    for key, (r, name) in sorted(WORST.items()):
        print(f"\n{key:8s} worst error / bound {r:.4f}  ({name})", end="")


class Guards:
    """buffers with a band of -0.0 on both sides (a stray `+= 0` flips the sign bit, a stray store changes the value)"""

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


def place(arr, off=0):
    """a device copy of ``arr`` that starts ``off`` floats past a 16-byte boundary -> (keep-alive, address)"""
    flat = np.ascontiguousarray(arr, np.float32).reshape(-1)
    buf = torch.full((flat.size + 8,), float("nan"), dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf[off:off + flat.size].copy_(torch.from_numpy(flat))
    return buf, buf.data_ptr() + 4 * off


def bits(t):
    return t.contiguous().view(torch.int32)


class Operands:
    def __init__(self, K, row, o):
        e = row["entry"]
        self.keep, self.ptrs = [], []
        if e == "tn":
            for la in range(row["launches"]):
                X = np.full((row["K"], row["ldx"]), np.nan, np.float32)  # (the padding of a row must never be read)
                X[:, :row["n"]] = o.x[la]
                buf, p = place(X, row["off"])
                self.keep.append(buf), self.ptrs.append(p)
        elif e == "nt":
            for la in range(row["launches"]):
                segs = []
                for s in range(row["nseg"]):
                    buf, p = place(o.x[la, s], 1 if row["mis"] == s else 0)
                    self.keep.append(buf), segs.append(p)
                self.ptrs.append(segs)
        else:
            buf, p = place(o.x, row.get("off", 0))
            self.keep.append(buf), self.ptrs.append(p)
        if e == "tnp":
            v, = gf.variants(K, row)
            self.n_tiles, self.n_blocks = v["n_tiles"], v["n_blocks"]
            tiles = torch.zeros(self.n_tiles * 3, dtype=torch.int32)
            slots = torch.zeros(row["H"] * row["W"] * 13, dtype=torch.int32)
            rc = K.lib.lk_conv3x3_pixpair_tables(row["H"], row["W"], row["Cin"], ctypes.c_void_p(tiles.data_ptr()), ctypes.c_void_p(slots.data_ptr()))
            assert rc == 0
            self.tiles, self.slots = tiles.to(DEV), slots.to(DEV)


def workspace_bytes(K, row):
    e = row["entry"]
    if e == "tn":
        return int(K.lib.lk_gram_workspace_bytes(row["n"], row["K"]))
    if e == "nt":
        return int(K.lib.lk_gram_nt_workspace_bytes(row["nseg"] * row["nb"], row["n"], row["L"]))
    if e == "conv":
        OH, OW = gf.conv_out_hw(row)
        return int(K.lib.lk_gram_workspace_bytes(row["n"], row["B"] * OH * OW))
    if e == "xcorr":
        return int(K.lib.lk_conv3x3_shiftcorr_workspace_bytes(row["B"], row["H"], row["W"], row["Cin"]))
    return 0


def run(K, row, o, ops):
    """launch the row through the C ABI into guarded buffers -> C on the host"""
    e = row["entry"]
    st = K._stream(torch.device(DEV))
    G = Guards()
    C = G.new(o.C0.shape, o.C0)
    nbytes = workspace_bytes(K, row)
    assert nbytes % 4 == 0
    persist = bool(row["flags"] & gf.PERSIST)
    ws = G.new((max(nbytes // 4, 1),), 0.0 if persist else float("nan"))
    vp = ctypes.c_void_p
    a, fl = float(o.alpha), int(row["flags"])
    for la in range(row.get("launches", 1)):
        if e == "tn":
            K._rc(K.lib.lk_gram_tn_f32(vp(ops.ptrs[la]), row["K"], row["n"], row["ldx"], a, vp(C.data_ptr()), fl, vp(ws.data_ptr()), nbytes, st),
                  "lk_gram_tn_f32")
        elif e == "nt":
            segs = (ctypes.c_void_p * row["nseg"])(*ops.ptrs[la])
            K._rc(K.lib.lk_gram_nt_seg_f32(ctypes.cast(segs, vp), row["nseg"], row["nb"], row["n"], row["L"], a, vp(C.data_ptr()), fl,
                                           vp(ws.data_ptr()), nbytes, st), "lk_gram_nt_seg_f32")
        elif e == "conv":
            (kh, kw), (sh, sw), (ph, pw), (dh, dw) = row["k"], row["s"], row["p"], row["d"]
            K._rc(K.lib.lk_gram_conv_nhwc_f32(vp(ops.ptrs[0]), row["B"], row["H"], row["W"], row["Cin"], kh, kw, sh, sw, ph, pw, dh, dw, a,
                                              vp(C.data_ptr()), fl, vp(ws.data_ptr()), nbytes, st), "lk_gram_conv_nhwc_f32")
        elif e == "xcorr":
            K._rc(K.lib.lk_conv3x3_shiftcorr_f32(vp(ops.ptrs[0]), row["B"], row["H"], row["W"], row["Cin"], a, vp(C.data_ptr()),
                                                 vp(ws.data_ptr()), nbytes, st), "lk_conv3x3_shiftcorr_f32")
        else:
            K._rc(K.lib.lk_conv3x3_pixpair_accumulate_f32(vp(ops.ptrs[0]), row["B"], row["H"], row["W"], row["Cin"], a, vp(C.data_ptr()),
                                                          vp(ops.tiles.data_ptr()), ops.n_tiles, st), "lk_conv3x3_pixpair_accumulate_f32")
    if persist:
        torch.cuda.synchronize()
        assert torch.equal(bits(C), bits(torch.from_numpy(o.C0).to(DEV))), "a persistent launch touched C"
        K._rc(K.lib.lk_gram_slabs_reduce_f32(vp(ws.data_ptr()), nbytes, row["n"], row.get("L", 0), a, vp(C.data_ptr()), fl & gf.UPPER, st),
              "lk_gram_slabs_reduce_f32")
    G.check(row["name"])
    return C.cpu()


def check_ints(row, o, got, T):
    want = torch.from_numpy(o.want.astype(np.float32))
    c0 = torch.from_numpy(o.C0)
    assert np.array_equal(want.double().numpy(), o.want)  # (the reference is representable: integers and halves below 2^24)
    if not (row["flags"] & gf.UPPER) or got.dim() != 2:
        bad = (got != want).nonzero()
        assert torch.equal(got, want), f"{row['name']}: {len(bad)} elements differ, first at {bad[0].tolist()}"
        return
    n = got.shape[0]
    idx = torch.arange(n)
    upper = idx[:, None] <= idx[None, :]
    assert torch.equal(got[upper], want[upper]), f"{row['name']}: upper triangle, first at {((got != want) & upper).nonzero()[0].tolist()}"
    low = ~upper
    assert bool(((got == want) | (bits(got) == bits(c0)))[low].all()), f"{row['name']}: an element below the diagonal is neither C0 nor the result"
    below = (idx // T)[:, None] > (idx // T)[None, :]
    assert torch.equal(bits(got)[below], bits(c0)[below]), f"{row['name']}: a tile strictly below the diagonal was written"


def check_mant(row, o, got):
    err = np.abs(got.double().numpy() - o.want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / o.tol)
    if row["flags"] & gf.UPPER and got.dim() == 2:  # below the diagonal: the result, or C0 untouched
        n = got.shape[0]
        low = np.tril(np.ones((n, n), bool), -1)
        untouched = bits(got).numpy() == bits(torch.from_numpy(o.C0)).numpy()
        r = np.where(low & untouched, 0.0, r)
    worst = float(r.max())
    fam = row["expect"][0].get("mode", "TNP")
    print(f"{row['name']}: error / bound = {worst:.4f}  (K = {o.K}: {worst * (o.K + 10):.2f} units of 2^-24 M)")
    if worst > WORST.get(fam, (-1.0, ""))[0]:
        WORST[fam] = (worst, row["name"])
    assert worst <= 1.0, (row["name"], worst)


@pytest.mark.parametrize("name", [r["name"] for r in gf.ROWS])
def test_row_is_exact_or_within_its_bound_inside_its_buffers_and_reproducible(K, name):
    row = gf.BY_NAME[name]
    var = gf.variants(K, row)
    for v, ex in zip(var, row["expect"]):
        assert v is not None and {k: v[k] for k in ex} == ex, (name, v)
    o = gf.build(row)
    ops = Operands(K, row, o)
    got = run(K, row, o, ops)
    assert not torch.isnan(got).any(), f"{name}: NaN in C (uninitialised workspace or operand padding was read)"
    if row["kind"] == "ints":
        check_ints(row, o, got, var[0]["T"])
        if gf.rows_count(row) == 0:  # K = 0, nb = 0
            assert torch.equal(bits(got), bits(torch.from_numpy(o.C0))), f"{name}: an empty product changed C"
    else:
        check_mant(row, o, got)
    again = run(K, row, o, ops)
    assert torch.equal(bits(again), bits(got)), f"{name}: a second identical launch differs"


# ---- route against route, exactly --------------------------------------------------------------------------------------------
def _ad_hoc(**kw):
    row = dict(kind="ints", flags=0, off=0, launches=1, mis=None)
    row.update(kw)
    return row


def test_shift_correlation_implicit_im2col_and_pixel_pair_assemble_agree_exactly(K):
    B, H, W, Cin = 2, 4, 4, 64
    geo = dict(B=B, H=H, W=W, Cin=Cin, n=9 * Cin)
    rows = [_ad_hoc(name="route-3x3", entry="xcorr", **geo), _ad_hoc(name="route-3x3", entry="conv", k=(3, 3), s=(1, 1), p=(1, 1), d=(1, 1), **geo)]
    o = gf.build(rows[0])
    got = [run(K, r, o, Operands(K, r, o)) for r in rows]
    # pixel-pair: blocks from zero with alpha = 1, then the assembly into C0 with the row's alpha (both triangles)
    rp = _ad_hoc(name="route-3x3", entry="tnp", **geo)
    rp["flags"] = gf.UPPER
    ob = gf.build(rp)
    assert np.array_equal(ob.x, o.x)
    ob.C0, ob.alpha = np.zeros_like(ob.C0), 1.0
    ops = Operands(K, rp, ob)
    blocks = run(K, rp, ob, ops).to(DEV)
    G = Guards()
    A = G.new(o.C0.shape, o.C0)
    vp = ctypes.c_void_p
    K._rc(K.lib.lk_conv3x3_pixpair_assemble_f32(vp(blocks.data_ptr()), vp(ops.slots.data_ptr()), H, W, Cin, float(o.alpha), vp(A.data_ptr()),
                                                K._stream(torch.device(DEV))), "lk_conv3x3_pixpair_assemble_f32")
    G.check("pixel-pair assemble")
    want = torch.from_numpy(o.want.astype(np.float32))
    for what, g in zip(("shift-correlation", "implicit im2col", "pixel-pair"), got + [A.cpu()]):
        assert torch.equal(g, want), what


def test_segments_equal_the_stacked_tensor_exactly(K):
    geo = dict(entry="nt", n=100, L=17, nb=2)
    seg = _ad_hoc(name="route-segments", nseg=3, **geo)
    o = gf.build(seg)
    a = run(K, seg, o, Operands(K, seg, o))
    stacked = _ad_hoc(name="route-segments", nseg=1, **{**geo, "nb": 6})
    os_ = gf.build(stacked)
    os_.x, os_.C0, os_.want = o.x.reshape(1, 1, 6, 100, 17), o.C0, o.want
    assert os_.alpha == o.alpha
    b = run(K, stacked, os_, Operands(K, stacked, os_))
    assert torch.equal(a, torch.from_numpy(o.want.astype(np.float32))) and torch.equal(bits(a), bits(b))


def test_two_persistent_launches_equal_one_launch_of_the_concatenation_exactly(K):
    two = _ad_hoc(name="route-persist", entry="tn", n=200, K=300, ldx=200, flags=gf.PERSIST, launches=2)
    o = gf.build(two)
    a = run(K, two, o, Operands(K, two, o))
    one = _ad_hoc(name="route-persist", entry="tn", n=200, K=600, ldx=200)
    o1 = gf.build(one)
    o1.x, o1.C0, o1.want = o.x.reshape(1, 600, 200), o.C0, o.want
    assert o1.alpha == o.alpha
    b = run(K, one, o1, Operands(K, one, o1))
    assert torch.equal(a, torch.from_numpy(o.want.astype(np.float32))) and torch.equal(bits(a), bits(b))
