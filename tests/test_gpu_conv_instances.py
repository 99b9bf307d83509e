"""Every launch form of the split-fp16 convolution engine (laplace_amd/csrc/lk_conv.hip) at its edges, held ELEMENT-WISE to the
tolerance of tests/conv_fixtures.py against the fp64 reference of the same operands: the generic kernel in its five tile shapes
with the plain / split-planes / VJP / forward epilogues, the persistent window form in both configurations, the strided form.

Per row of the table (tests/test_conv_fixtures.py proves on the CPU that the table reaches every instantiation and edge):
  * the launch runs what the row claims (``lk_conv_launch_variant``, asked on THIS device)
  * every element within the tolerance, no element exempt; every row keeps its fp64 reference
  * guard bands of -0.0 / sentinels in front of and behind EVERY output buffer (fp32 out, both planes, mask bytes, y, the sexp /
    bound / amax words); pixels of residue classes a launch does not own stay bit-unchanged
  * the amax word: bit-equal to max|out| over the written pixels (plain epilogue), within 1e-5 (fused epilogues)
  * planes |h| < 2^15, ``out_sexp`` the exponent of the guaranteed bound, forward mask bytes exactly ``y > 0``
  * a second identical launch is bit-identical
and route against route on the same operands: the five tile shapes, window against generic, split tail against unsplit, strided
against the class-by-class route.  Worst error / tolerance per family: profiles/conv_instances.md.  -m gpu only."""
import ctypes
import math

import pytest
import torch

from tests import conv_fixtures as cf

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 1024  # elements in front of and behind every output buffer
SENTINEL = {torch.uint8: 0xA5, torch.int32: -77777}
UNWRITTEN = -123456.0
WORST = {}


@pytest.fixture(scope="module")
def K():
    from laplace_amd._lib import get_kernels

    return get_kernels()


@pytest.fixture(scope="module", autouse=True)
def _report():
    """the worst error / tolerance per family, printed when the module is done (pytest -s): what profiles/conv_instances.md records"""
    yield
    for key, (r, name) in sorted(WORST.items()):
        print(f"\n{key:28s} worst error / tolerance {r:.4f}  ({name})", end="")


def note(key, r, name):
    if r > WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (r, name)


class Guards:
    """output buffers with a band of -0.0 (floats: a stray `+= 0` flips the sign bit, a stray store changes the value) or of a
    sentinel (bytes, words) on both sides"""

    def __init__(self):
        self.items = []

    def new(self, shape, dtype, fill=None):
        n = math.prod(shape)
        buf = torch.empty(n + 2 * GUARD, dtype=dtype, device=DEV)
        buf.fill_(-0.0 if dtype.is_floating_point else SENTINEL[dtype])
        v = buf[GUARD:GUARD + n].view(shape)
        if fill is not None:
            v.fill_(fill)
        self.items.append((buf, n))
        return v

    def check(self, what):
        torch.cuda.synchronize()
        for buf, n in self.items:
            band = torch.cat([buf[:GUARD], buf[GUARD + n:]])
            if buf.dtype.is_floating_point:
                ok = bool((torch.signbit(band) & (band == 0)).all())
            else:
                ok = bool((band == SENTINEL[buf.dtype]).all())
            assert ok, f"{what}: wrote outside a {buf.dtype} buffer of {n} elements"


def P(t):
    return None if t is None else t.data_ptr()


def planes_value(h, l, sexp):
    """fp64 value of two planes ``[N, ...]`` under ``sexp`` (1 or N words)"""
    s = sexp.double().reshape(-1, *([1] * (h.dim() - 1)))
    return ((h.double() + l.double()) * torch.exp2(-s)).cpu()


def word(t):
    """a float device word as the kernels leave it (bit pattern of a non-negative float)"""
    return t.cpu()


class Prepared:
    """the row's operands on the device, split as the producers of the sweep would hand them over"""

    def __init__(self, K, row, o):
        self.o = o
        bwd = row["dir"] == "bwd"
        self.src = []
        for x, W, k, p in cf._sources(row, o):
            xd = x.to(DEV)
            if row.get("per_image"):
                xs = K.split_images_f16x2(xd)
                if row["entry"] == "planes" and not row.get("amax"):
                    xs.amax = None  # (the bound is then 2^(15 - sexp[n]))
            else:
                xs = K.split_f16x2(xd)
                if row.get("amax") or row["entry"] == "forward":
                    xs.amax = K.absmax(xd)
            Wd = W.to(DEV)
            wp, ws = K.conv_prep_weights(Wd, bwd)
            l1 = Wd.abs().float().sum(dim=(0, 2, 3) if bwd else (1, 2, 3)).max().reshape(1).contiguous()
            self.src.append((xs, wp, ws, l1))
        self.wc = None
        if row.get("wc"):
            wp = self.src[0][1]
            two, T, N, Kd = wp.shape
            self.wc = wp.view(two, T, N, Kd // 16, 16).permute(0, 1, 3, 2, 4).contiguous()
        dev = lambda name: getattr(o, name).to(DEV).contiguous() if hasattr(o, name) else None  # noqa: E731
        self.add = K.split_f16x2(dev("add")) if hasattr(o, "add") else None
        self.mult = dev("mask") if hasattr(o, "mask") else dev("fmult")
        self.mult_amax = K.absmax(self.mult) if hasattr(o, "fmult") else None
        self.scale = dev("scale")
        self.scale_amax = K.absmax(self.scale) if self.scale is not None else None
        self.base = dev("base")
        if row["entry"] == "forward":
            self.bn_scale, self.bn_shift = dev("bn_scale"), dev("bn_shift")
            self.bn_scale_amax, self.bn_shift_amax = K.absmax(self.bn_scale), K.absmax(self.bn_shift)
            self.addend, self.addend_bound = dev("addend"), dev("addend_bound")


def run(K, row, prep, config=None):
    """launch the row (every class of a backward-data row) into guarded buffers -> dict of CPU results"""
    cfg = row["config"] if config is None else config
    o = prep.o
    N, Nc = row["N"], row["Nc"]
    Hi, Wi = cf.gemm_in_hw(row)
    Ho, Wo = cf.gemm_out_hw(row)
    G = Guards()
    xs, wp, ws, l1 = prep.src[0]
    st = K._stream(xs.planes.device)
    z = K._zero16(xs.planes.device)
    res = {}
    las = cf.launches(row)
    e = row["entry"]
    flat3 = lambda taps: (ctypes.c_int * (3 * len(taps)))(*[int(v) for t in taps for v in t])  # noqa: E731
    if e == "plain":
        out = G.new((N, Ho, Wo, Nc), torch.float32, UNWRITTEN)
        if row.get("accumulate"):
            out.copy_(prep.base)
        amax = G.new((1,), torch.float32, 0.0)
        for la in las:
            before = out.clone()
            K.conv_nhwc_f16x2(xs, wp, ws, la["Hc"], la["Wc"], la["in_mul"], out, la["out_step"], la["oh0"], la["ow0"], la["taps"],
                              accumulate=bool(row.get("accumulate")), amax_out=amax, config=cfg)
            mine = cf.class_mask(row, [la]).to(DEV)
            if not (cfg & cf.BIT_NCHW):
                assert torch.equal(out[:, ~mine].view(torch.int32), before[:, ~mine].view(torch.int32)), "pixels of another class changed"
        G.check(row["name"])
        got = out.view(N, Nc, Ho, Wo).permute(0, 2, 3, 1) if cfg & cf.BIT_NCHW else out
        res.update(out=got.cpu(), amax=word(amax))
    elif e == "planes":
        la, = las
        ns = N if row.get("per_image") else 1
        h = G.new((N, Ho * Wo // 16, Nc, 16), torch.float16, float("nan"))
        l = G.new((N, Ho * Wo // 16, Nc, 16), torch.float16, float("nan"))
        sexp = G.new((ns,), torch.int32)
        in_amax = xs.amax if (xs.amax is not None and xs.amax.numel() == ns) else None
        K._rc(K.lib.lk_conv_nhwc_f16x2_planes(P(xs.planes[0]), P(xs.planes[1]), P(xs.sexp), ns, P(in_amax), N, Hi, Wi, row["Kc"], P(wp[0]),
                                              P(wp[1]), P(ws), P(l1), Nc, Ho, Wo, la["in_mul"], len(la["taps"]), flat3(la["taps"]), P(z),
                                              P(h), P(l), P(sexp), int(cfg), st), "lk_conv_nhwc_f16x2_planes")
        G.check(row["name"])
        unchunk = lambda t: t.permute(0, 2, 1, 3).reshape(N, Nc, Ho, Wo).permute(0, 2, 3, 1)  # noqa: E731
        res.update(o=planes_value(unchunk(h), unchunk(l), sexp), h=h.cpu(), sexp=sexp.cpu())
    elif e == "forward":
        la, = las
        y = G.new((N, Ho, Wo, Nc), torch.float32, float("nan"))
        mask = G.new((N, Ho, Wo, Nc), torch.uint8) if (row["act"] == 1 and row.get("mask", True)) else None
        h = l = None
        if row.get("planes", True):
            h, l = G.new((N, Ho, Wo, Nc), torch.float16, float("nan")), G.new((N, Ho, Wo, Nc), torch.float16, float("nan"))
        sexp, bound, amax = G.new((N,), torch.int32), G.new((N,), torch.float32, float("nan")), G.new((N,), torch.float32, 0.0)
        ab = prep.addend_bound
        K._rc(K.lib.lk_conv_bn_act_nhwc_f16x2(
            P(xs.planes[0]), P(xs.planes[1]), P(xs.sexp), xs.sexp.numel(), P(xs.amax), xs.amax.numel(), N, Hi, Wi, row["Kc"], P(wp[0]),
            P(wp[1]), P(ws), P(l1), Nc, Ho, Wo, la["in_mul"], len(la["taps"]), flat3(la["taps"]), P(z), P(prep.bn_scale), P(prep.bn_shift),
            P(prep.bn_scale_amax), P(prep.bn_shift_amax), P(prep.addend), P(ab), 1 if ab is None else ab.numel(), int(row["act"]), P(y),
            P(mask), P(h), P(l), P(sexp), P(bound), P(amax), int(cfg), st), "lk_conv_bn_act_nhwc_f16x2")
        G.check(row["name"])
        res.update(out=y.cpu(), sexp=sexp.cpu(), bound=bound.cpu(), amax=word(amax), mask=None if mask is None else mask.cpu())
        if h is not None:
            res.update(o=planes_value(h, l, sexp), h=h.cpu())
    else:
        la, = las
        h, l = G.new((N, Ho, Wo, Nc), torch.float16, float("nan")), G.new((N, Ho, Wo, Nc), torch.float16, float("nan"))
        sexp, amax = G.new((1,), torch.int32), G.new((1,), torch.float32, 0.0)
        add, mult = prep.add, prep.mult
        m_is_float = int(mult is not None and mult.dtype == torch.float32)
        mask_rows = 0 if mult is None else mult.shape[0] * Ho * Wo
        tail = (P(z), None if add is None else P(add.planes[0]), None if add is None else P(add.planes[1]), None if add is None else P(add.sexp),
                P(mult), m_is_float, P(prep.mult_amax), mask_rows, P(prep.scale), P(prep.scale_amax), P(h), P(l), P(sexp), P(amax), int(cfg), st)
        if e == "strided":
            src = []
            for i in range(2):
                if i < len(prep.src):
                    g_, wp_, ws_, l1_ = prep.src[i]
                    src += [P(g_.planes[0]), P(g_.planes[1]), P(g_.sexp), P(g_.amax), P(wp_[0]), P(wp_[1]), P(ws_), P(l1_)]
                else:
                    src += [None] * 8
            flat = (ctypes.c_int * (6 * len(la["taps"])))(*[int(v) for t in la["taps"] for v in t])
            K._rc(K.lib.lk_conv_nhwc_f16x2_vjp_strided(*src, N, Hi, Wi, row["Kc"], Nc, Ho, Wo, row["s"], len(la["taps"]), flat, *tail),
                  "lk_conv_nhwc_f16x2_vjp_strided")
        else:
            head = (P(xs.planes[0]), P(xs.planes[1]), P(xs.sexp), P(xs.amax), N, Hi, Wi, row["Kc"], P(wp[0]), P(wp[1]), P(ws), P(l1))
            geo = (Nc, Ho, Wo, len(la["taps"]), flat3(la["taps"]))
            if prep.wc is not None:
                K._rc(K.lib.lk_conv_nhwc_f16x2_vjp_wc(*head, P(prep.wc[0]), P(prep.wc[1]), *geo, *tail), "lk_conv_nhwc_f16x2_vjp_wc")
            else:
                K._rc(K.lib.lk_conv_nhwc_f16x2_vjp(*head, *geo, *tail), "lk_conv_nhwc_f16x2_vjp")
        G.check(row["name"])
        res.update(o=planes_value(h, l, sexp), h=h.cpu(), l=l.cpu(), sexp=sexp.cpu(), amax=word(amax))
    return res


def expected_sexp(bound):
    """the exponent the guaranteed bound gives, and the neighbour the device's fp32 evaluation may reach when the bound sits on
    a power of two to within fp32 rounding"""
    lg = math.log2(bound)
    s = {cf.sexp_of(bound)}
    if abs(lg - round(lg)) < 1e-5:
        s |= {cf.sexp_of(bound * (1 + 1e-4)), cf.sexp_of(bound * (1 - 1e-4))}
    return s


NAMES = [r["name"] for r in cf.ROWS]


@pytest.mark.parametrize("name", NAMES)
def test_row_is_within_its_tolerance_inside_its_buffers_and_reproducible(K, name):
    row = cf.resolve(cf.BY_NAME[name], K)
    las = cf.launches(row)
    for la in las:
        var = cf.variant(K, row, la)
        ex = {k: v for k, v in row["expect"].items() if k != "walk"}
        assert var is not None and {k: var[k] for k in ex} == ex, (name, var)
        if row["expect"].get("walk") or "split_S" in ex:
            assert var["grid"] + 1 <= var["n_tiles"] <= 1.5 * var["grid"], var
    o = cf.build(row)
    prep = Prepared(K, row, o)
    got = run(K, row, prep)
    e = row["entry"]
    key = f"{row['family']}-{e}"
    written = cf.class_mask(row, las)
    if "out" in got:
        r = cf.ratio(got["out"][:, written], o.want[:, written], o.tol[:, written])
        print(f"{name}: fp32 output error / tolerance = {r:.4f}")
        note(key, r, name)
        assert r <= 1.0, r
        if e == "plain":
            assert bool((got["out"][:, ~written] == UNWRITTEN).all())
            assert got["amax"].view(torch.int32).item() == got["out"][:, written].abs().max().view(torch.int32).item()  # from the stored values
    if "o" in got:
        tol = o.tol_planes if e == "forward" else o.tol
        r = cf.ratio(got["o"], o.want, tol)
        print(f"{name}: planes error / tolerance = {r:.4f}")
        note(key + "-planes" if e == "forward" else key, r, name)
        assert r <= 1.0, r
        assert got["h"].float().abs().max().item() < 2.0 ** 15
        bounds = o.bound_out.tolist() if torch.is_tensor(o.bound_out) else [o.bound_out]
        if e == "forward" or (e == "planes" and row.get("per_image")):
            assert len(bounds) == row["N"]
        for s, b in zip(got["sexp"].tolist(), bounds):
            assert s in expected_sexp(b), (s, b)
    if e in ("vjp", "strided"):
        top = got["o"].abs().max().item()
        assert abs(got["amax"].item() - top) <= 1e-5 * top
    if e == "forward":
        y = got["out"]
        tops = y.abs().amax(dim=(1, 2, 3))
        assert bool(((got["amax"] - tops).abs() <= 1e-5 * tops).all())
        assert bool(((got["bound"].double() - o.bound_out).abs() <= 1e-6 * o.bound_out).all())
        if got["mask"] is not None:
            assert torch.equal(got["mask"], (y > 0).to(torch.uint8))
    again = run(K, row, prep)
    for k_, v in got.items():
        if v is not None:
            assert torch.equal(torch.nan_to_num(v.double(), nan=-1.0), torch.nan_to_num(again[k_].double(), nan=-1.0)), f"second launch differs in {k_}"


def _pair_ratio(a, b, tol):
    return cf.ratio(a, b.double(), 2 * tol)


@pytest.mark.parametrize("entry", ["plain", "planes", "forward", "vjp"])
def test_the_five_tile_shapes_agree(K, entry):
    """same operands, same K order per element (taps major, chunks minor, one accumulator per element whatever the tile): the
    tile shapes are expected to agree to the bit"""
    row = cf.resolve(cf.BY_NAME[f"tile4-{entry}"], K)
    o = cf.build(row)
    prep = Prepared(K, row, o)
    runs = {t: run(K, row, prep, config=(row["config"] & ~(7 << 12)) | (t << 12)) for t in cf.TILES}
    auto = run(K, row, prep, config=row["config"] & ~(7 << 12))
    key = "out" if "out" in auto else "o"
    for t, r in runs.items():
        assert torch.equal(r[key], runs[4][key]), f"tile {t} differs from tile 4 in {key}"
        assert torch.equal(r["sexp"], runs[4]["sexp"]) if "sexp" in r else True
    assert any(torch.equal(auto[key], r[key]) for r in runs.values())


WINDOW_ROUTES = [r["name"] for r in cf.ROWS if r["family"] == "window" and r["name"].startswith("win") and not r["config"] & cf.BIT_SPLIT]


@pytest.mark.parametrize("name", WINDOW_ROUTES)
def test_window_form_against_the_generic_kernel(K, name):
    """bit 27 sends the same launch to the generic fused kernel (another order of the K steps): same scale, twice the tolerance"""
    row = cf.resolve(cf.BY_NAME[name], K)
    o = cf.build(row)
    prep = Prepared(K, row, o)
    win, gen = run(K, row, prep), run(K, row, prep, config=row["config"] | cf.BIT_NO_WIN)
    var = cf.variant(K, dict(row, config=row["config"] | cf.BIT_NO_WIN), cf.launches(row)[0])
    assert var["kernel"] == "generic"
    assert torch.equal(win["sexp"], gen["sexp"])
    r = _pair_ratio(win["o"], gen["o"], o.tol)
    note("route window-generic", r, name)
    assert r <= 1.0, r


@pytest.mark.parametrize("name", [r["name"] for r in cf.ROWS if r["config"] & cf.BIT_SPLIT])
def test_split_tail_against_the_ragged_last_round(K, name):
    row = cf.resolve(cf.BY_NAME[name], K)
    o = cf.build(row)
    prep = Prepared(K, row, o)
    split, whole = run(K, row, prep), run(K, row, prep, config=row["config"] & ~cf.BIT_SPLIT)
    assert cf.variant(K, dict(row, config=row["config"] & ~cf.BIT_SPLIT), cf.launches(row)[0])["split_S"] == 1
    assert torch.equal(split["sexp"], whole["sexp"])
    r = _pair_ratio(split["o"], whole["o"], o.tol)
    note("route split-unsplit", r, name)
    assert r <= 1.0, r


@pytest.mark.parametrize("name", [r["name"] for r in cf.ROWS if r["entry"] == "strided" and r["s"] == 2])
def test_strided_form_against_the_class_by_class_route(K, name):
    """one fused launch against a plain launch per residue class (and source) into an fp32 tensor followed by the element-wise VJP
    kernel: twice the tolerance"""
    row = cf.resolve(cf.BY_NAME[name], K)
    o = cf.build(row)
    prep = Prepared(K, row, o)
    fused = run(K, row, prep)
    N, H, W, Nc = row["N"], row["H"], row["W"], row["Nc"]
    dx = torch.zeros(N, H, W, Nc, device=DEV)
    amax = torch.zeros(1, device=DEV)
    for i, ((xs, wp, ws, _), (k, p)) in enumerate(zip(prep.src, ((row["k"], row["p"]), ((1, 1), (0, 0))))):
        for Hc, Wc, oh0, ow0, taps in cf._backward_plan(2, p, k, H, W):
            if taps:
                K.conv_nhwc_f16x2(xs, wp, ws, Hc, Wc, 1, dx, 2, oh0, ow0, taps, accumulate=i > 0, amax_out=amax, config=2)
    ref = K.vjp_nhwc_split(dx, K.absmax(dx), prep.add, prep.mult, prep.mult_amax, prep.scale, prep.scale_amax, o.S, (N, H, W, Nc))
    r = _pair_ratio(fused["o"], planes_value(ref.planes[0], ref.planes[1], ref.sexp), o.tol)
    note("route strided-classes", r, name)
    assert r <= 1.0, r
