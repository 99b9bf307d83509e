"""The dense last-layer, Jacobian, diagonal and element-wise kernels on the device (-m gpu): csrc/lk_ll.hip, csrc/lk_diag.hip
and csrc/lk_vjp.hip through the C ABI on every case of tests/dense_fixtures.py, against float64 evaluated from the same fp32
operands, inside the fixtures' per-element bounds (tests/test_dense_fixtures.py shows on the CPU that the tables reach every
launch form, that a plain fp32 evaluation sits inside the bounds and that the mutants and the subtracting GGN leave them).

Every output, and the workspace of ``lk_ll_ggn_full_f32``, lies between NaN guard bands; outputs that are not accumulated
onto start as NaN, so an element that is not written fails its bound; the inputs are compared with what was handed over;
each call is made twice and must return the same bits.  Then a small MLP whose forward pass is exact in fp32, through
``HipGGN(FeatureExtractor(model), "classification", last_layer=True).full``, against the fp64 oracle."""
import copy
import ctypes

import pytest
import torch

from tests import dense_fixtures as DF

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64
GUARD_BYTE = 0xA5
WORST = {}


@pytest.fixture(autouse=True, scope="module")
def _report():
    """the worst error / bound per kernel, printed when the module is done (pytest -s): what profiles/dense_instances.md records"""
    yield
    for key, (r, name) in sorted(WORST.items()):
        print(f"\n{key:18s} worst error / bound {r:.4f}  ({name})", end="")


def dev(t):
    return (t.float() if t.dtype == torch.float64 else t).to(DEV)


def _p(b):
    """the address of a banded buffer's payload (also where the payload is empty), or NULL"""
    return None if b is None else ctypes.c_void_p(b.ptr)


class _Banded:
    """``init`` (or a NaN / 0xA5 fill of ``shape``) inside guard bands of ``PAD`` elements, ``off`` elements past an aligned base"""

    def __init__(self, init=None, shape=None, dtype=torch.float32, off=0):
        if init is not None:
            shape, dtype = tuple(init.shape), (torch.uint8 if init.dtype == torch.bool else init.dtype)
        n = 1
        for d in shape:
            n *= d
        self.guard = float("nan") if dtype == torch.float32 else GUARD_BYTE
        self.buf = torch.full((2 * PAD + off + n,), self.guard, dtype=dtype, device=DEV)
        self.lo, self.hi = PAD + off, PAD + off + n
        self.t = self.buf[self.lo:self.hi].view(*shape)
        if init is not None:
            self.t.copy_(init.to(dtype))
        self.init = None if init is None else self.t.clone()
        self.ptr = self.buf.data_ptr() + self.lo * self.buf.element_size()
        assert self.buf.data_ptr() % 16 == 0 and self.ptr % 16 == (off * self.buf.element_size()) % 16

    def bands_intact(self):
        lo, hi = self.buf[:self.lo], self.buf[self.hi:]
        if self.guard != self.guard:
            return bool(lo.isnan().all()) and bool(hi.isnan().all())
        return bool((lo == self.guard).all()) and bool((hi == self.guard).all())

    def unchanged(self):
        a, b = self.t, self.init
        return bool(((a == b) | (a.isnan() & b.isnan())).all()) if a.is_floating_point() else torch.equal(a, b)


def _same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return bool(((a == b) | (a.isnan() & b.isnan())).all()) if a.is_floating_point() else torch.equal(a, b)


class AbiKernels:
    """the interface of ``dense_fixtures.Fp32Kernels`` on the HIP library's C entry points"""

    def __init__(self, hip):
        self.hip, self.lib = hip, hip.lib

    def _twice(self, run):
        """``run() -> (rc, inputs, outputs[, scratch])``: the checks every call gets, and a second call for the same bits"""
        res = []
        for _ in range(2):
            rc, ins, outs, *scratch = run()
            assert rc == 0, self.lib.lk_last_error()
            torch.cuda.synchronize()
            for b in ins:
                assert b is None or (b.unchanged() and b.bands_intact()), "an input changed"
            for b in list(outs) + list(scratch[0] if scratch else ()):
                assert b is None or b.bands_intact(), "written outside an output's extent"
            res.append([None if b is None else b.t for b in outs])
        for a, b in zip(*res):
            assert _same_bits(a, b), "two equal calls differ"
        return res[0]

    def _st(self):
        return self.hip._stream(torch.device(DEV))

    def ll_ggn_full(self, phi, probs, C, has_bias, alpha, H0):
        B, D = phi.shape
        need = int(self.lib.lk_ll_ggn_workspace_bytes(B, C, D))

        def run():
            ph, pr, H = _Banded(phi), (None if probs is None else _Banded(probs)), _Banded(H0)
            ws = _Banded(shape=((need + 3) // 4,))
            rc = self.lib.lk_ll_ggn_full_f32(_p(ph), _p(pr), B, C, D, int(has_bias), float(alpha),
                                             _p(H), _p(ws), need, self._st())
            return rc, (ph, pr), (H,), (ws,)

        return self._twice(run)[0]

    def dense_quadform_ll(self, phi, Sigma, C, has_bias):
        B, D = phi.shape

        def run():
            ph, Sg, fv = _Banded(phi), _Banded(Sigma), _Banded(shape=(B, C, C))
            rc = self.lib.lk_dense_quadform_ll_f32(_p(ph), _p(Sg), B, C, D, int(has_bias), _p(fv), None, 0, self._st())
            return rc, (ph, Sg), (fv,)

        return self._twice(run)[0]

    def jac_last_layer(self, phi, C, has_bias):
        B, D = phi.shape
        P = C * D + (C if has_bias else 0)

        def run():
            ph, Js = _Banded(phi), _Banded(shape=(B, C, P))
            return self.lib.lk_jac_last_layer_f32(_p(ph), B, C, D, int(has_bias), _p(Js), self._st()), (ph,), (Js,)

        return self._twice(run)[0]

    def diag_ggn_linear(self, a, g, alpha, hw0, hb0):
        Cc, B, Do = g.shape
        Di = a.shape[1]

        def run():
            a_, g_, hw, hb = _Banded(a), _Banded(g), _Banded(hw0), (None if hb0 is None else _Banded(hb0))
            rc = self.lib.lk_diag_ggn_linear_f32(_p(a_), _p(g_), B, Cc, Di, Do, float(alpha), _p(hw),
                                                 _p(hb), self._st())
            return rc, (a_, g_), (hw, hb)

        return tuple(self._twice(run))

    def jac_linear(self, a, g, Js0, col0, bcol0):
        Cc, B, Do = g.shape

        def run():
            a_, g_, Js = _Banded(a), _Banded(g), _Banded(Js0)
            rc = self.lib.lk_jac_linear_f32(_p(a_), _p(g_), B, Cc, a.shape[1], Do, _p(Js), Js0.shape[-1], col0, bcol0,
                                            self._st())
            return rc, (a_, g_), (Js,)

        return self._twice(run)[0]

    def jac_conv(self, x, g, c, Js0, col0, bcol0):
        Cc, B, Do = g.shape[:3]

        def run():
            x_, g_, Js = _Banded(x), _Banded(g), _Banded(Js0)
            rc = self.lib.lk_jac_conv_f32(_p(x_), _p(g_), B, Cc, c["Cin"], c["H"], c["W"], Do, *c["k"], *c["s"], *c["p"],
                                          *c["d"], _p(Js), Js0.shape[-1], col0, bcol0, self._st())
            return rc, (x_, g_), (Js,)

        return self._twice(run)[0]

    def sq_colsum(self, Js, rows, P, col0, width, alpha, h0):
        def run():
            J, h = _Banded(Js), _Banded(h0)
            return self.lib.lk_sq_colsum_f32(_p(J), rows, P, col0, width, float(alpha), _p(h), self._st()), (J,), (h,)

        return self._twice(run)[0]

    def vjp_scale_mask(self, g, g2, m, scale, S, per, C, HW, mis=None):
        def run():
            g_ = _Banded(g, off=int(mis == "g"))
            h_ = None if g2 is None else _Banded(g2, off=int(mis == "g2"))
            m_ = None if m is None else _Banded(m, off=int(mis == "m"))
            s_ = None if scale is None else _Banded(scale)
            out = _Banded(shape=(S, per), off=int(mis == "out"))
            rc = self.lib.lk_vjp_scale_mask_f32(_p(g_), _p(h_), _p(m_),
                                                int(m is not None and m.dtype == torch.float32),
                                                _p(s_), S, per, C, HW, _p(out), self._st())
            return rc, (g_, h_, m_, s_), (out,)

        return self._twice(run)[0]

    def bn_act_forward(self, x, scale, shift, addend, C, HW, relu, want_mask, mis=None):
        def run():
            x_, sc, sh = _Banded(x, off=int(mis == "x")), _Banded(scale), _Banded(shift)
            ad = None if addend is None else _Banded(addend, off=int(mis == "addend"))
            y = _Banded(shape=tuple(x.shape), off=int(mis == "y"))
            mk = _Banded(shape=tuple(x.shape), dtype=torch.uint8, off=int(mis == "mask")) if relu and want_mask else None
            rc = self.lib.lk_bn_act_fwd_f32(_p(x_), _p(sc), _p(sh), _p(ad), x.numel(), C, HW,
                                            int(relu), _p(y), _p(mk), self._st())
            return rc, (x_, sc, sh, ad), (y, mk)

        return tuple(self._twice(run))


@pytest.fixture(scope="module")
def K():
    from laplace_amd._lib import get_kernels

    return AbiKernels(get_kernels())


def _hold(kernel, res):
    for name, r in res.items():
        print(f"{kernel} {name}: {r:.4f}")
        if r != r or r > WORST.get(kernel, (-1.0, ""))[0]:
            WORST[kernel] = (r, name)
    bad = {n: r for n, r in res.items() if not DF.ok(r)}
    assert not bad, f"{kernel}: error / bound {bad}"


@pytest.mark.parametrize("c", DF.LL_CASES, ids=DF.ll_id)
def test_ll_ggn_full(K, c):
    """element bound, smallest eigenvalue >= -||bound||_F, no negative diagonal entry"""
    res = DF.check_ll_ggn(K, dev, [c])
    el, eig, neg = DF.LL_FIGURES[DF.ll_id(c)]
    print(f"ll_ggn_full {DF.ll_id(c)}: element {el:.4g} eigenvalue {eig:.4g} negative diagonal entries {neg}")
    for key, v in (("ll_ggn_full", el), ("ll_ggn_full eig", eig)):
        if v != v or v > WORST.get(key, (-1.0, ""))[0]:
            WORST[key] = (v, DF.ll_id(c))
    assert DF.ok(el), f"element error is {el:.4g} of its bound"
    assert DF.ok(eig), f"-lambda_min is {eig:.4g} of ||bound||_F"
    assert neg == 0 and DF.ok(res[DF.ll_id(c)])


@pytest.mark.parametrize("c", DF.QF_CASES, ids=DF.qf_id)
def test_dense_quadform_ll(K, c):
    _hold("dense_quadform_ll", DF.check_quadform(K, dev, [c]))


@pytest.mark.parametrize("check,kernel", [("check_jac_last_layer", "jac_last_layer"), ("check_diag_linear", "diag_ggn_linear"),
                                          ("check_jac_linear", "jac_linear"), ("check_jac_conv", "jac_conv"),
                                          ("check_sq_colsum", "sq_colsum"), ("check_vjp", "vjp_scale_mask"),
                                          ("check_bn_act", "bn_act_forward")])
def test_table(K, check, kernel):
    _hold(kernel, getattr(DF, check)(K, dev))


@pytest.mark.parametrize("kind", list(DF.MODEL_SCALES))
def test_last_layer_full_of_a_model(kind):
    """two minibatches of a model with a logit margin of about 15 (and of 1): the returned H against the oracle's inside the
    element bound summed over the batches, and log det (H + 1e-4 I) against the oracle's to 1e-4"""
    from laplace_amd import HipGGN
    from laplace_amd.mirror import FeatureExtractor

    m64, X, _ = DF.exact_mlp(kind)
    b = HipGGN(FeatureExtractor(copy.deepcopy(m64).float()).to(DEV), "classification", last_layer=True)
    with torch.no_grad():
        f64 = m64(X)
        f32 = copy.deepcopy(m64).float().to(DEV)(X.float().to(DEV))
    assert torch.equal(f32.double().cpu(), f64), "the forward pass is exact in fp32"
    top = f64.topk(2, 1).values
    margin = top[:, 0] - top[:, 1]
    assert (10 <= margin.min() and margin.max() <= 20) if kind == "saturated" else margin.max() < 2
    r, lam, nb, neg, ld, ld_want = DF.model_figures(kind, lambda Xs, ys, phi, f: b.full(Xs.float().to(DEV), ys.to(DEV))[1])
    print(f"model {kind}: element error / bound {r:.4f}, lambda_min {lam:.3e} (-||bound||_F {-nb:.3e}), logdet {ld:.6f} "
          f"against {ld_want:.6f}")
    WORST[f"model {kind}"] = (r, "two minibatches of 8")
    assert DF.ok(r), f"element error is {r:.4g} of its bound"
    assert lam >= -nb and neg == 0
    assert abs(ld - ld_want) <= 1e-4 * abs(ld_want)
