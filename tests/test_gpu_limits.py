"""The LAST ACCEPTED value of the shape limits of the C ABI, run on the device and compared with fp64 (-m gpu).

tests/test_capi_contracts.py holds the table of limits and checks, without a device, that every guard refuses the first
value past its limit.  This file runs the real kernels AT the limits, through the `HipKernels` wrappers: a grid
dimension of 65535, the raised dynamic-LDS limit of the LDS-staged quadratic forms, the 65535-image seams of the Python
wrappers, the widest cotangent the persistent window convolution takes.  The other extents of every case are kept
minimal: what is tested is the index arithmetic at the edge.

Tolerances are the ones the existing test of the same entry point asserts (1e-5 of the largest element for the
convolutions, 4e-6 between two device routes of one sum, 2e-6 for the split Gram, 1e-6 for the fp32 GEMM and the pure
data movers, the 1e-4 default of test_gpu_kernels.py elsewhere); every comparison is recorded (tests/parity_log.py).

Last-accepted cases that are NOT run here (the guard itself is covered by tests/test_capi_contracts.py):

| limit                                                        | reason                                                       |
|--------------------------------------------------------------|--------------------------------------------------------------|
| lk_syevj_f32 / lk_syevj_batched_f32, n = 32768               | 4 GiB matrix, 16 GiB workspace, an fp64 eigh of hours        |
| lk_pack_upper_f32 / lk_unpack_upper_f32, n = 65535           | 17 GiB matrix                                                |
| lk_ll_ggn_full_f32, C (D + 1) = 2^20 - 1                     | a 4 TiB dense GGN                                            |
| grid.x < 2^31 workgroups (lk_bn_act_fwd_f32, lk_vjp_*, ...)  | > 2^39 elements                                              |
| the 2^31-row / 2^40-element bounds of the convolutions       | > 8 GiB of operands                                          |
| the 2^29 / 2^31 element products of the shared quadratic     | > 8 GiB of operands (or an fp64 reference of many minutes)   |
|   forms, lk_diag_ggn_shared_f32, lk_quadform_shared_grid_f32 |                                                              |
| lk_gram_conv_nhwc_f32 / lk_conv3x3_shiftcorr_f32, 2^31 rows  | > 8 GiB of operands                                          |
| lk_conv3x3_pixpair_*: 524288 blocks (203 x 200 x 64 map)     | 8 GiB of blocks, fp64 reference of minutes                   |
| plain convolution with T = 9, planes output at Ho Wo = 16    | already run: every 3 x 3 case of tests/test_gpu_conv.py;     |
|                                                              | lk_conv_nhwc_f16x2_planes on 4 x 4 maps (L = 16) by the      |
|                                                              | 512-512 case of tests/test_gpu_quad_planes.py                |
"""
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu
# LK_TEST_DEVICE=cpu runs the test bodies on the fp64 kernel emulation (a self-check of this file's references on a
# machine without a device; cases that need the library itself are then not meaningful and skip)
DEV = os.environ.get("LK_TEST_DEVICE", "cuda")
ON_DEVICE = DEV != "cpu"
needs_library = pytest.mark.skipif(not ON_DEVICE, reason="a limit of the HIP library, not of the emulation")


@pytest.fixture(autouse=True)
def _kernels():
    if ON_DEVICE:
        yield
        return
    from laplace_amd import _lib
    from tests.emulated_kernels import EmulatedKernels

    prev = _lib.set_kernels_for_testing(EmulatedKernels())
    yield
    _lib.set_kernels_for_testing(prev)


def K():
    from laplace_amd._lib import get_kernels

    return get_kernels()


def rel(got, want, tag=None):
    """max|got - want| / max|want|, recorded"""
    from tests.parity_log import record_error

    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return record_error((got - want).abs().max().item() / (want.abs().max().item() + 1e-300), tag)


def relel(got, want):
    """elementwise relative error of positive sums (as tests/test_gpu_prior_grid.py), recorded"""
    from tests.parity_log import record_error

    got, want = got.double().cpu(), want.double().cpu()
    return record_error(((got - want).abs() / want.abs().clamp_min(1e-30)).max().item())


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def f32(t):
    return None if t is None else t.float().to(DEV).contiguous()


# ---- 16-bit grid dimensions --------------------------------------------------------------------------------------------------
def test_jac_linear_with_65535_sample_class_rows():
    """grid.y = B * Cc = 65535 (13107 samples x 5 outputs): the last row is (n, c) = (13106, 4)"""
    B, Cc, Di, Do = 13107, 5, 3, 2
    a, g = rnd(B, Di, seed=1), rnd(Cc, B, Do, seed=2)
    P = 1 + Do * Di + Do + 2
    gJ = torch.full((B, Cc, P), 7.0, device=DEV)
    K().jac_linear(f32(a), f32(g), gJ, 1, 1 + Do * Di)
    want = torch.full((B, Cc, P), 7.0, dtype=torch.float64)
    want[:, :, 1:1 + Do * Di] = torch.einsum("cno,ni->ncoi", g, a).reshape(B, Cc, Do * Di)
    want[:, :, 1 + Do * Di:1 + Do * Di + Do] = g.permute(1, 0, 2)
    assert rel(gJ, want) < 1e-6
    assert rel(gJ[-1, -1], want[-1, -1]) < 1e-6  # the row of the last workgroup


def test_jac_conv_with_65535_sample_class_slices():
    """grid.z = B * Cc = 65535"""
    B, Cc, Cin, H, Do, k = 13107, 5, 1, 3, 2, 3
    x, g = rnd(B, Cin, H, H, seed=3), rnd(Cc, B, Do, H, H, seed=4)
    Dk = Cin * k * k
    P = Do * Dk + Do
    gJ = torch.zeros(B, Cc, P, device=DEV)
    K().jac_conv(f32(x), f32(g), (k, k), 1, 1, 1, gJ, 0, Do * Dk)
    patches = F.unfold(x, k, padding=1)  # [B, Dk, L]
    want = torch.zeros(B, Cc, P, dtype=torch.float64)
    want[:, :, :Do * Dk] = torch.einsum("cnol,nkl->ncok", g.reshape(Cc, B, Do, H * H), patches).reshape(B, Cc, Do * Dk)
    want[:, :, Do * Dk:] = g.sum((3, 4)).permute(1, 0, 2)
    assert rel(gJ, want) < 1e-5
    assert rel(gJ[-1, -1], want[-1, -1]) < 1e-5


def test_jac_conv_with_65535_output_tiles():
    """grid.y = ceil(Do / 16) = 65535 (a 1 x 1 convolution of one channel on a 2 x 1 map)"""
    B, Cc, Do = 2, 2, 65535 * 16
    x, g = rnd(B, 1, 2, 1, seed=3), rnd(Cc, B, Do, 2, 1, seed=4)
    gJ = torch.zeros(B, Cc, 2 * Do, device=DEV)
    K().jac_conv(f32(x), f32(g), (1, 1), 1, 0, 1, gJ, 0, Do)
    want = torch.cat([torch.einsum("cnol,nl->nco", g.reshape(Cc, B, Do, 2), x.reshape(B, 2)), g.sum((3, 4)).permute(1, 0, 2)], 2)
    assert rel(gJ, want) < 1e-5
    assert rel(gJ[:, :, Do - 16:Do], want[:, :, Do - 16:Do]) < 1e-5  # the last tile of outputs


def test_nchw_to_nhwc_with_65535_images_and_65535_channel_tiles():
    """grid.z = B = 65535; grid.y = ceil(C / 64) = 65535"""
    x = rnd(65535, 3, 2, 2, seed=5).float().to(DEV)
    got = K().nchw_to_nhwc(x)
    assert torch.equal(got, x.permute(0, 2, 3, 1).contiguous())
    x = torch.randn(1, 65535 * 64, 2, 1, generator=torch.Generator().manual_seed(5)).to(DEV)
    assert torch.equal(K().nchw_to_nhwc(x), x.permute(0, 2, 3, 1).contiguous())


def test_unsplit_transpose_with_65535_images_and_a_wide_map():
    """grid.z = S * B = 65535; separately grid.y = ceil(L / 32) = 65535, the most positions the guard accepts"""
    S, B, H, W, C = 5, 13107, 2, 1, 8
    x = torch.randn(S * B, H, W, C, generator=torch.Generator().manual_seed(6)).to(DEV)
    u = K().unsplit_transpose(K().split_f16x2(x), S, B)
    want = x.reshape(S, B, H * W, C).permute(1, 0, 3, 2)
    assert u.shape == (B, S, C, H * W) and rel(u, want) < 1e-6
    S, B, H, W, C = 1, 1, 65535 * 32, 1, 8
    x = torch.randn(S * B, H, W, C, generator=torch.Generator().manual_seed(7)).to(DEV)
    u = K().unsplit_transpose(K().split_f16x2(x), S, B)
    want = x.reshape(S, B, H * W, C).permute(1, 0, 3, 2)
    assert rel(u, want) < 1e-6
    assert rel(u[..., -32:], want[..., -32:]) < 1e-6  # the last tile of positions


def test_diag_quadform_js_with_65535_samples():
    """grid = (C, C, B) with B = 65535"""
    B, C, P = 65535, 2, 5
    Js, var = rnd(B, C, P, seed=8), rnd(P, seed=9).abs()
    got = K().diag_quadform_js(f32(Js), f32(var))
    want = torch.einsum("ncp,p,nkp->nck", Js, var, Js)
    assert rel(got, want) < 1e-4
    assert rel(got[-1], want[-1]) < 1e-4


def test_dense_quadform_ll_with_361_classes():
    """grid.y = C (C + 1) / 2 = 65341 class pairs (362 classes are refused)"""
    B, C, D = 3, 361, 2
    phi = rnd(B, D, seed=10)
    P = C * D + C
    A = rnd(P, P, seed=11) / P ** 0.5
    Sigma = A @ A.T + torch.eye(P, dtype=torch.float64)
    got = K().dense_quadform_ll(f32(phi), f32(Sigma), C, True)
    J = torch.zeros(B, C, P, dtype=torch.float64)  # J_n = I_C (x) [phi_n, 1] in the order weight [C][D], bias [C]
    for c in range(C):
        J[:, c, c * D:(c + 1) * D] = phi
        J[:, c, C * D + c] = 1.0
    want = torch.einsum("ncp,pq,nkq->nck", J, Sigma, J)
    assert got.shape == (B, C, C)
    assert rel(got, want) < 1e-4
    assert rel(got[:, -1, -1], want[:, -1, -1]) < 1e-4  # the last pair


def test_diag_ggn_linear_with_65535_output_tiles():
    """grid.y = ceil(Do / 16) = 65535"""
    B, Cc, Di, Do = 3, 2, 1, 65535 * 16
    a, g = rnd(B, Di, seed=12), rnd(Cc, B, Do, seed=13)
    ghw, ghb = torch.zeros(Do * Di, device=DEV), torch.zeros(Do, device=DEV)
    K().diag_ggn_linear(f32(a), f32(g), 0.7, ghw, ghb)
    gsq = (g ** 2).sum(0)  # [B, Do]
    assert rel(ghw, 0.7 * torch.einsum("no,ni->oi", gsq, a ** 2).reshape(-1)) < 1e-4
    assert rel(ghb, 0.7 * gsq.sum(0)) < 1e-4
    assert rel(ghb[-16:], 0.7 * gsq.sum(0)[-16:]) < 1e-4


@needs_library
def test_gemm_with_65535_row_tiles():
    """grid.y = ceil(M / 64) = 65535"""
    M, N, Kd = 65535 * 64, 3, 2
    g = torch.Generator().manual_seed(14)
    A, B = torch.randn(1, M, Kd, generator=g).to(DEV), torch.randn(1, Kd, N, generator=g).to(DEV)
    C = torch.full((1, M, N), 7.0, device=DEV)
    K().gemm(A, B, C, 1, M, N, Kd, Kd, N, N, sa=M * Kd, sb=0, sc=M * N, alpha=0.5)
    want = 0.5 * A.double() @ B.double()
    assert rel(C, want) < 1e-6
    assert rel(C[0, -64:], want[0, -64:]) < 1e-6


# ---- the split Gram's three families -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,R", [(4096, 77), (64, 77), (128, 77), (4096, 300)])
def test_gram_of_a_split_tensor_at_its_widths(C, R):
    """C = 64, 128 and the widest accepted 4096 (528 tile pairs in grid.x), ragged row counts"""
    from laplace_amd._lib import SplitTensor

    torch.manual_seed(C + R)
    X = torch.randn(R, C, device=DEV) * torch.exp(torch.randn(R, 1, device=DEV))
    pad = (-R) % 8
    xs = K().split_f16x2(torch.cat([X, torch.zeros(pad, C, device=DEV)]).contiguous())
    xs.planes = xs.planes[:, :R]
    G0 = torch.randn(C, C, device=DEV)
    G = G0.clone()
    K().gram_tn_f16x2(SplitTensor(xs.planes.contiguous(), xs.sexp), 0.5, G)
    want = G0.double() + 0.5 * (X.double().T @ X.double())
    idx = torch.arange(C, device=DEV) // 32
    upper = idx[:, None] <= idx[None, :]
    assert rel(torch.where(upper, G.double(), want), want) < 2e-6
    assert torch.equal(G[~upper], G0[~upper])


# ---- likelihood roots at the switch-over -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2000, 2001])
def test_softmax_roots_at_the_cholesky_limit(C):
    """C = 2000: the Cholesky root at LK_SOFTMAX_CHOL_MAX_C (64016 bytes of dynamic LDS); C = 2001: the wrapper's
    switch-over to the symmetric root"""
    from tests.emulated_kernels import EmulatedKernels

    B = 3
    f = rnd(B, C, seed=C) * 2
    y = torch.randint(C, (B,), generator=torch.Generator().manual_seed(1))
    la = torch.zeros(1, dtype=torch.float64)
    chol = C <= getattr(K(), "softmax_chol_max_c", C)  # (the emulation has no such limit)
    assert chol == (C <= 2000) or not ON_DEVICE
    want = EmulatedKernels().softmax_hess_sqrt(f, y, la, cholesky=chol)
    lg = torch.zeros(1, device=DEV)
    got = K().softmax_hess_sqrt(f32(f), y.to(DEV), lg, cholesky=True)
    assert got.shape == ((C - 1) if chol else C, B, C)
    assert rel(got, want) < 1e-5
    assert rel(lg, la) < 1e-5
    S = got.permute(1, 2, 0).double().cpu()
    p = torch.softmax(f, -1)
    assert rel(S @ S.transpose(1, 2), torch.diag_embed(p) - p.unsqueeze(2) * p.unsqueeze(1)) < 1e-5


# ---- the class tile's cap ----------------------------------------------------------------------------------------------------------
def test_ten_outputs_and_ten_seeds():
    """C = 10 outputs of the shared quadratic form, S = 10 seeds of the shared GGN diagonal (11 are refused)"""
    B, C, Do, Dk, L = 2, 10, 5, 7, 3
    u, v = rnd(B, C, Do, L, seed=1), rnd(B, Dk, L, seed=2)
    l1, l2 = rnd(Do, seed=3).abs(), rnd(Dk, seed=4).abs()
    d = torch.tensor([0.3], dtype=torch.float64)
    got = K().kron_quadform_shared(f32(u), f32(v), f32(l1), f32(l2), f32(d), torch.zeros(B, C, C, device=DEV))
    J = torch.einsum("ncol,nil->ncoi", u, v)
    want = torch.einsum("ncoi,nkoi,oi->nck", J, J, 1.0 / (torch.outer(l1, l2) + d))
    assert rel(got, want) < 1e-4
    got = K().diag_ggn_shared(f32(u), f32(v), 0.7, torch.zeros(Do * Dk, device=DEV))
    assert rel(got, 0.7 * (J ** 2).sum((0, 1)).reshape(-1)) < 1e-4


# ---- the raised dynamic-LDS limit of the LDS-staged quadratic forms ---------------------------------------------------------------
def _kron_rowsums(v2, l1, l2, d):
    """T[n][o] = sum_i v2[n][i] / (l1[o] l2[i] + d), in slices of the outputs (the table is Do x Di)"""
    out = torch.empty(v2.shape[0], l1.numel(), dtype=torch.float64)
    for o0 in range(0, l1.numel(), 256):
        out[:, o0:o0 + 256] = v2 @ (1.0 / (torch.outer(l1[o0:o0 + 256], l2) + d)).T
    return out


# (Do, Di): Di + 2 Do floats of LDS = 64 KiB - 4 B, 64 KiB + 4 B (first use of the raised limit), 150 KiB exactly (the last
# accepted width), and a Linear(25088, 4096) head (133 KiB)
LDS_WIDTHS = [(100, 16183), (100, 16185), (200, 38000), (4096, 25088)]


@pytest.mark.parametrize("Do,Di", LDS_WIDTHS, ids=[f"{4 * (w[1] + 2 * w[0])}B" for w in LDS_WIDTHS])
@pytest.mark.parametrize("bias", [True, False])
def test_linear_quadratic_forms_across_the_64KiB_line(Do, Di, bias):
    """Sums of 16183 .. 38000 terms (the widest tested before: 512), asserted at the entry points' existing bound of
    1e-4.  Measured on the MI355X: see profiles/limits_parity.md."""
    B, C = 3, 2
    u, v = rnd(C, B, Do, seed=1), rnd(B, Di, seed=2)
    l1, l2, lb = rnd(Do, seed=3).abs(), rnd(Di, seed=4).abs(), rnd(Do, seed=5).abs()
    d = torch.tensor([0.5], dtype=torch.float64)
    ub = u * 0.5
    T = _kron_rowsums(v ** 2, l1, l2, d)
    want = torch.einsum("cno,kno,no->nck", u, u, T)
    if bias:
        want = want + torch.einsum("cno,kno,o->nck", ub, ub, 1.0 / (lb + d))
    got = K().kron_quadform_linear(f32(u), f32(v), f32(l1), f32(l2), f32(d), torch.zeros(B, C, C, device=DEV),
                                   f32(ub) if bias else None, f32(lb) if bias else None, f32(d) if bias else None)
    assert rel(got, want) < 1e-4
    vw, vb = rnd(Do, Di, seed=6).abs(), rnd(Do, seed=7).abs()
    want = torch.einsum("cno,kno,no->nck", u, u, (v ** 2) @ vw.T)
    if bias:
        want = want + torch.einsum("cno,kno,o->nck", u, u, vb)
    got = K().diag_quadform_linear(f32(v), f32(u), f32(vw.reshape(-1)), f32(vb) if bias else None, torch.zeros(B, C, C, device=DEV))
    assert rel(got, want) < 1e-4


@pytest.mark.parametrize("mode", ["kron", "diag"])
def test_linear_quadratic_form_keeps_a_bias_block_of_small_terms(mode):
    """4096 outputs whose weight terms sum to 2^18 exactly and whose 4096 bias terms are 0.015 each: every one of them is
    below half an ulp of the running sum (2^-6), so a single fp32 accumulator that runs through the weight block and then
    the bias block drops all of them (2.3e-4 of the result, past the 1e-4 contract); the bias block has its own accumulator.
    Bound: the 1e-4 of the entry point's existing test."""
    B, C, Do, Di, b = 2, 1, 4096, 64, 0.015
    ones = lambda *s: torch.ones(*s, device=DEV)  # noqa: E731
    u, v = ones(C, B, Do), ones(B, Di)
    want = torch.full((B, C, C), Do * Di + Do * b, dtype=torch.float64)
    if mode == "kron":  # W(o, i) = 1 / (1 * 1 + 0) = 1, bias weight 1 / (lb + 0) = b
        zero = torch.zeros(1, device=DEV)
        got = K().kron_quadform_linear(u, v, ones(Do), ones(Di), zero, torch.zeros(B, C, C, device=DEV), u, ones(Do) / b, zero)
    else:
        got = K().diag_quadform_linear(v, u, ones(Do * Di), ones(Do) * b, torch.zeros(B, C, C, device=DEV))
    assert rel(got, want) < 1e-4
    if ON_DEVICE:
        var = torch.zeros(2, B, C, device=DEV)
        deltas = torch.zeros(2, device=DEV)
        if mode == "kron":
            K().quadform_linear_grid(u, v, ones(Do), ones(Di), deltas, 0, var, u, ones(Do) / b)
        else:  # 1 / (h + 0) with h = 1
            K().quadform_linear_grid(u, v, ones(Do * Di), None, deltas, 2, var, u, ones(Do) / b)
        assert rel(var, want.reshape(1, B, C).expand(2, B, C)) < 1e-4


def _grid_weights64(w0, w1, d, mode, Do, Di):
    d = d.double().reshape(-1, 1, 1)
    if mode == 0:
        return 1.0 / (torch.outer(w0.double(), w1.double())[None] + d)
    if mode == 1:
        sd = d.sqrt()
        return 1.0 / ((w0.double()[None, :, None] + sd) * (w1.double()[None, None, :] + sd))
    return 1.0 / (w0.double().reshape(1, Do, Di) + d)


# the grid kernel stages 4 samples per workgroup: 4 (Di + GS Do) floats, GS grid points per LDS chunk.  With Do = 100:
# Di = 3896 is the widest layer that still gets GS = 2 inside 64 KiB, 3897 the first with GS = 1, 3997 the first whose single
# chunk is past 64 KiB (the raised limit), 9500 the last accepted width (150 KiB)
GRID_WIDTHS = [(3896, 2), (3897, 1), (3997, 1), (9500, 1)]


@needs_library
@pytest.mark.parametrize("Di,GS", GRID_WIDTHS, ids=[f"Di{w[0]}-GS{w[1]}" for w in GRID_WIDTHS])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_linear_grid_kernel_at_its_lds_chunking_edges(Di, GS, mode):
    """G = GS (one chunk), GS + 1 and a G that leaves a ragged last chunk; against the per-point fp64 loop"""
    gen = torch.Generator().manual_seed(Di + mode)
    B, C, Do = 5, 2, 100
    u, v = torch.randn(C, B, Do, generator=gen), torch.randn(B, Di, generator=gen)
    ub, wb = torch.randn(C, B, Do, generator=gen), torch.rand(Do, generator=gen) + 0.1
    if mode == 2:
        w0, w1 = torch.rand(Do, Di, generator=gen) * 3, None
    else:
        w0, w1 = torch.rand(Do, generator=gen) * 2 + 0.01, torch.rand(Di, generator=gen) * 2 + 0.01
    dev = lambda t: None if t is None else t.to(DEV).contiguous()  # noqa: E731
    for G in (GS, GS + 1, 2 * GS + 1 if GS > 1 else 3):
        deltas = torch.logspace(-3, 3, G)
        var = torch.zeros(G, B, C, device=DEV)
        K().quadform_linear_grid(dev(u), dev(v), dev(w0.reshape(-1) if mode == 2 else w0), dev(w1), dev(deltas), mode, var,
                                 dev(ub), dev(wb))
        want = torch.empty(G, B, C, dtype=torch.float64)
        for gi in range(G):  # the per-point loop
            W = _grid_weights64(w0, w1, deltas[gi:gi + 1], mode, Do, Di)[0]
            want[gi] = torch.einsum("cno,no->nc", u.double() ** 2, (v.double() ** 2) @ W.T)
            want[gi] += torch.einsum("cno,o->nc", ub.double() ** 2, 1.0 / (wb.double() + deltas[gi].double()))
        assert relel(var, want) < 1e-5, (G, mode)


# ---- the 65535-image seams of the Python wrappers -----------------------------------------------------------------------------
SEAM = 65535  # HipKernels.MAX_IMAGES_PER_LAUNCH


@pytest.mark.parametrize("N", [SEAM, SEAM + 1, SEAM + 9])
def test_split_images_across_the_launch_seam(N):
    """one launch, two launches, a ragged second launch; images on both sides of the seam equal a run of those images
    alone, bit for bit"""
    from laplace_amd._lib import HipKernels

    assert HipKernels.MAX_IMAGES_PER_LAUNCH == SEAM
    g = torch.Generator().manual_seed(N)
    x = (torch.randn(N, 1, 1, 8, generator=g) * 10.0 ** (torch.rand(N, 1, 1, 1, generator=g) * 12 - 8)).to(DEV).contiguous()
    st = K().split_images_f16x2(x)
    assert st.sexp.numel() == N and st.amax.numel() == N
    assert torch.equal(st.amax.cpu(), x.abs().reshape(N, -1).amax(1).cpu())
    a, b = st.float().double().cpu().flatten(1), x.double().cpu().flatten(1)
    from tests.parity_log import record_error

    assert record_error(((a - b).abs().amax(1) / b.abs().amax(1)).max().item()) < 2.0 ** -21  # image by image
    lo = SEAM - 6
    alone = K().split_images_f16x2(x[lo:].contiguous())
    assert torch.equal(alone.planes, st.planes[:, lo:]) and torch.equal(alone.sexp, st.sexp[lo:])
    assert torch.equal(alone.amax, st.amax[lo:])


@pytest.mark.parametrize("N", [SEAM, SEAM + 1, SEAM + 9])
@pytest.mark.parametrize("with_addend", [False, True])
def test_bn_act_forward_nhwc_across_the_launch_seam(N, with_addend):
    C = 8
    g = torch.Generator().manual_seed(N + 1)
    sc = 10.0 ** (torch.rand(N, 1, 1, 1, generator=g) * 10 - 5)
    x = (torch.randn(N, 1, 1, C, generator=g).abs() * sc).to(DEV).contiguous()
    addend = (torch.randn(N, 1, 1, C, generator=g).abs() * sc).to(DEV).contiguous() if with_addend else None
    scale = (torch.rand(C, generator=g) + 0.5).to(DEV)
    shift = torch.zeros(C, device=DEV)

    def run(xx, aa):
        n = xx.shape[0]
        in_amax = (xx.abs().reshape(n, -1).amax(1) / 48.0).contiguous()
        a_bound = aa.abs().reshape(n, -1).amax(1).contiguous() if aa is not None else None
        return K().bn_act_forward_nhwc(xx, in_amax, scale, shift, K().absmax(scale), K().absmax(shift), 1, addend=aa,
                                       addend_bound=a_bound, x_mul=torch.tensor([64.0], device=DEV),
                                       x_add=torch.tensor([0.0], device=DEV))

    y, mask, split, bound = run(x, addend)
    want = x.double() * scale.double()
    if with_addend:
        want = want + addend.double()
    want = want.clamp_min(0)
    from tests.parity_log import record_error

    a, b = y.double().cpu().flatten(1), want.cpu().flatten(1)
    assert record_error(((a - b).abs().amax(1) / (b.abs().amax(1) + 1e-300)).max().item()) < 2e-6  # image by image
    assert torch.equal(mask.view(torch.bool).cpu(), (y > 0).cpu())
    assert torch.equal(split.amax.cpu(), y.abs().reshape(N, -1).amax(1).cpu())
    a = split.float().double().cpu().flatten(1)
    b = y.double().cpu().flatten(1)
    assert record_error(((a - b).abs().amax(1) / (b.abs().amax(1) + 1e-300)).max().item()) < 2.0 ** -20
    assert bool((bound.cpu() * (1 + 1e-6) >= split.amax.cpu()).all())
    lo = SEAM - 6
    y2, mask2, split2, bound2 = run(x[lo:].contiguous(), None if addend is None else addend[lo:].contiguous())
    assert torch.equal(y2, y[lo:]) and torch.equal(mask2, mask[lo:]) and torch.equal(bound2, bound[lo:])
    assert torch.equal(split2.planes, split.planes[:, lo:]) and torch.equal(split2.sexp, split.sexp[lo:])
    assert torch.equal(split2.amax, split.amax[lo:])


# ---- the persistent window form of the fused backward-data, at each eligibility edge ---------------------------------------------
# (cotangent channels = the layer's out_channels, result channels = its in_channels, map H x W, images, eligible)
WINDOW_EDGES = [
    (64, 64, 12, 47, 1, True),      # Wi = 47 (the window's LDS rows), N Hi Wi = 564
    (64, 64, 4, 4, 32, True),       # Hi Wi = 16 and N Hi Wi = 512 exactly
    (4064, 64, 8, 8, 8, True),      # Ci = 4064: KC = 254 chunks, the largest the 8-bit fields of the tile descriptor hold
    (4096, 64, 8, 8, 8, False),     # Ci = 4096: refused by lk_conv_winp_eligible, runs the generic fused kernel
]


@needs_library
@pytest.mark.parametrize("cot,res,H,W,N,eligible", WINDOW_EDGES, ids=[f"ci{c[0]}-{c[2]}x{c[3]}-n{c[4]}" for c in WINDOW_EDGES])
def test_window_form_at_its_eligibility_edges(cot, res, H, W, N, eligible):
    """against fp64 (1e-5 of the largest element) and against the generic kernel (4e-6: another order of the K steps), with
    addend + mask + scale.  The two wide cases sum 9 x 4064 / 9 x 4096 products per element, 8 x more than any case
    measured before; for them the error of an fp32 accumulation on the host of the same operands rounded to fp32 is
    recorded next to the device's (tag <host fp32>).  Measured on the MI355X: see profiles/limits_parity.md."""
    from laplace_amd import conv as cv

    Kn = K()
    torch.manual_seed(cot * 7 + res + 3 + 1)
    m = nn.Conv2d(res, cot, 3, 1, 1, bias=False).to(DEV)
    torch.manual_seed(29)
    g = torch.randn(N, cot, H, W, device=DEV) * 1e-2
    gs = Kn.split_f16x2(g.permute(0, 2, 3, 1).contiguous())
    prep = cv.PreparedConv(m)
    assert bool(Kn.conv_winp_eligible(N, H, W, cot, res, 9)) == eligible
    mask = (torch.rand(N, H, W, res, device=DEV) > 0.4).to(torch.uint8)
    addend = Kn.split_f16x2(torch.randn(N, H, W, res, device=DEV) * 0.05)
    sc = (torch.rand(res, device=DEV) * 1.5 + 0.25).contiguous()
    kw = {"add": addend, "mult": mask, "scale": sc, "scale_amax": Kn.absmax(sc)}
    w64, g64 = m.weight.double().cpu(), g.double().cpu()
    want = torch.nn.grad.conv2d_input((N, res, H, W), w64, g64, stride=1, padding=1).permute(0, 2, 3, 1)
    want = (want + addend.float().double().cpu()) * mask.double().cpu() * sc.double().cpu()
    if cot >= 4064:
        host = torch.nn.grad.conv2d_input((N, res, H, W), w64.float(), g64.float(), stride=1, padding=1).permute(0, 2, 3, 1)
        host = (host + addend.float().cpu()) * mask.float().cpu() * sc.float().cpu()
        print(f"host fp32 accumulation, Ci = {cot}: {rel(host, want, tag='host fp32'):.3e}")
    prev = Kn.conv_config
    try:
        Kn.conv_config = 2
        fused = cv.conv_backward_data_vjp(prep, gs, (H, W), **kw)
        Kn.conv_config = 2 | (1 << 27)  # (bit 27: the persistent form off)
        ref = cv.conv_backward_data_vjp(prep, gs, (H, W), **kw)
    finally:
        Kn.conv_config = prev
    e_routes, e_fp64 = rel(fused.float(), ref.float()), rel(fused.float(), want)
    print(f"window form Ci = {cot} {H}x{W} n{N}: vs generic {e_routes:.3e}, vs fp64 {e_fp64:.3e}")
    assert torch.equal(fused.sexp, ref.sexp) and e_routes < 4e-6
    if not eligible:
        assert torch.equal(fused.planes, ref.planes)  # the same kernel both times
    assert abs(fused.amax.item() - fused.float().abs().max().item()) <= 1e-5 * fused.amax.item()
    assert e_fp64 < 1e-5
    assert rel(ref.float(), want) < 1e-5


# ---- the strided backward-data with all twelve tap slots ----------------------------------------------------------------------------
@needs_library
def test_strided_fused_launch_with_twelve_taps():
    """lk_conv_nhwc_f16x2_vjp_strided at T = 12 (13 are refused): laplace_amd/conv.py never builds more than ten (3 x 3 + 1 x 1), so
    the table is built by hand — two sources of six weight slices each (2 x 3 kernels), three taps in each of the four residue
    classes of a stride-2 launch, offsets in {-1, 0, 1}^2 — with addend + mask + scale.  Against fp64 (1e-5 of the largest
    element) and against the class-by-class route: eight plain launches into an fp32 tensor + the element-wise VJP (4e-6)."""
    from laplace_amd import conv as cv

    Kn = K()
    cot, res, Hi, N, S = 64, 32, 4, 8, 2
    Ho, B = 2 * Hi, N // S
    torch.manual_seed(41)
    convs = [nn.Conv2d(res, cot, (2, 3), bias=False).to(DEV) for _ in range(2)]  # weights [cot, res, 2, 3]: six slices each
    gs32 = [torch.randn(N, Hi, Hi, cot, device=DEV) * 1e-2, torch.randn(N, Hi, Hi, cot, device=DEV) * 3.0]
    gs = [Kn.split_f16x2(g) for g in gs32]
    preps = [cv.PreparedConv(m) for m in convs]
    # tap t: offsets (t % 3 - 1, (t // 3) % 3 - 1), slice t % 6 of source t // 6, residue class t % 4
    taps = [(t % 3 - 1, (t // 3) % 3 - 1, t % 6, t // 6, (t % 4) // 2, (t % 4) % 2) for t in range(12)]
    assert len(taps) == 12 and {(t[4], t[5]) for t in taps} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    mask = (torch.rand(B, Ho, Ho, res, device=DEV) > 0.4).to(torch.uint8)
    addend = Kn.split_f16x2(torch.randn(N, Ho, Ho, res, device=DEV) * 0.05)
    sc = (torch.rand(res, device=DEV) * 1.5 + 0.25).contiguous()
    sources = [(g, *p.backward_planes(), p.backward_l1()) for g, p in zip(gs, preps)]
    fused = Kn.conv_nhwc_f16x2_vjp_strided(sources, Ho, Ho, 2, taps, add=addend, mult=mask, scale=sc, scale_amax=Kn.absmax(sc))
    # fp64: dX[n, 2 i + oh0, 2 j + ow0, r] = sum over the class's taps of sum_c g[n, i + dh, j + dw, c] W[c, r, slice]
    want = torch.zeros(N, Ho, Ho, res, dtype=torch.float64)
    for dh, dw, sl, src, oh0, ow0 in taps:
        g = F.pad(gs32[src].double().cpu(), (0, 0, 1, 1, 1, 1))  # one ring of zeros around the map
        W = convs[src].weight.detach().double().cpu().reshape(cot, res, 6)[:, :, sl]
        want[:, oh0::2, ow0::2] += torch.einsum("nijc,cr->nijr", g[:, 1 + dh:1 + dh + Hi, 1 + dw:1 + dw + Hi], W)
    want = want + addend.float().double().cpu()
    want = (want.reshape(S, B, Ho, Ho, res) * mask.double().cpu()).reshape(N, Ho, Ho, res) * sc.double().cpu()
    # the class-by-class route
    dx = torch.zeros(N, Ho, Ho, res, device=DEV)
    for src in range(2):
        planes, sexp = preps[src].backward_planes()
        for oh0 in range(2):
            for ow0 in range(2):
                mine = [(t[0], t[1], t[2]) for t in taps if t[3] == src and (t[4], t[5]) == (oh0, ow0)]
                assert mine
                Kn.conv_nhwc_f16x2(gs[src], planes, sexp, Hi, Hi, 1, dx, 2, oh0, ow0, mine, accumulate=True)
    ref = Kn.vjp_nhwc_split(dx, Kn.absmax(dx), addend, mask, None, sc, Kn.absmax(sc), S, (N, Ho, Ho, res))
    e_routes, e_fp64 = rel(fused.float(), ref.float()), rel(fused.float(), want)
    print(f"strided launch with 12 taps: vs class by class {e_routes:.3e}, vs fp64 {e_fp64:.3e}")
    assert e_routes < 4e-6
    assert abs(fused.amax.item() - fused.float().abs().max().item()) <= 1e-5 * fused.amax.item()
    assert fused.planes[0].abs().max().item() < 2.0 ** 15
    assert e_fp64 < 1e-5
    assert rel(ref.float(), want) < 1e-5
