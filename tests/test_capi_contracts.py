"""The argument contracts of the C ABI (include/laplace_hip.h), probed at their edges WITHOUT a device.

Every guard of laplace_amd/csrc returns LK_EINVAL before the first HIP call, and with no device visible a call that
passes its guards ends in LK_ELAUNCH (or LK_OK for an empty problem) without a kernel ever running.  So "the guard
refused" and "the guard let it through" can be told apart on the CPU tier.  ROWS is the table: one row per limit, with
a complete in-contract argument list, the last accepted and the first refused value of one argument (or a pair), and
a fragment of the message the refusal must carry.  Each pair was derived by reading the guard AND the kernel it
protects (grid extents, 32-bit index products, packed field widths, LDS budgets), not copied from the guard.

The probes run in a CHILD process that cannot see a device (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES empty in the
child's environment only); the child's first act is to assert that, so a regressed guard can never launch a kernel on
the dummy host pointers used here, whatever machine the suite runs on.

Pointer arguments default to the address of a zeroed, 16-byte aligned host buffer; a row overrides one with None
(NULL), "odd" (an address that is 4 mod 16), "other" (a second aligned buffer), a list of ints (a host array of int32 / int64 as the parameter's type
says) or ("ptrs", n) (a host array of n buffer addresses).  `accept=None` marks a limit whose accepted side cannot be
probed without a device (the host code reads device properties before the launch) or which has no accepted neighbour
(a NULL pointer); tests/test_gpu_limits.py runs the accepted side of the numeric ones on the device.
"""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LK_OK, LK_EINVAL, LK_EWORKSPACE, LK_ELAUNCH = 0, -1, -2, -3
BIG = 1 << 40  # a workspace size no guard finds too small (nothing is ever touched: there is no device)


# ---- the header, parsed: name -> [(kind, ctype text, parameter name)] ------------------------------------------------------
def header_prototypes():
    text = open(os.path.join(ROOT, "include", "laplace_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(lk_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = []
        body = " ".join(m.group(2).split())
        if body not in ("", "void"):
            for p in body.split(","):
                p = p.strip()
                pm = re.match(r"(.*?)(\w+)$", p)
                ctype, pname = pm.group(1).strip(), pm.group(2)
                kind = "ptr" if "*" in ctype else ("flt" if ctype in ("float", "double") else "int")
                params.append((kind, ctype, pname))
        out[m.group(1)] = params
    return out


# ---- the table -------------------------------------------------------------------------------------------------------------
def R(fn, base, accept, refuse, fragment):
    return {"fn": fn, "base": base, "accept": accept, "refuse": refuse, "fragment": fragment}


VALUE_PROBES = []  # (key, function, named arguments) of the size_t / int host functions
TAPS9 = [v for t in range(9) for v in (t // 3 - 1, t % 3 - 1, t)]  # {dh, dw, wt} of a 3x3 / padding-1 window
ROWS = []


def _rows(*rows):
    ROWS.extend(rows)


# ---- lk_lik.hip ------------------------------------------------------------------------------------------------------------
_LIK = dict(B=4, C=10)
_rows(
    R("lk_softmax_hess_sqrt_f32", _LIK, {"C": (1 << 24) - 1}, {"C": 1 << 24}, "lk_softmax_hess_sqrt_f32: bad arguments"),
    R("lk_softmax_hess_sqrt_f32", _LIK, {"B": (1 << 31) - 1}, {"B": 1 << 31}, "lk_softmax_hess_sqrt_f32: bad arguments"),
    R("lk_softmax_hess_sqrt_f32", _LIK, {"ws": None, "loss_accum": None}, {"ws": None}, "the loss needs a workspace"),
    # 4 waves x (2C + 1) floats of dynamic LDS: C = 2000 is 64016 bytes, under the 65536 a launch may ask for by default
    R("lk_softmax_hess_chol_f32", _LIK, {"C": 2000}, {"C": 2001}, "(2 <= C <= 2000)"),
    R("lk_softmax_hess_chol_f32", _LIK, {"C": 2}, {"C": 1}, "(2 <= C <= 2000)"),
    R("lk_softmax_hess_chol_f32", _LIK, {"ws": None, "y": None}, {"ws": None}, "the loss needs a workspace"),
    R("lk_sq_err_sum_f32", dict(numel=100, scale=1.0), {"numel": 0}, {"numel": -1}, "lk_sq_err_sum_f32: bad arguments"),
    R("lk_sq_err_sum_f32", dict(numel=100, scale=1.0), None, {"ws": None}, "lk_sq_err_sum_f32: bad arguments"),
)

# ---- lk_pack.hip: grid.y = n -----------------------------------------------------------------------------------------------
_rows(
    R("lk_pack_upper_f32", {}, {"n": 65535}, {"n": 65536}, "lk_pack_upper_f32: bad arguments (n <= 65535)"),
    R("lk_unpack_upper_f32", {}, {"n": 65535}, {"n": 65536}, "lk_unpack_upper_f32: bad arguments (n <= 65535)"),
    R("lk_pack_upper_f32", {}, {"n": 0}, {"n": -1}, "lk_pack_upper_f32: bad arguments"),
)

# ---- lk_diag.hip -----------------------------------------------------------------------------------------------------------
_DL = dict(B=4, Cc=5, Di=3, Do=2, alpha=1.0)
_JL = dict(B=4, Cc=5, Di=3, Do=2, P=8, col0=0, bcol0=6)
_JC = dict(B=4, Cc=5, Cin=2, H=4, W=4, Do=3, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, P=64, col0=0, bcol0=54)
_rows(
    # grid.y = ceil(Do / 16)
    R("lk_diag_ggn_linear_f32", _DL, {"Do": 65535 * 16}, {"Do": 65535 * 16 + 1}, "lk_diag_ggn_linear_f32: Do too large"),
    R("lk_diag_ggn_linear_f32", _DL, {"Cc": 1}, {"Cc": 0}, "lk_diag_ggn_linear_f32: bad arguments"),
    # B, Cc, Di travel as int (2^32 samples would be read as none); grid.x = ceil(Di / 16)
    R("lk_diag_ggn_linear_f32", _DL, {"B": (1 << 31) - 1}, {"B": 1 << 31}, "lk_diag_ggn_linear_f32: B, Cc, Di must be < 2^31"),
    R("lk_diag_ggn_linear_f32", _DL, {"B": (1 << 31) - 1}, {"B": 1 << 32}, "lk_diag_ggn_linear_f32: B, Cc, Di must be < 2^31"),
    R("lk_diag_ggn_linear_f32", _DL, {"Cc": (1 << 31) - 1}, {"Cc": 1 << 31}, "lk_diag_ggn_linear_f32: B, Cc, Di must be < 2^31"),
    R("lk_diag_ggn_linear_f32", _DL, {"Di": (1 << 31) - 17}, {"Di": (1 << 31) - 16}, "lk_diag_ggn_linear_f32: B, Cc, Di must be < 2^31"),
    R("lk_jac_linear_f32", _JL, {"Di": (1 << 31) - 1, "Do": 1, "P": 1 << 31, "bcol0": -1}, {"Di": 1 << 31, "Do": 1, "P": 1 << 32, "bcol0": -1},
      "lk_jac_linear_f32: Di, Do must be < 2^31"),
    R("lk_sq_colsum_f32", dict(rows=4, P=1 << 40, col0=0, width=8, alpha=1.0), {"width": (1 << 39) - 1}, {"width": 1 << 39}, "lk_sq_colsum_f32: width too large"),
    # grid.y = B * Cc
    R("lk_jac_linear_f32", _JL, {"B": 13107}, {"B": 13108}, "lk_jac_linear_f32: B*C too large for grid.y"),
    R("lk_jac_linear_f32", _JL, {"P": 6, "bcol0": -1}, {"P": 5, "bcol0": -1}, "lk_jac_linear_f32: bad arguments"),
    R("lk_jac_linear_f32", _JL, {"col0": 0}, {"col0": -1}, "lk_jac_linear_f32: bad arguments"),
    # grid.z = B * Cc, grid.y = ceil(Do / 16)
    R("lk_jac_conv_f32", _JC, {"B": 13107}, {"B": 13108}, "lk_jac_conv_f32: B*C too large for grid.z"),
    R("lk_jac_conv_f32", _JC, {"Do": 65535 * 16, "P": 65535 * 16 * 18, "bcol0": -1}, {"Do": 65535 * 16 + 1, "P": 1 << 40, "bcol0": -1},
      "lk_jac_conv_f32: Do too large for grid.y"),
    R("lk_jac_conv_f32", _JC, {"sh": 1}, {"sh": 0}, "lk_jac_conv_f32: bad geometry"),
    R("lk_jac_conv_f32", _JC, {"H": 1, "W": 1}, {"H": 1, "W": 1, "ph": 0, "pw": 0}, "lk_jac_conv_f32: empty output"),
    R("lk_jac_conv_f32", _JC, {"P": 54, "bcol0": -1}, {"P": 53, "bcol0": -1}, "lk_jac_conv_f32: column range outside Js"),
    R("lk_sq_colsum_f32", dict(rows=4, P=10, col0=2, width=8, alpha=1.0), {"width": 8}, {"width": 9}, "lk_sq_colsum_f32: bad arguments"),
)

# ---- lk_ll.hip -------------------------------------------------------------------------------------------------------------
_LL = dict(B=4, C=3, D=5, has_bias=1, alpha=1.0, ws_bytes=BIG)
_rows(
    # P = C (D + 1) < 2^20: the dense GGN is P x P
    R("lk_ll_ggn_full_f32", _LL, {"C": 1023, "D": 1024}, {"C": 1024, "D": 1023}, "lk_ll_ggn_full_f32: P too large"),
    R("lk_ll_ggn_full_f32", _LL, {"D": 1}, {"D": 0}, "lk_ll_ggn_full_f32: bad arguments"),
    R("lk_jac_last_layer_f32", dict(B=4, C=3, D=5, has_bias=1), {"C": 1}, {"C": 0}, "lk_jac_last_layer_f32: bad arguments"),
    R("lk_jac_last_layer_f32", dict(B=4, C=3, D=5, has_bias=1), {"D": (1 << 31) - 1}, {"D": 1 << 31}, "lk_jac_last_layer_f32: C, D must be < 2^31"),
    R("lk_dense_quadform_ll_f32", dict(B=4, C=3, D=5, has_bias=1, ws_bytes=0), {"D": (1 << 31) - 2}, {"D": (1 << 31) - 1}, "D must be < 2^31 - 1, B < 2^38"),
    R("lk_dense_quadform_ll_f32", dict(B=4, C=3, D=5, has_bias=1, ws_bytes=0), {"B": (1 << 38) - 1}, {"B": 1 << 38}, "D must be < 2^31 - 1, B < 2^38"),
    # grid.y = C (C + 1) / 2: 361 classes are 65341 pairs, 362 are 65703
    R("lk_dense_quadform_ll_f32", dict(B=4, C=3, D=5, has_bias=1, ws_bytes=0), {"C": 361}, {"C": 362},
      "lk_dense_quadform_ll_f32: too many class pairs"),
    R("lk_dense_quadform_ll_f32", dict(B=4, C=3, D=5, has_bias=1, ws_bytes=0), {"B": 0}, {"B": -1}, "lk_dense_quadform_ll_f32: bad arguments"),
)

# ---- lk_kron.hip -----------------------------------------------------------------------------------------------------------
_LD = dict(n1=4, n2=3, damping=0, ws_bytes=BIG)
_QL = dict(B=4, Cc=3, Do=8, Di=16)
_rows(
    R("lk_kron_logdet_f32", _LD, {"n1": 1}, {"n1": 0}, "lk_kron_logdet_f32: bad arguments"),
    R("lk_kron_logdet_f32", _LD, {"n2": 0, "l2": None}, {"n2": 1, "l2": None}, "lk_kron_logdet_f32: bad arguments"),
    R("lk_kron_logdet_f32", _LD, {"damping": 1, "d_l1": None, "d_l2": None, "d_delta": None}, {"damping": 1}, "no derivatives with damping"),
    R("lk_kron_logdet_blocks_f32", dict(nblocks=2, l1=("ptrs", 2), n1=[4, 4], l2=("ptrs", 2), n2=[3, 0], ws_bytes=BIG),
      {"n1": [(1 << 30) - 5, 4]}, {"n1": [1 << 30, 4]}, "lk_kron_logdet_blocks_f32: bad block"),
    R("lk_kron_logdet_blocks_f32", dict(nblocks=2, l1=("ptrs", 2), n1=[4, 4], l2=("ptrs", 2), n2=[3, 0], ws_bytes=BIG),
      {"n1": [(1 << 29), (1 << 29) - 1]}, {"n1": [1 << 29, 1 << 29]}, "lk_kron_logdet_blocks_f32: too many eigenvalues"),
    R("lk_kron_logdet_blocks_f32", dict(nblocks=2, l1=("ptrs", 2), n1=[4, 4], l2=("ptrs", 2), n2=[3, 0], ws_bytes=BIG),
      {"nblocks": 0, "l1": None}, {"l1": None}, "lk_kron_logdet_blocks_f32: bad arguments"),
    # dynamic LDS = (Di + 2 Do) floats <= 150 KiB = 38400 floats
    R("lk_kron_quadform_linear_f32", _QL, {"Do": 200, "Di": 38000}, {"Do": 200, "Di": 38001}, "(Di + 2*Do = 38401 floats)"),
    R("lk_kron_quadform_linear_f32", _QL, {"ub": None, "lb": None}, {"lb": None}, "bias block needs lb and delta_b"),
    R("lk_kron_quadform_linear_f32", _QL, {"Cc": 1}, {"Cc": 0}, "lk_kron_quadform_linear_f32: bad arguments"),
    # grid.x = B workgroups and (int)B: 2^31 samples are past the grid, 2^32 + k would be read as k; Cc * Cc is formed in int
    R("lk_kron_quadform_linear_f32", _QL, {"B": (1 << 31) - 1}, {"B": 1 << 31}, "quadform_linear: B must be < 2^31 and Cc <= 32768"),
    R("lk_kron_quadform_linear_f32", _QL, {"B": (1 << 31) - 1}, {"B": (1 << 32) + 3}, "quadform_linear: B must be < 2^31 and Cc <= 32768"),
    R("lk_kron_quadform_linear_f32", _QL, {"Cc": 32768}, {"Cc": 32769}, "quadform_linear: B must be < 2^31 and Cc <= 32768"),
    R("lk_diag_quadform_linear_f32", _QL, {"B": (1 << 31) - 1}, {"B": 1 << 31}, "quadform_linear: B must be < 2^31 and Cc <= 32768"),
    R("lk_diag_quadform_linear_f32", _QL, {"Cc": 32768}, {"Cc": 32769}, "quadform_linear: B must be < 2^31 and Cc <= 32768"),
    R("lk_kron_logdet_f32", _LD, {"n1": (1 << 31) - 5}, {"n1": (1 << 31) - 4}, "lk_kron_logdet_f32: n1, n2 must be < 2^31 - 4"),
    R("lk_kron_logdet_f32", _LD, {"n2": (1 << 31) - 5}, {"n2": (1 << 31) - 4}, "lk_kron_logdet_f32: n1, n2 must be < 2^31 - 4"),
    R("lk_diag_quadform_linear_f32", _QL, {"Do": 4096, "Di": 30208}, {"Do": 4096, "Di": 30209}, "(Di + 2*Do = 38401 floats)"),
    R("lk_diag_quadform_linear_f32", _QL, {"Do": 1}, {"Do": 0}, "lk_diag_quadform_linear_f32: bad arguments"),
    # grid = (C, C, B)
    R("lk_diag_quadform_js_f32", dict(B=4, C=3, P=7), {"B": 65535}, {"B": 65536}, "lk_diag_quadform_js_f32: bad arguments"),
    R("lk_diag_quadform_js_f32", dict(B=4, C=3, P=7), {"C": 65535}, {"C": 65536}, "lk_diag_quadform_js_f32: bad arguments"),
)

# ---- lk_gemm.hip -----------------------------------------------------------------------------------------------------------
_GM = dict(batch=2, M=64, N=64, K=8, lda=8, ldb=64, ldc=64, lde=0, stride_a=512, stride_b=512, stride_c=4096, trans_a=0,
           trans_b=0, alpha=1.0, accumulate=0)
_rows(
    # grid.y = ceil(M / 64) row tiles
    R("lk_gemm_f32", _GM, {"M": 65535 * 64}, {"M": 65535 * 64 + 1}, "lk_gemm_f32: too many row tiles"),
    R("lk_gemm_f32", _GM, {"K": (1 << 31) - 1}, {"K": 1 << 31}, "lk_gemm_f32: extents too large"),
    R("lk_gemm_f32", _GM, {"batch": 65536 * 32768 - 1}, {"batch": 65536 * 32768}, "lk_gemm_f32: extents too large"),
    R("lk_gemm_f32", _GM, {"N": 0}, {"N": -1}, "lk_gemm_f32: bad arguments"),
    R("lk_kron_pow_f32", dict(n1=4, n2=3, exponent=-1.0, damping=0), {"n1": 0}, {"n1": -1}, "lk_kron_pow_f32: bad arguments"),
    R("lk_kron_pow_f32", dict(n1=4, n2=3, exponent=-1.0, damping=0), {"n1": (1 << 31) - 1}, {"n1": 1 << 31}, "lk_kron_pow_f32: n1, n2 must be < 2^31"),
    R("lk_kron_pow_f32", dict(n1=4, n2=3, exponent=-1.0, damping=0), {"l2": None, "n2": -1}, {"n2": -1}, "lk_kron_pow_f32: bad arguments"),
)

# ---- lk_vjp.hip ------------------------------------------------------------------------------------------------------------
_BN = dict(total=2 * 3 * 4, C=3, HW=4, relu=1)
_VS = dict(m_is_float=0, S=2, per_sample=24, C=3, HW=4)
_rows(
    R("lk_bn_act_fwd_f32", _BN, {"total": 24}, {"total": 25}, "lk_bn_act_fwd_f32: bad arguments"),
    R("lk_bn_act_fwd_f32", _BN, {"C": 1, "HW": (1 << 31) - 1, "total": (1 << 31) - 1}, {"C": 1, "HW": 1 << 31, "total": 1 << 31},
      "lk_bn_act_fwd_f32: bad arguments"),
    # 256 elements per workgroup (unaligned form), grid.x < 2^31
    R("lk_bn_act_fwd_f32", _BN, {"C": 1, "HW": 1, "total": ((1 << 31) - 1) * 256, "x": "odd"}, {"C": 1, "HW": 1, "total": (1 << 31) * 256, "x": "odd"},
      "lk_bn_act_fwd_f32: grid too large"),
    R("lk_vjp_scale_mask_f32", _VS, {"per_sample": 24}, {"per_sample": 25}, "per_sample must be B*C*HW"),
    R("lk_vjp_scale_mask_f32", _VS, {"S": (1 << 30) - 1}, {"S": 1 << 30}, "lk_vjp_scale_mask_f32: extents too large"),
    R("lk_vjp_scale_mask_f32", _VS, {"scale": None, "per_sample": ((1 << 31) - 1) * 256, "g": "odd"},
      {"scale": None, "per_sample": (1 << 31) * 256, "g": "odd"}, "lk_vjp_scale_mask_f32: grid too large"),
    R("lk_vjp_scale_mask_f32", _VS, {"S": 0}, {"S": -1}, "lk_vjp_scale_mask_f32: bad arguments"),
)

# ---- lk_norm.hip -----------------------------------------------------------------------------------------------------------
_JN = dict(S=3, B=4, L=5, Ch=6, layout=0, P=20, wcol0=2, bcol0=8)
_rows(
    R("lk_jac_norm_affine_f32", _JN, {"layout": 1}, {"layout": 2}, "lk_jac_norm_affine_f32: bad arguments"),
    R("lk_jac_norm_affine_f32", _JN, {"L": (1 << 30) - 1}, {"L": 1 << 30}, "lk_jac_norm_affine_f32: extent too large"),
    R("lk_jac_norm_affine_f32", _JN, {"B": (1 << 31) - 1, "Ch": 1, "bcol0": -1}, {"B": 1 << 31, "Ch": 1, "bcol0": -1}, "lk_jac_norm_affine_f32: extent too large"),
    R("lk_jac_norm_affine_f32", _JN, {"bcol0": 14}, {"bcol0": 15}, "lk_jac_norm_affine_f32: column range outside Js"),
    R("lk_jac_norm_affine_f32", _JN, {"bcol0": 8}, {"bcol0": 7}, "lk_jac_norm_affine_f32: weight and bias columns overlap"),
)

# ---- lk_grid.hip -----------------------------------------------------------------------------------------------------------
_LG = dict(G=3, mode=0, B=4, C=3, Do=8, Di=16)
_SG = dict(G=3, mode=0, B=4, C=3, Do=8, Dk=16, L=4, seed_major=0, ws_bytes=BIG)
_rows(
    # dynamic LDS = GRID_LIN_NB (Di + GS Do) floats <= 150 KiB with GRID_LIN_NB = 4 samples per workgroup: Di + Do <= 9600
    R("lk_quadform_linear_grid_f32", _LG, {"Do": 100, "Di": 9500}, {"Do": 100, "Di": 9501}, "layer too wide for the LDS-staged kernel (Di = 9501, Do = 100)"),
    R("lk_quadform_linear_grid_f32", _LG, {"mode": 2}, {"mode": 3}, "lk_quadform_linear_grid_f32: bad arguments"),
    R("lk_quadform_linear_grid_f32", _LG, {"mode": 2, "w1": None}, {"mode": 1, "w1": None}, "Kron modes need l2"),
    R("lk_quadform_linear_grid_f32", _LG, {"ub": None, "wb": None}, {"wb": None}, "bias block needs its weights"),
    R("lk_quadform_linear_grid_f32", _LG, {"G": (1 << 24) - 1}, {"G": 1 << 24}, "lk_quadform_linear_grid_f32: sizes out of range"),
    R("lk_quadform_linear_grid_f32", _LG, {"B": (1 << 30) - 1}, {"B": 1 << 30}, "lk_quadform_linear_grid_f32: sizes out of range"),
    R("lk_quadform_shared_grid_f32", _SG, {"mode": 2}, {"mode": 3}, "lk_quadform_shared_grid_f32: bad arguments"),
    R("lk_quadform_shared_grid_f32", _SG, {"mode": 2, "w1": None}, {"mode": 0, "w1": None}, "Kron modes need l2"),
    R("lk_quadform_shared_grid_f32", _SG, {"B": (1 << 25) - 1}, {"B": 1 << 25}, "lk_quadform_shared_grid_f32: sizes out of range"),
    R("lk_quadform_shared_grid_f32", _SG, {"L": 1 << 13, "Dk": (1 << 16) - 1}, {"L": 1 << 13, "Dk": 1 << 16}, "lk_quadform_shared_grid_f32: sizes out of range"),
    R("lk_quadform_shared_grid_f32", _SG, {"C": 4, "L": 1 << 12, "Do": (1 << 15) - 1}, {"C": 4, "L": 1 << 12, "Do": 1 << 15}, "lk_quadform_shared_grid_f32: sizes out of range"),
    R("lk_quadform_shared_grid_f32", _SG, {"seed_major": 1, "C": 4, "B": 4, "L": 1 << 12, "Do": (1 << 15) - 1},
      {"seed_major": 1, "C": 4, "B": 4, "L": 1 << 12, "Do": 1 << 15}, "lk_quadform_shared_grid_f32: sizes out of range"),
    R("lk_probit_nll_grid_f32", dict(G=3, B=4, C=5), {"C": (1 << 24) - 1}, {"C": 1 << 24}, "lk_probit_nll_grid_f32: bad arguments"),
    R("lk_probit_nll_grid_f32", dict(G=3, B=4, C=5), {"G": (1 << 31) - 1}, {"G": 1 << 31}, "lk_probit_nll_grid_f32: bad arguments"),
)

# ---- lk_quadconv.hip -------------------------------------------------------------------------------------------------------
_QS = dict(B=4, C=3, Do=32, Dk=16, L=16, ws_bytes=BIG)
_QP = dict(v_nsexp=1, B=4, C=3, Do=32, Dk=16, L=16, ws_bytes=BIG)
_DG = dict(B=4, S=3, Do=32, Dk=16, L=16, alpha=1.0, ws_bytes=BIG)
for _fn in ("lk_kron_quadform_shared_f32", "lk_diag_quadform_shared_f32"):
    _rows(
        # the class tile: at most 10 outputs per launch
        R(_fn, _QS, {"C": 10}, {"C": 11}, _fn + ": more than 10 outputs"),
        # 32-bit element offsets inside one sample's operands; B * split workgroups
        R(_fn, _QS, {"B": (1 << 25) - 1}, {"B": 1 << 25}, _fn + ": sizes out of range"),
        R(_fn, _QS, {"C": 4, "L": 1 << 12, "Do": (1 << 15) - 1}, {"C": 4, "L": 1 << 12, "Do": 1 << 15}, _fn + ": sizes out of range"),
        R(_fn, _QS, {"L": 1 << 13, "Dk": (1 << 16) - 1}, {"L": 1 << 13, "Dk": 1 << 16}, _fn + ": sizes out of range"),
        R(_fn, _QS, {"L": 1}, {"L": 0}, _fn + ": bad arguments"),
    )
_rows(
    R("lk_diag_quadform_shared_f32", _QS, {"Do": 1 << 15, "Dk": (1 << 16) - 1, "L": 1, "C": 1}, {"Do": 1 << 15, "Dk": 1 << 16, "L": 1, "C": 1},
      "lk_diag_quadform_shared_f32: sizes out of range"),
    R("lk_kron_quadform_shared_seedmajor_f32", _QS, {"C": 10}, {"C": 11}, "lk_kron_quadform_shared_seedmajor_f32: more than 10 outputs"),
    R("lk_kron_quadform_shared_seedmajor_f32", _QS, {"C": 4, "B": 4, "L": 1 << 12, "Do": (1 << 15) - 1}, {"C": 4, "B": 4, "L": 1 << 12, "Do": 1 << 15},
      "lk_kron_quadform_shared_seedmajor_f32: sizes out of range"),
    R("lk_kron_quadform_shared_seedmajor_f32", _QS, {"Dk": 1}, {"Dk": 0}, "lk_kron_quadform_shared_seedmajor_f32: bad arguments"),
    R("lk_kron_quadform_shared_planes_f16x2", _QP, {"C": 10}, {"C": 11}, "lk_kron_quadform_shared_planes_f16x2: more than 10 outputs"),
    R("lk_kron_quadform_shared_planes_f16x2", _QP, {"L": 32}, {"L": 24}, "L % 16 == 0, Do % 32 == 0"),
    R("lk_kron_quadform_shared_planes_f16x2", _QP, {"Do": 64}, {"Do": 48}, "L % 16 == 0, Do % 32 == 0"),
    R("lk_kron_quadform_shared_planes_f16x2", _QP, {"v_nsexp": 4}, {"v_nsexp": 3}, "v_nsexp in {1, B}"),
    R("lk_kron_quadform_shared_planes_f16x2", _QP, {"C": 4, "B": 4, "L": 1 << 12, "Do": (1 << 15) - 32}, {"C": 4, "B": 4, "L": 1 << 12, "Do": 1 << 15},
      "lk_kron_quadform_shared_planes_f16x2: sizes out of range"),
    R("lk_kron_quadform_shared_planes_f16x2", _QP, None, {"v_l": "odd"}, "16-byte aligned planes"),
    R("lk_kron_quadform_shared_planes_f16x2", _QP, None, {"zero16": None}, "lk_kron_quadform_shared_planes_f16x2: bad arguments"),
    # at most 10 seeds per call
    R("lk_diag_ggn_shared_f32", _DG, {"S": 10}, {"S": 11}, "more than 10 seeds per call"),
    R("lk_diag_ggn_shared_f32", _DG, {"S": 4, "L": 1 << 12, "Do": (1 << 15) - 1}, {"S": 4, "L": 1 << 12, "Do": 1 << 15}, "lk_diag_ggn_shared_f32: sizes out of range"),
    R("lk_diag_ggn_shared_f32", _DG, {"Do": 1 << 15, "Dk": (1 << 16) - 1, "L": 1, "S": 1}, {"Do": 1 << 15, "Dk": 1 << 16, "L": 1, "S": 1},
      "lk_diag_ggn_shared_f32: sizes out of range"),
    R("lk_diag_ggn_shared_f32", _DG, {"S": 1}, {"S": 0}, "lk_diag_ggn_shared_f32: bad arguments"),
    R("lk_diag_ggn_shared_f32", _DG, {"B": (1 << 31) - 1}, {"B": 1 << 31}, "lk_diag_ggn_shared_f32: sizes out of range"),
)

# ---- lk_eigh.hip -----------------------------------------------------------------------------------------------------------
_rows(
    R("lk_syevj_f32", dict(n=8, clamp=1, max_sweeps=0, ws_bytes=BIG), {"n": 0}, {"n": -1}, "lk_syevj_f32: bad arguments"),
    # (the accepted side of n <= 32768 would enqueue 24 sweeps of launches: tests/test_gpu_limits.py names it as left out)
    R("lk_syevj_f32", dict(n=8, clamp=1, max_sweeps=0, ws_bytes=BIG), None, {"n": 32769}, "lk_syevj_f32: bad arguments"),
    R("lk_syevj_batched_f32", dict(count=2, A=("ptrs", 2), n=[8, 8], w=("ptrs", 2), Q=("ptrs", 2), info=("ptrs", 2), ws=("ptrs", 2),
                                   ws_bytes=[BIG, BIG], clamp=1, max_sweeps=0, streams=("ptrs", 1), nstreams=1),
      None, {"n": [8, 32769]}, "lk_syevj_batched_f32: bad matrix"),
    R("lk_syevj_batched_f32", dict(count=2, A=("ptrs", 2), n=[8, 8], w=("ptrs", 2), Q=("ptrs", 2), info=("ptrs", 2), ws=("ptrs", 2),
                                   ws_bytes=[BIG, BIG], clamp=1, max_sweeps=0, streams=("ptrs", 1), nstreams=1),
      {"count": 0, "nstreams": 1}, {"count": 0, "nstreams": 0}, "lk_syevj_batched_f32: bad arguments"),
)

# ---- lk_comm.cpp: only the checks that return before RCCL is looked for ------------------------------------------------------
_rows(
    R("lk_comm_unique_id", {}, None, {"id128": None}, "lk_comm_unique_id: null pointer"),
    R("lk_comm_init_rank", dict(nranks=2, rank=1), None, {"rank": 2}, "lk_comm_init_rank: bad arguments"),
    R("lk_comm_init_rank", dict(nranks=2, rank=1), None, {"nranks": 0, "rank": 0}, "lk_comm_init_rank: bad arguments"),
    R("lk_allreduce_sum_f32", dict(count=4), {"count": 0}, {"count": -1}, "lk_allreduce_sum_f32: bad arguments"),
    R("lk_allreduce_sum_f32", dict(count=4), {"count": 0, "buf": None}, {"buf": None}, "lk_allreduce_sum_f32: bad arguments"),
)

# ---- lk_gram.hip -----------------------------------------------------------------------------------------------------------
_GT = dict(K=16, n=8, ldx=8, alpha=1.0, flags=0, ws_bytes=BIG)
_GS = dict(segs=("ptrs", 16), nseg=2, nb=3, n=8, L=4, alpha=1.0, flags=0, ws_bytes=BIG)
_GC = dict(B=2, H=4, W=4, Cin=4, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, alpha=1.0, flags=0, ws_bytes=BIG)
_PA = dict(B=2, H=2, W=2, Cin=64, alpha=1.0, n_tiles=10)  # (a 2 x 2 map has 10 pixel pairs)
_AS = dict(H=4, W=4, Cin=64, alpha=1.0, upper_only=0)
_rows(
    R("lk_gram_slabs_reduce_f32", dict(slabs_bytes=BIG, n=8, L_nt=0, alpha=1.0, flags=0), {"n": 1}, {"n": 0}, "lk_gram_slabs_reduce_f32: bad arguments"),
    R("lk_gram_slabs_reduce_f32", dict(slabs_bytes=BIG, n=8, L_nt=0, alpha=1.0, flags=0), None, {"n": 1 << 30}, "lk_gram_slabs_reduce_f32: bad arguments"),
    R("lk_gram_slabs_reduce_f32", dict(slabs_bytes=BIG, n=8, L_nt=0, alpha=1.0, flags=0), None, {"slabs_bytes": 16}, "buffer smaller than one slab"),
    R("lk_gram_tn_f32", _GT, {"ldx": 8}, {"ldx": 7}, "lk_gram_tn_f32: bad arguments"),
    R("lk_gram_tn_f32", _GT, None, {"n": 1 << 30, "ldx": 1 << 30}, "lk_gram_tn_f32: n too large"),
    R("lk_gram_nt_seg_f32", _GS, {"nseg": 16}, {"nseg": 17}, "(at most 16 segments)"),
    R("lk_gram_nt_seg_f32", _GS, None, {"L": 1 << 30}, "lk_gram_nt_seg_f32: dims too large"),
    R("lk_gram_nt_seg_f32", _GS, None, {"segs": [0, 0]}, "lk_gram_nt_seg_f32: null segment"),
    R("lk_gram_nt_f32", dict(nb=3, n=8, L=4, alpha=1.0, flags=0, ws_bytes=BIG), None, {"X": None}, "lk_gram_nt_f32: bad arguments"),
    R("lk_gram_conv_nhwc_f32", _GC, {"sw": 1}, {"sw": 0}, "lk_gram_conv_nhwc_f32: bad arguments"),
    R("lk_gram_conv_nhwc_f32", _GC, {"H": 1, "W": 1}, {"H": 1, "W": 1, "ph": 0, "pw": 0}, "lk_gram_conv_nhwc_f32: empty output"),
    # rows of the patch matrix are indexed with 32 bits (and padded to a chunk of 64)
    R("lk_gram_conv_nhwc_f32", _GC, {"B": ((1 << 31) - 80) // 16}, {"B": (1 << 31) // 16}, "B*OH*OW must be < 2^31"),
    # grid = (ceil(HW / 64), ceil(C / 64), B)
    R("lk_nchw_to_nhwc_f32", dict(B=2, C=3, HW=4), {"B": 65535}, {"B": 65536}, "batch too large for grid.z"),
    R("lk_nchw_to_nhwc_f32", dict(B=2, C=3, HW=4), {"C": 65535 * 64}, {"C": 65535 * 64 + 1}, "C too large for grid.y"),
    R("lk_nchw_to_nhwc_f32", dict(B=2, C=3, HW=4), {"HW": 1}, {"HW": 0}, "lk_nchw_to_nhwc_f32: bad arguments"),
    R("lk_symmetrize_f32", {}, {"n": 0}, {"n": -1}, "lk_symmetrize_f32: bad arguments"),
    # grid = (ceil(n / 64), ceil(n / 64))
    R("lk_symmetrize_f32", {}, {"n": 65535 * 64}, {"n": 65535 * 64 + 1}, "lk_symmetrize_f32: n too large for grid.y"),
    R("lk_permute_sym_f32", dict(Cin=4, KK=9, accumulate=0, dst="other"), {"Cin": (1 << 24) // 9}, {"Cin": (1 << 24) // 9 + 1}, "Cin * KK must be < 2^24"),
    R("lk_permute_sym_f32", dict(Cin=4, KK=9, accumulate=0, dst="other"), {"KK": 1}, {"KK": 0}, "lk_permute_sym_f32: bad arguments"),
    R("lk_permute_sym_f32", dict(Cin=4, KK=9, accumulate=0, dst="other"), None, {"dst": "same"}, "lk_permute_sym_f32: bad arguments"),
    R("lk_finalize_factors_f32", dict(count=2, src=("ptrs", 2), dst=[0, 0], scale=[0, 0], n=[8, 8], cin=[8, 8], kk=[1, 1]),
      {"n": [8, (1 << 24) - 1]}, {"n": [8, 1 << 24]}, "lk_finalize_factors_f32: bad factor"),
    R("lk_finalize_factors_f32", dict(count=2, src=("ptrs", 2), dst=[0, 0], scale=[0, 0], n=[8, 8], cin=[8, 8], kk=[1, 1]),
      {"count": 0, "n": None}, {"n": None}, "lk_finalize_factors_f32: bad arguments"),
    R("lk_finalize_factors_f32", dict(count=1, src=("ptrs", 1), dst=[0], scale=[0], n=[36], cin=[4], kk=[9]),
      None, {"dst": [0]}, "a permuted factor needs dst != src"),
    R("lk_conv3x3_pixpair_plan", dict(H=4, W=4, Cin=64), {"Cin": 128}, {"Cin": 96}, "needs Cin % 64 == 0"),
    # up to 13 blocks of Cin x Cin floats per pixel, indexed with 32 bits: a 203 x 200 map of 64 channels has 521773 blocks
    # (< 2^31 / 4096 = 524288; border pixels lack some of their 13 shifts), one more row of pixels makes 524358
    R("lk_conv3x3_pixpair_plan", dict(H=4, W=4, Cin=64), {"H": 203, "W": 200}, {"H": 204, "W": 200}, "lk_conv3x3_pixpair_plan: problem too large"),
    R("lk_conv3x3_pixpair_plan", dict(H=4, W=4, Cin=64), None, {"H": 1 << 20, "W": 1 << 20}, "lk_conv3x3_pixpair_plan: problem too large"),
    R("lk_conv3x3_pixpair_tables", dict(H=2, W=2, Cin=64, tiles=[0] * 64, slots=[0] * 64), {"Cin": 64}, {"Cin": 32}, "needs Cin % 64 == 0"),
    R("lk_conv3x3_pixpair_tables", dict(H=2, W=2, Cin=64, tiles=[0] * 64, slots=[0] * 64), None, {"slots": None}, "lk_conv3x3_pixpair_tables: null table"),
    R("lk_conv3x3_pixpair_accumulate_f32", _PA, {"n_tiles": 10}, {"n_tiles": 11}, "table does not match the geometry"),
    R("lk_conv3x3_pixpair_accumulate_f32", _PA, None, {"x": "odd"}, "unaligned input"),
    R("lk_conv3x3_pixpair_accumulate_f32", _PA, {"B": 0}, {"B": -1}, "lk_conv3x3_pixpair_accumulate_f32: bad arguments"),
    R("lk_conv3x3_pixpair_assemble2_f32", _AS, {"Cin": 4}, {"Cin": 6}, "Cin % 4 == 0 and 16-byte aligned buffers"),
    R("lk_conv3x3_pixpair_assemble2_f32", _AS, {"blocks2": None}, {"blocks2": "odd"}, "Cin % 4 == 0 and 16-byte aligned buffers"),
    R("lk_conv3x3_pixpair_assemble2_f32", _AS, {"H": 4095, "W": 4096}, {"H": 4096, "W": 4096}, "lk_conv3x3_pixpair_assemble_f32: bad arguments"),
    R("lk_conv3x3_pixpair_assemble_f32", dict(H=4, W=4, Cin=64, alpha=1.0), {"Cin": 1864132}, {"Cin": 1864136}, "lk_conv3x3_pixpair_assemble_f32: bad arguments"),
    R("lk_conv3x3_pixgram_assemble_f32", dict(H=4, W=4, Cin=8, alpha=1.0), {"H": 16383, "W": 16384}, {"H": 16384, "W": 16384},
      "lk_conv3x3_pixgram_assemble_f32: bad arguments"),
    R("lk_conv3x3_shiftcorr_f32", dict(B=2, H=4, W=4, Cin=8, alpha=1.0, ws_bytes=BIG), {"H": 2}, {"H": 1}, "lk_conv3x3_shiftcorr_f32: bad arguments"),
    R("lk_conv3x3_shiftcorr_f32", dict(B=2, H=4, W=4, Cin=8, alpha=1.0, ws_bytes=BIG), None, {"B": (1 << 31) // 16}, "lk_conv3x3_shiftcorr_f32: problem too large"),
    R("lk_conv3x3_shiftcorr_f32", dict(B=2, H=4, W=4, Cin=8, alpha=1.0, ws_bytes=BIG), None, {"Cin": 671089}, "lk_conv3x3_shiftcorr_f32: problem too large"),
)

# ---- lk_sweep16.hip --------------------------------------------------------------------------------------------------------
_VN = dict(m_is_float=0, C=8, S=2, per=64)
_BA = dict(x_namax=1, addend_nbound=1, act=1, C=8, N=4, per=64)
_UT = dict(S=3, B=4, L=5, C=6)
_G16 = dict(R=100, C=128, alpha=1.0, ws_bytes=BIG)
_P13 = dict(B=2, H=4, W=4, Cin=64, alpha=1.0)
_P16 = dict(B=2, H=2, W=2, Cin=64, alpha=1.0, n_tiles=10)
_rows(
    R("lk_vjp_nhwc_split_f16x2", _VN, {"per": 64, "scale": None}, {"per": 68, "scale": None}, "lk_vjp_nhwc_split_f16x2: per % 8 == 0"),
    R("lk_vjp_nhwc_split_f16x2", _VN, {"C": 16}, {"C": 12, "per": 96}, "scale needs C % 8 == 0"),
    R("lk_vjp_nhwc_split_f16x2", _VN, {"S": (1 << 30) - 1}, {"S": 1 << 30}, "lk_vjp_nhwc_split_f16x2: per % 8 == 0"),
    R("lk_vjp_nhwc_split_f16x2", _VN, {"scale": None, "per": ((1 << 31) - 1) * 2048}, {"scale": None, "per": (1 << 31) * 2048}, "lk_vjp_nhwc_split_f16x2: grid too large"),
    R("lk_vjp_nhwc_split_f16x2", _VN, {"g": None, "g_amax": None}, {"g_amax": None}, "the fp32 addend needs its max"),
    R("lk_vjp_nhwc_split_f16x2", _VN, {"g2_h": None, "g2_l": None}, {"g2_l": None}, "incomplete split addend"),
    # grid.y = N images
    R("lk_bn_act_fwd_nhwc_f16x2", _BA, {"N": 65535}, {"N": 65536}, "lk_bn_act_fwd_nhwc_f16x2: at most 65535 images"),
    R("lk_bn_act_fwd_nhwc_f16x2", _BA, {"C": 16}, {"C": 12, "per": 96}, "C % 8 == 0, act in 0..2"),
    R("lk_bn_act_fwd_nhwc_f16x2", _BA, {"act": 2}, {"act": 3}, "C % 8 == 0, act in 0..2"),
    R("lk_bn_act_fwd_nhwc_f16x2", _BA, {"x_namax": 4}, {"x_namax": 3}, "x_amax has 1 or N words"),
    R("lk_bn_act_fwd_nhwc_f16x2", _BA, {"addend_nbound": 4}, {"addend_nbound": 2}, "the addend needs its bound"),
    R("lk_bn_act_fwd_nhwc_f16x2", _BA, {"y_h": None, "y_l": None}, {"y_l": None}, "both planes or none"),
    R("lk_bn_act_fwd_nhwc_f16x2", _BA, None, {"y_bound": None}, "lk_bn_act_fwd_nhwc_f16x2: null pointer"),
    # grid = (ceil(C / 32), ceil(L / 32), S * B)
    R("lk_unsplit_transpose_f32", _UT, {"S": 5, "B": 13107}, {"S": 5, "B": 13108}, "lk_unsplit_transpose_f32: bad arguments (S * B <= 65535)"),
    R("lk_unsplit_transpose_f32", _UT, {"L": 65535 * 32}, {"L": 65535 * 32 + 1}, "lk_unsplit_transpose_f32: L too large for grid.y"),
    R("lk_unsplit_transpose_f32", _UT, {"C": (1 << 31) - 33}, {"C": (1 << 31) - 32}, "lk_unsplit_transpose_f32: C too large"),
    # the three accepted families: 64, 128 k, at most 4096 (528 tile pairs in grid.x, 32 x 32 tiles of 128)
    R("lk_gram_tn_f16x2", _G16, {"C": 4096}, {"C": 4224}, "C must be 64 or a multiple of 128"),
    R("lk_gram_tn_f16x2", _G16, {"C": 64}, {"C": 32}, "C must be 64 or a multiple of 128"),
    R("lk_gram_tn_f16x2", _G16, {"C": 128}, {"C": 192}, "C must be 64 or a multiple of 128"),
    # (100 rows of 128 columns: one K slice of one 128 x 128 tile pair)
    R("lk_gram_tn_f16x2", _G16, {"ws_bytes": 128 * 128 * 4}, {"ws_bytes": 128 * 128 * 4 - 1}, "lk_gram_tn_f16x2: workspace too small"),
    R("lk_gram_tn_f16x2", _G16, None, {"zero16": None}, "lk_gram_tn_f16x2: null pointer"),
    R("lk_conv3x3_pixpair_accumulate13_f16x2", _P13, {"Cin": 64}, {"Cin": 128}, "needs Cin == 64"),
    # 13 Cin^2 floats per pixel, 32-bit offsets: 201 x 200 pixels x 53248 = 2140569600 < 2^31 <= 202 x 200 x 53248
    R("lk_conv3x3_pixpair_accumulate13_f16x2", _P13, {"H": 201, "W": 200}, {"H": 202, "W": 200}, "needs Cin == 64"),
    R("lk_conv3x3_pixpair_accumulate13_f16x2", _P13, {"B": 0}, {"B": -1}, "lk_conv3x3_pixpair_accumulate13_f16x2: bad arguments"),
    R("lk_conv3x3_pixpair_accumulate_f16x2", _P16, {"Cin": 128}, {"Cin": 96}, "needs Cin % 64 == 0"),
    R("lk_conv3x3_pixpair_accumulate_f16x2", _P16, {"n_tiles": 0}, {"n_tiles": -1}, "lk_conv3x3_pixpair_accumulate_f16x2: bad arguments"),
)

# ---- lk_conv.hip -----------------------------------------------------------------------------------------------------------
_CV = dict(in_nsexp=1, N=8, Hi=8, Wi=8, Ci=64, Co=64, Hc=8, Wc=8, in_mul=1, Ho=8, Wo=8, out_step=1, oh0=0, ow0=0, T=9, taps=TAPS9,
           accumulate=0, config=2)
_CP = dict(in_nsexp=1, N=8, Hi=4, Wi=4, Ci=64, Co=64, Ho=4, Wo=4, in_mul=1, T=9, taps=TAPS9, config=2)
_CB = dict(in_nsexp=1, in_namax=1, N=8, Hi=8, Wi=8, Ci=64, Co=64, Ho=8, Wo=8, in_mul=1, T=9, taps=TAPS9, addend_nbound=1, act=1, config=2)
_CJ = dict(N=8, Hi=8, Wi=8, Ci=64, Co=64, Ho=8, Wo=8, T=9, taps=TAPS9, mask_is_float=0, mask_rows=512, config=2)
_S4 = [v for a in range(2) for b in range(2) for v in (0, 0, 2 * a + b, 0, a, b)]  # one tap per residue class of a stride-2 backward
_S12 = [v for t in range(12) for v in (0, 0, t, 0, (t // 2) % 2, t % 2)]
_CS = dict(in2_h=None, in2_l=None, in2_sexp=None, in2_amax=None, w2_h=None, w2_l=None, w2_sexp=None, w2_l1=None, N=8, Hi=4, Wi=4,
           Ci=64, Co=64, Ho=8, Wo=8, os=2, T=4, taps=_S4, mask_is_float=0, mask_rows=512, config=0)
_rows(
    R("lk_absmax_f32", dict(n=64, inner=4, C=4), {"inner": 1}, {"inner": 0}, "lk_absmax_f32: bad arguments"),
    R("lk_absmax_f32", dict(n=64, inner=4, C=4), {"cscale": None, "C": 0}, {"C": 0}, "lk_absmax_f32: bad arguments"),
    R("lk_copy_absmax_f32", dict(n=64), {"n": 68}, {"n": 66}, "16-byte aligned buffers, n % 4 == 0"),
    R("lk_copy_absmax_f32", dict(n=64), None, {"y": "odd"}, "16-byte aligned buffers, n % 4 == 0"),
    R("lk_split_f16x2", dict(n=64, bound_mul=1.0), {"n": 72}, {"n": 68}, "lk_split_f16x2: bad arguments (n % 8 == 0)"),
    R("lk_im2col_split_f16x2", dict(B=2, H=8, W=8, C=3, KH=3, KW=3, stride=1, pad=1, Ho=8, Wo=8, Kp=64), {"Kp": 32}, {"Kp": 24},
      "(Kp % 8 == 0, Kp >= KH * KW * C)"),
    R("lk_im2col_split_f16x2", dict(B=2, H=8, W=8, C=3, KH=3, KW=3, stride=1, pad=1, Ho=8, Wo=8, Kp=64), {"Kp": 40}, {"Kp": 36},
      "(Kp % 8 == 0, Kp >= KH * KW * C)"),
    R("lk_im2col_split_f16x2", dict(B=2, H=8, W=8, C=3, KH=3, KW=3, stride=1, pad=1, Ho=8, Wo=8, Kp=64), {"Ho": 9}, {"Ho": 10},
      "output grid outside the input"),
    # one thread per 8 columns of a row, 32-bit thread index: B Ho Wo Kp / 8 < 2^31
    R("lk_im2col_split_f16x2", dict(B=2, H=8, W=8, C=3, KH=3, KW=3, stride=1, pad=1, Ho=8, Wo=8, Kp=64), {"B": (1 << 22) - 1}, {"B": 1 << 22},
      "lk_im2col_split_f16x2: too large"),
    R("lk_im2col_split_f16x2", dict(B=2, H=8, W=8, C=8, KH=3, KW=3, stride=1, pad=1, Ho=8, Wo=8, Kp=128), {"C": 3, "x": "odd"}, {"x": "odd"},
      "x must be 16-byte aligned"),
    # grid.y = N images
    R("lk_split_images_f16x2", dict(N=4, per=64), {"N": 65535}, {"N": 65536}, "(per % 8 == 0, N < 65536)"),
    R("lk_split_images_f16x2", dict(N=4, per=64), {"per": 72}, {"per": 68}, "(per % 8 == 0, N < 65536)"),
    R("lk_conv_prep_weights_f16x2", dict(Co=8, Ci=8, taps=9, transpose=1), {"taps": 9}, {"taps": 10}, "lk_conv_prep_weights_f16x2: bad arguments"),
    R("lk_conv_prep_weights_f16x2", dict(Co=8, Ci=8, taps=9, transpose=1), {"Ci": 1}, {"Ci": 0}, "lk_conv_prep_weights_f16x2: bad arguments"),
    # the plain convolution: nine tap slots in its geometry block
    R("lk_conv_nhwc_f16x2", _CV, {"T": 9}, {"T": 10}, "Ci % 32 == 0, 1..9 taps"),
    R("lk_conv_nhwc_f16x2", _CV, {"Ci": 96}, {"Ci": 80}, "Ci % 32 == 0, 1..9 taps"),
    R("lk_conv_nhwc_f16x2", _CV, {"Ci": 32}, {"Ci": 16}, "Ci % 32 == 0, 1..9 taps"),
    # GEMM rows (N Hc Wc) are 32-bit; operand offsets 64-bit below 2^40 elements
    R("lk_conv_nhwc_f16x2", _CV, {"N": (1 << 25) - 1}, {"N": 1 << 25}, "lk_conv_nhwc_f16x2: tensor too large"),
    R("lk_conv_nhwc_f16x2", _CV, {"N": 1, "Hi": 1 << 17, "Wi": (1 << 17) - 1}, {"N": 1, "Hi": 1 << 17, "Wi": 1 << 17}, "lk_conv_nhwc_f16x2: tensor too large"),
    R("lk_conv_nhwc_f16x2", _CV, {"in_nsexp": 8}, {"in_nsexp": 7}, "in_nsexp is 1 or N"),
    R("lk_conv_nhwc_f16x2", _CV, {"config": 18, "Hi": 2, "Wi": 2, "Hc": 2, "Wc": 2, "Ho": 2, "Wo": 2},
      {"config": 18, "Hi": 3, "Wi": 3, "Hc": 3, "Wc": 3, "Ho": 3, "Wo": 3}, "position-contiguous output needs a dense grid"),
    R("lk_conv_nhwc_f16x2", _CV, {"config": 18, "accumulate": 0}, {"config": 18, "accumulate": 1}, "position-contiguous output needs a dense grid"),
    R("lk_conv_nhwc_f16x2", _CV, None, {"taps": None}, "lk_conv_nhwc_f16x2: null pointer"),
    # planes output: written in chunks of 16 positions
    R("lk_conv_nhwc_f16x2_planes", _CP, {"Hi": 4, "Wi": 4, "Ho": 4, "Wo": 4}, {"Hi": 6, "Wi": 6, "Ho": 6, "Wo": 6}, "Ho * Wo % 16 == 0"),
    R("lk_conv_nhwc_f16x2_planes", _CP, None, {"w_l1": None}, "lk_conv_nhwc_f16x2_planes: null pointer"),
    R("lk_conv_nhwc_f16x2_planes", _CP, {"T": 9}, {"T": 10}, "Ci % 32 == 0, 1..9 taps"),
    R("lk_conv_bn_act_nhwc_f16x2", _CB, {"Co": 72}, {"Co": 68}, "Co % 8 == 0, act in 0..1"),
    R("lk_conv_bn_act_nhwc_f16x2", _CB, {"act": 1}, {"act": 2}, "Co % 8 == 0, act in 0..1"),
    R("lk_conv_bn_act_nhwc_f16x2", _CB, {"in_namax": 8}, {"in_namax": 7}, "in_amax has 1 or N words"),
    R("lk_conv_bn_act_nhwc_f16x2", _CB, {"addend_nbound": 8}, {"addend_nbound": 7}, "the addend needs its bound"),
    R("lk_conv_bn_act_nhwc_f16x2", _CB, {"y_h": None, "y_l": None}, {"y_h": None}, "both planes or none"),
    R("lk_conv_bn_act_nhwc_f16x2", _CB, {"in_nsexp": 8}, {"in_nsexp": 2}, "in_nsexp is 1 or N"),
    R("lk_conv_bn_act_nhwc_f16x2", _CB, None, {"N": 1 << 20, "Co": 1 << 14}, "lk_conv_bn_act_nhwc_f16x2: tensor too large"),
    R("lk_conv_bn_act_nhwc_f16x2", _CB, None, {"y_amax": None}, "lk_conv_bn_act_nhwc_f16x2: null pointer"),
)
for _fn in ("lk_conv_nhwc_f16x2_vjp", "lk_conv_nhwc_f16x2_vjp_wc"):
    _rows(
        R(_fn, _CJ, {"Co": 72}, {"Co": 68}, "lk_conv_nhwc_f16x2_vjp: Co % 8 == 0"),
        R(_fn, _CJ, {"T": 9}, {"T": 10}, "Ci % 32 == 0, 1..9 taps"),
        R(_fn, _CJ, {"mask_rows": (1 << 31) - 1}, {"mask_rows": 1 << 31}, "lk_conv_nhwc_f16x2_vjp: mask_rows out of range"),
        R(_fn, _CJ, {"mask_rows": 1}, {"mask_rows": 0}, "lk_conv_nhwc_f16x2_vjp: mask_rows"),
        R(_fn, _CJ, {"add_h": None, "add_l": None}, {"add_l": None}, "lk_conv_nhwc_f16x2_vjp: incomplete addend"),
        R(_fn, _CJ, {"scale": None, "scale_amax": None}, {"scale_amax": None}, "scale needs its bound"),
        R(_fn, _CJ, None, {"out_amax": None}, "lk_conv_nhwc_f16x2_vjp: null pointer"),
    )
_rows(
    R("lk_conv_nhwc_f16x2_vjp_wc", _CJ, {"wc_h": None, "wc_l": None}, {"wc_l": None}, "incomplete chunk-major weights"),
    # the strided backward-data: twelve tap slots
    R("lk_conv_nhwc_f16x2_vjp_strided", _CS, {"T": 12, "taps": _S12}, {"T": 13, "taps": _S12}, "1..12 taps, Ci % 32 == 0, Co % 8 == 0"),
    R("lk_conv_nhwc_f16x2_vjp_strided", _CS, {"Co": 72}, {"Co": 68}, "1..12 taps, Ci % 32 == 0, Co % 8 == 0"),
    R("lk_conv_nhwc_f16x2_vjp_strided", _CS, {"Ci": 96}, {"Ci": 80}, "1..12 taps, Ci % 32 == 0, Co % 8 == 0"),
    R("lk_conv_nhwc_f16x2_vjp_strided", _CS, {"os": 2}, {"os": 3, "Ho": 12, "Wo": 12}, "stride 1 or 2"),
    R("lk_conv_nhwc_f16x2_vjp_strided", _CS, {"Ho": 8}, {"Ho": 9}, "stride 1 or 2, Ho = os * Hi"),
    R("lk_conv_nhwc_f16x2_vjp_strided", _CS, {"N": (1 << 25) - 1}, {"N": 1 << 25}, "lk_conv_nhwc_f16x2_vjp_strided: tensor too large"),
    R("lk_conv_nhwc_f16x2_vjp_strided", _CS, {"mask_rows": (1 << 31) - 1}, {"mask_rows": 1 << 31}, "lk_conv_nhwc_f16x2_vjp_strided: mask_rows"),
    R("lk_conv_nhwc_f16x2_vjp_strided", _CS, {"add_h": None}, {"add_sexp": None}, "lk_conv_nhwc_f16x2_vjp_strided: incomplete addend"),
    R("lk_conv_nhwc_f16x2_vjp_strided", _CS, {"scale": None, "scale_amax": None}, {"scale_amax": None}, "scale needs its bound"),
    R("lk_conv_nhwc_f16x2_vjp_strided", _CS, None, {"in2_h": 1}, "incomplete second source"),
    R("lk_conv_nhwc_f16x2_vjp_strided", _CS, None, {"taps": [0, 0, 0, 1, 0, 0] + _S4[6:]}, "lk_conv_nhwc_f16x2_vjp_strided: tap source"),
    R("lk_conv_nhwc_f16x2_vjp_strided", _CS, None, {"taps": [0, 0, 0, 0, 2, 0] + _S4[6:]}, "residue class of a tap"),
    R("lk_conv_nhwc_f16x2_vjp_strided", _CS, None, {"taps": _S4[6:12] + _S4[6:]}, "a residue class without taps"),
    R("lk_conv_nhwc_f16x2_vjp_strided", _CS, None, {"out_amax": None}, "lk_conv_nhwc_f16x2_vjp_strided: null pointer"),
)

# ---- values of the pure host functions -------------------------------------------------------------------------------------
# lk_conv_winp_eligible(N, Hi, Wi, Ci, Co, T, mask_is_float): every condition, last accepted -> 1, first refused -> 0
WINP_BASE = dict(N=8, Hi=8, Wi=8, Ci=64, Co=64, T=9, mask_is_float=0)
WINP_EDGES = [
    ("T == 9", {"T": 9}, {"T": 8}),
    ("T == 9 (above)", {"T": 9}, {"T": 10}),
    ("Wi <= 47", {"Wi": 47, "Hi": 2}, {"Wi": 48, "Hi": 2}),  # (the window's LDS rows)
    ("Hi * Wi >= 16", {"N": 32, "Hi": 4, "Wi": 4}, {"N": 64, "Hi": 3, "Wi": 5}),
    ("Ci % 32 == 0", {"Ci": 96}, {"Ci": 80}),
    ("Ci >= 32", {"Ci": 32}, {"Ci": 0}),
    ("Ci <= 4064", {"Ci": 4064}, {"Ci": 4096}),  # (KC = Ci / 16 <= 254: the 8-bit chunk fields of the tile descriptor)
    ("Ci <= 4064 (far)", {"Ci": 4064}, {"Ci": 8192}),
    ("Co >= 64", {"Co": 64}, {"Co": 0}),
    ("Co % 64 == 0", {"Co": 128}, {"Co": 96}),
    ("N Hi Wi Ci < 2^30", {"N": 262143, "Hi": 8, "Wi": 8, "Ci": 64}, {"N": 262144, "Hi": 8, "Wi": 8, "Ci": 64}),
    ("N Hi Wi Co < 2^31", {"N": 131071, "Hi": 8, "Wi": 8, "Ci": 32, "Co": 256}, {"N": 131072, "Hi": 8, "Wi": 8, "Ci": 32, "Co": 256}),
    ("N Hi Wi >= 512", {"N": 8}, {"N": 7}),
    ("byte mask", {"mask_is_float": 0}, {"mask_is_float": 1}),
]
for _name, _acc, _ref in WINP_EDGES:
    VALUE_PROBES.append((f"winp {_name} +", "lk_conv_winp_eligible", {**WINP_BASE, **_acc}))
    VALUE_PROBES.append((f"winp {_name} -", "lk_conv_winp_eligible", {**WINP_BASE, **_ref}))

# lk_gram_launch_variant(entry, n, K, L, vec4_ok, flags, out): 0 for a launch the entry point makes, negative for what it refuses
# or launches nothing for (host only: make_plan and the launch rules, no device)
GRAM_VARIANT_BASE = dict(entry=0, n=8, K=16, L=4, vec4_ok=1, flags=0)
GRAM_VARIANT_EDGES = [
    ("entry <= 4", {"entry": 4}, {"entry": 5}),
    ("entry >= 0", {"entry": 0}, {"entry": -1}),
    ("n >= 1", {"n": 1}, {"n": 0}),
    ("n < 2^30", {"n": 1 << 20}, {"n": 1 << 30}),
    ("K >= 0", {"K": 0}, {"K": -1}),
    ("NT: L >= 1", {"entry": 1, "L": 1}, {"entry": 1, "L": 0}),
    ("NT: L < 2^30", {"entry": 1, "L": (1 << 30) - 1, "K": 1}, {"entry": 1, "L": 1 << 30, "K": 1}),
    ("CONV: K < 2^31 - 64", {"entry": 2, "K": (1 << 31) - 65}, {"entry": 2, "K": (1 << 31) - 64}),
    ("XCORR: K >= 1", {"entry": 3, "K": 1}, {"entry": 3, "K": 0}),
    ("XCORR: 25 Cin < 2^24", {"entry": 4, "n": 671088}, {"entry": 4, "n": 671089}),
    ("out", {}, {"out": None}),
]
for _name, _acc, _ref in GRAM_VARIANT_EDGES:
    VALUE_PROBES.append((f"gramvar {_name} +", "lk_gram_launch_variant", {**GRAM_VARIANT_BASE, **_acc}))
    VALUE_PROBES.append((f"gramvar {_name} -", "lk_gram_launch_variant", {**GRAM_VARIANT_BASE, **_ref}))

# *_workspace_bytes at 0, 1 and the largest extent the entry point accepts: monotone, no wrap to a small number
WORKSPACE_LADDERS = {
    "lk_loss_workspace_bytes": [dict(B=0), dict(B=1), dict(B=(1 << 31) - 1)],
    "lk_gram_workspace_bytes": [dict(n=0, K=0), dict(n=1, K=1), dict(n=4608, K=1 << 20), dict(n=(1 << 15), K=(1 << 31) - 65)],
    "lk_gram_nt_workspace_bytes": [dict(nb_total=0, n=0, L=0), dict(nb_total=1, n=1, L=1), dict(nb_total=1152, n=512, L=1024)],
    "lk_conv3x3_shiftcorr_workspace_bytes": [dict(B=0, H=0, W=0, Cin=0), dict(B=1, H=2, W=2, Cin=1), dict(B=128, H=32, W=32, Cin=64),
                                             dict(B=1 << 17, H=32, W=32, Cin=512)],
    "lk_gram_tn_f16x2_workspace_bytes": [dict(R=0, C=64), dict(R=1, C=64), dict(R=1 << 20, C=128), dict(R=1 << 30, C=4096)],
    "lk_ll_ggn_workspace_bytes": [dict(B=0, C=0, D=0), dict(B=1, C=1, D=1), dict(B=1 << 20, C=1023, D=1024)],
    "lk_syevj_workspace_bytes": [dict(n=0), dict(n=1), dict(n=4608), dict(n=32768)],
    "lk_kron_logdet_workspace_bytes": [dict(n1=0), dict(n1=1), dict(n1=(1 << 30) - 1)],
    "lk_kron_logdet_blocks_workspace_bytes": [dict(total_rows=0, nblocks=0), dict(total_rows=1, nblocks=1), dict(total_rows=(1 << 30) - 1, nblocks=1 << 20)],
    "lk_quadform_shared_workspace_bytes": [dict(B=0, C=1, Do=1, Dk=1), dict(B=1, C=1, Do=1, Dk=1), dict(B=(1 << 25) - 1, C=10, Do=512, Dk=4608)],
    "lk_diag_ggn_shared_workspace_bytes": [dict(B=0, Do=1, Dk=1), dict(B=1, Do=1, Dk=1), dict(B=1 << 20, Do=1 << 15, Dk=(1 << 16) - 1)],
    "lk_quadform_shared_grid_workspace_bytes": [dict(B=0, C=1, Do=1, Dk=1, G=1), dict(B=1, C=1, Do=1, Dk=1, G=1),
                                                dict(B=(1 << 25) - 1, C=1000, Do=512, Dk=4608, G=(1 << 24) - 1)],
}
for _fn, _ladder in WORKSPACE_LADDERS.items():
    for _k, _vals in enumerate(_ladder):
        VALUE_PROBES.append((f"ws {_fn} {_k}", _fn, _vals))
VALUE_PROBES.append(("ws lk_dense_quadform_ll_workspace_bytes", "lk_dense_quadform_ll_workspace_bytes", dict(B=1 << 20, C=361, D=4096)))

# lk_conv3x3_pixpair_plan(H, W, Cin) -> (rc, tile, n_tiles, n_blocks)
PLAN_CASES = [(1, 1, 64), (2, 2, 64), (4, 4, 128), (8, 8, 192), (203, 200, 64), (204, 200, 64)]


def pixpair_blocks(H, W):
    """pixel pairs (q, q + D) a 3x3 window can see, D in the half plane {(0,0..2), (1..2,-2..2)}"""
    half = [(0, d) for d in range(3)] + [(dy, dx) for dy in (1, 2) for dx in range(-2, 3)]
    return sum(0 <= y + dy < H and 0 <= x + dx < W for y in range(H) for x in range(W) for dy, dx in half)


# ---- the child ---------------------------------------------------------------------------------------------------------------
class _Probe:
    def __init__(self):
        from laplace_amd._lib import load_library

        self.lib = load_library()
        self.protos = header_prototypes()
        self.keep = []
        raw = ctypes.create_string_buffer(1 << 16)
        self.keep.append(raw)
        self.buf = (ctypes.addressof(raw) + 63) & ~63

    def _array(self, ctype, values):
        if "int64_t" in ctype or "size_t" in ctype:
            arr = (ctypes.c_int64 * max(len(values), 1))(*values)
        else:
            arr = (ctypes.c_int32 * max(len(values), 1))(*values)
        self.keep.append(arr)
        return ctypes.addressof(arr)

    def args(self, fn, values):
        out = []
        left = dict(values)
        for kind, ctype, pname in self.protos[fn]:
            v = left.pop(pname, "__default__")
            if kind == "ptr":
                if isinstance(v, str) and v == "__default__":
                    v = self.buf
                elif v is None:
                    v = None
                elif isinstance(v, str) and v == "odd":
                    v = self.buf + 4
                elif isinstance(v, str) and v == "same":
                    v = self.buf
                elif isinstance(v, str) and v == "other":
                    v = self.buf + 4096
                elif isinstance(v, (list, tuple)) and len(v) == 2 and v[0] == "ptrs":
                    arr = (ctypes.c_void_p * max(v[1], 1))(*([self.buf] * v[1]))
                    self.keep.append(arr)
                    v = ctypes.addressof(arr)
                elif isinstance(v, (list, tuple)):
                    v = self._array(ctype, list(v))
                if pname == "stream":
                    v = None
                if ctype.replace(" ", "") == "void**":  # lk_comm_init_rank's out parameter
                    v = ctypes.cast(v, ctypes.POINTER(ctypes.c_void_p)) if v else None
                out.append(v)
            else:
                if isinstance(v, str) and v == "__default__":
                    raise KeyError(f"{fn}: no value for {pname}")
                out.append(v)
        if left:
            raise KeyError(f"{fn}: unknown parameters {sorted(left)}")
        return out

    def call(self, fn, values):
        rc = getattr(self.lib, fn)(*self.args(fn, values))
        msg = self.lib.lk_last_error()
        return int(rc), (msg.decode(errors="replace") if msg else "")


SENTINEL = ("lk_symmetrize_f32", {"n": -1})
SENTINEL_ALT = ("lk_pack_upper_f32", {"n": -1})


def _child_main():
    import torch

    def emit(obj):
        sys.stdout.write(json.dumps(obj) + "\n")
        sys.stdout.flush()

    if torch.cuda.device_count() != 0:
        emit({"fatal": "device visible"})
        return 3
    P = _Probe()
    by_fn = {}
    for i, row in enumerate(ROWS):
        by_fn.setdefault(row["fn"], []).append((i, row))
    for fn, rows in by_fn.items():
        try:
            for i, row in rows:
                for side in ("refuse", "accept"):
                    if row[side] is None:
                        continue
                    emit({"start": [i, side]})
                    # (there is no call that clears the thread's message, and some LK_ELAUNCH paths leave it alone: a refusal of
                    #  ANOTHER entry point first, so that a message of this one can only come from this call)
                    P.call(*(SENTINEL_ALT if fn == SENTINEL[0] else SENTINEL))
                    rc, msg = P.call(fn, {**row["base"], **row[side]})
                    emit({"row": i, "side": side, "rc": rc, "msg": msg})
        except Exception as exc:  # a malformed row: reported, the other entry points still run
            emit({"error": fn, "what": f"{type(exc).__name__}: {exc}"})
    # the pure host functions, by value
    vals = {}
    for key, fn, values in VALUE_PROBES:
        emit({"start": [key, "value"]})
        try:
            vals[key] = int(getattr(P.lib, fn)(*P.args(fn, values)))
        except Exception as exc:
            emit({"error": fn, "what": f"{type(exc).__name__}: {exc}"})
    emit({"values": vals})
    plan = {}
    for H, W, Cin in PLAN_CASES:
        emit({"start": [f"plan {H} {W} {Cin}", "value"]})
        out = (ctypes.c_int64 * 3)()
        a = ctypes.addressof(out)
        rc = P.lib.lk_conv3x3_pixpair_plan(H, W, Cin, a, a + 8, a + 16)
        plan[f"{H},{W},{Cin}"] = [int(rc)] + [int(v) for v in out]
    emit({"plan": plan})
    # a limit a Python caller meets in ordinary use: the predictive hands lk_unsplit_transpose_f32 C * B images (100 classes x 656
    # samples are 65600); the wrapper must turn the refusal into LaplaceHipError with the C message
    emit({"start": ["unsplit_transpose wrapper", "value"]})
    from laplace_amd._lib import HipKernels, LaplaceHipError, SplitTensor

    Kn = HipKernels(P.lib)
    Kn._stream = lambda dev: None  # (no device here: the guard returns before the stream is looked at)
    st = SplitTensor(torch.zeros(2, 65600, 1, 1, 8, dtype=torch.float16), torch.zeros(1, dtype=torch.int32))
    try:
        Kn.unsplit_transpose(st, 100, 656)
        emit({"wrapper": "no error"})
    except LaplaceHipError as exc:
        emit({"wrapper": str(exc)})
    emit({"done": True})
    return 0




# ---- the parent ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probes():
    from laplace_amd._lib import LIB_PATH

    if not os.path.exists(LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = ""
    env["ROCR_VISIBLE_DEVICES"] = ""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child"]
    proc = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    res = {"rows": {}, "errors": [], "values": {}, "plan": {}, "last": None, "done": False}
    for line in proc.stdout.splitlines():
        try:
            obj = json.loads(line)
        except ValueError:
            continue
        if "fatal" in obj:
            pytest.fail(f"the probing child refused to run: {obj['fatal']}")
        elif "start" in obj:
            res["last"] = obj["start"]
        elif "row" in obj:
            res["rows"][(obj["row"], obj["side"])] = (obj["rc"], obj["msg"])
        elif "error" in obj:
            res["errors"].append(obj)
        elif "values" in obj:
            res["values"] = obj["values"]
        elif "plan" in obj:
            res["plan"] = obj["plan"]
        elif "wrapper" in obj:
            res["wrapper"] = obj["wrapper"]
        elif "done" in obj:
            res["done"] = True
    if proc.returncode != 0 or not res["done"]:
        last = res["last"]
        where = f"row {last[0]} ({ROWS[last[0]]['fn']}, {last[1]} side)" if last and isinstance(last[0], int) else str(last)
        pytest.fail(f"the probing child ended with status {proc.returncode} (negative: a signal); last probe started: {where}\n"
                    + proc.stderr[-2000:])
    assert not res["errors"], res["errors"]
    return res


def _row_id(i):
    row = ROWS[i]
    return f"{row['fn']}[{','.join(f'{k}={v}' for k, v in row['refuse'].items())}]"[:110]


def test_table_is_well_formed():
    protos = header_prototypes()
    assert len(ROWS) >= 150
    for row in ROWS:
        assert row["fn"] in protos, row["fn"]
        names = {p[2] for p in protos[row["fn"]]}
        for side in ("base", "accept", "refuse"):
            assert row[side] is None or set(row[side]) <= names, (row["fn"], side, sorted(set(row[side]) - names))
        assert row["refuse"], row["fn"]
        assert row["fragment"]


@pytest.mark.parametrize("i", range(len(ROWS)), ids=_row_id)
def test_guard_edges(probes, i):
    """first refused -> LK_EINVAL with the entry point's own message; last accepted -> anything but a refusal"""
    row = ROWS[i]
    rc, msg = probes["rows"][(i, "refuse")]
    assert rc == LK_EINVAL, f"{row['fn']} accepted {row['refuse']} (rc={rc}: {msg})"
    assert row["fragment"] in msg, f"{row['fn']} refused {row['refuse']} with another message: {msg}"
    if row["accept"] is not None:
        rc, msg = probes["rows"][(i, "accept")]
        assert rc != LK_EINVAL, f"{row['fn']} refused the in-contract {row['accept']}: {msg}"
        assert rc in (LK_OK, LK_ELAUNCH, LK_EWORKSPACE), (rc, msg)
        sentinel = (SENTINEL_ALT if row["fn"] == SENTINEL[0] else SENTINEL)[0] + ":"
        if rc != LK_OK and not msg.startswith(sentinel):  # (the sentinel still there: the failing launch set no message)
            assert "bad arguments" not in msg and row["fragment"] not in msg, msg


# ---- the pure host functions, by value -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [e[0] for e in WINP_EDGES])
def test_winp_eligibility_edges(probes, name):
    """lk_conv_winp_eligible on both sides of each of its conditions (the accepted side also differs from the refused one
    in nothing else, so a dropped condition shows as a 1 where a 0 is expected)"""
    assert probes["values"][f"winp {name} +"] == 1, f"{name}: the last accepted shape is not eligible"
    assert probes["values"][f"winp {name} -"] == 0, f"{name}: the first refused shape is eligible"


@pytest.mark.parametrize("name", [e[0] for e in GRAM_VARIANT_EDGES])
def test_gram_launch_variant_edges(probes, name):
    """lk_gram_launch_variant answers (0) on the last shape the entry point launches and refuses (negative) the first it does not"""
    assert probes["values"][f"gramvar {name} +"] == 0, f"{name}: the last accepted shape is refused"
    assert probes["values"][f"gramvar {name} -"] < 0, f"{name}: the first refused shape is answered"


@pytest.mark.parametrize("fn", sorted(WORKSPACE_LADDERS))
def test_workspace_sizes_are_monotone(probes, fn):
    sizes = [probes["values"][f"ws {fn} {k}"] for k in range(len(WORKSPACE_LADDERS[fn]))]
    sizes = [v + (1 << 64) if v < 0 else v for v in sizes]  # (size_t read back through a signed conversion)
    # an empty problem asks for no more than the smallest one (lk_gram_tn_f16x2 sizes one tile's partials even for no rows),
    # and the smallest one asks for something
    assert 0 <= sizes[0] <= sizes[1], f"{fn}: {sizes[0]} bytes at extent 0, {sizes[1]} at extent 1"
    assert sizes[1] > 0, f"{fn}: no workspace at extent 1"
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), f"{fn} is not monotone along {WORKSPACE_LADDERS[fn]}: {sizes}"
    assert sizes[-1] < 1 << 62, sizes  # no wrap, and nothing like (size_t)-1
    assert sizes[-1] >= 1 << 10, f"{fn}: the largest accepted extent asks for {sizes[-1]} bytes"


def test_workspace_sizes_known_values(probes):
    v = probes["values"]
    assert v["ws lk_loss_workspace_bytes 2"] == (((1 << 31) - 1 + 3) // 4 + 1) * 4
    assert v["ws lk_syevj_workspace_bytes 3"] >= 4 * 32768 * 32768 * 4
    assert v["ws lk_kron_logdet_workspace_bytes 2"] == ((1 << 30) - 1) * 8
    assert v["ws lk_dense_quadform_ll_workspace_bytes"] == 0  # (the kernel needs none)
    # lk_gram_tn_f16x2: 100 rows of 128 columns are one split of one 128 x 128 tile pair ... R = 2^30 at C = 4096
    assert v["ws lk_gram_tn_f16x2_workspace_bytes 3"] >= 528 * 128 * 128 * 4


def test_pixpair_plan_values(probes):
    for H, W, Cin in PLAN_CASES:
        rc, tile, n_tiles, n_blocks = probes["plan"][f"{H},{W},{Cin}"]
        nb = pixpair_blocks(H, W)
        if nb * Cin * Cin < 1 << 31:
            T = 128 if Cin % 128 == 0 else 64
            assert (rc, tile, n_blocks, n_tiles) == (LK_OK, T, nb, nb * (Cin // T) ** 2), (H, W, Cin)
        else:
            assert rc == LK_EINVAL, (H, W, Cin)
    assert probes["plan"]["203,200,64"][0] == LK_OK and probes["plan"]["204,200,64"][0] == LK_EINVAL


def test_a_refusal_reaches_the_python_caller_as_laplace_hip_error(probes):
    """HipKernels.unsplit_transpose with S * B = 100 * 656 images (laplace_amd/backend.py hands it classes x predictive batch)"""
    assert "rc=-1" in probes["wrapper"] and "lk_unsplit_transpose_f32: bad arguments (S * B <= 65535)" in probes["wrapper"]


# ---- completeness: every guarded entry point owns a first-refused row --------------------------------------------------------
def _function_bodies(text):
    """name -> body of every function definition at namespace / file level of a source file (brace matching)"""
    out = {}
    for m in re.finditer(r"^(?:extern \"C\" |static |inline |template\s*<[^>]*>\s*)*[\w:<>\*&\s]+?\b(\w+)\s*\(([^;{}]*)\)\s*\{", text, flags=re.M):
        depth, j = 1, m.end()
        while depth and j < len(text):
            depth += {"{": 1, "}": -1}.get(text[j], 0)
            j += 1
        out.setdefault(m.group(1), (m.group(0).lstrip().startswith('extern "C"'), text[m.end():j]))
    return out


def guarded_entry_points():
    csrc = os.path.join(ROOT, "laplace_amd", "csrc")
    guarded = set()
    for fname in sorted(os.listdir(csrc)):
        if not fname.endswith((".hip", ".cpp")):
            continue
        text = open(os.path.join(csrc, fname)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        bodies = _function_bodies(text)
        has_guard = lambda b: "LK_REQUIRE" in b or re.search(r"return\s+LK_EINVAL", b) is not None  # noqa: E731
        for name, (is_c, body) in bodies.items():
            if not (is_c and name.startswith("lk_")):
                continue
            helpers = [h for h in re.findall(r"\b(launch_\w+|\w+_impl|conv_dispatch)\s*\(", body) if h in bodies]
            if has_guard(body) or any(has_guard(bodies[h][1]) for h in helpers):
                guarded.add(name)
    return guarded


def test_every_guarded_entry_point_owns_a_refused_row():
    guarded = guarded_entry_points()
    assert len(guarded) >= 60, sorted(guarded)  # the parser found the library (76 entry points, most of them guarded)
    have = {row["fn"] for row in ROWS if row["refuse"]}
    missing = sorted(guarded - have)
    assert not missing, f"guarded entry points without a first-refused row: {missing}"


if __name__ == "__main__" and "--child" in sys.argv:
    sys.exit(_child_main())
