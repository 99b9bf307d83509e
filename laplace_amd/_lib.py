"""ctypes binding of ``csrc/liblaplace_hip.so`` (the C ABI declared in include/laplace_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every hot operation is one of
our HIP entry points.  There is NO fallback: if the shared library is missing, or a tensor is
not an fp32 contiguous tensor on a ROCm device, the call raises.

The tensor-level API lives on :class:`HipKernels`; ``get_kernels()`` returns the process-wide
instance.  Tests that exercise *host logic* on a CPU-only box install a stand-in through
``set_kernels_for_testing`` (see tests/emulated_kernels.py) — the product never does.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# (LK_LIB: another build of the same library, e.g. csrc/liblaplace_hip_dev.so with the kernels' development switches)
LIB_PATH = os.environ.get("LK_LIB") or os.path.join(_HERE, "csrc", "liblaplace_hip.so")

LK_GRAM_UPPER_ONLY = 1
LK_GRAM_SLABS_PERSIST = 2

_c_f32p = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int
_f32 = ctypes.c_float
_sz = ctypes.c_size_t
_vp = ctypes.c_void_p
_u32 = ctypes.c_uint

# name -> (restype, argtypes); the single source of truth shared with tests/test_capi_symbols.py
SIGNATURES = {
    "lk_version": (_int, []),
    "lk_last_error": (ctypes.c_char_p, []),
    "lk_im2col_split_f16x2": (_int, [_vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
    "lk_comm_unique_id": (_int, [_vp]),
    "lk_comm_init_rank": (_int, [ctypes.POINTER(ctypes.c_void_p), _int, _vp, _int]),
    "lk_comm_destroy": (_int, [_vp]),
    "lk_allreduce_sum_f32": (_int, [_vp, _vp, _i64, _vp]),
    "lk_loss_workspace_bytes": (_sz, [_i64]),
    "lk_softmax_hess_sqrt_f32": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "lk_softmax_hess_chol_f32": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "lk_sq_err_sum_f32": (_int, [_vp, _vp, _i64, _f32, _vp, _vp, _vp]),
    "lk_gram_workspace_bytes": (_sz, [_i64, _i64]),
    "lk_gram_nt_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "lk_gram_launch_variant": (_int, [_int, _i64, _i64, _i64, _int, _u32, _vp]),
    "lk_gram_slabs_reduce_f32": (_int, [_vp, _sz, _i64, _i64, _f32, _vp, _u32, _vp]),
    "lk_gram_tn_f32": (_int, [_vp, _i64, _i64, _i64, _f32, _vp, _u32, _vp, _sz, _vp]),
    "lk_gram_nt_f32": (_int, [_vp, _i64, _i64, _i64, _f32, _vp, _u32, _vp, _sz, _vp]),
    "lk_gram_nt_seg_f32": (_int, [_vp, _i64, _i64, _i64, _i64, _f32, _vp, _u32, _vp, _sz, _vp]),
    "lk_gram_conv_nhwc_f32": (
        _int,
        [_vp, _i64, _i64, _i64, _i64, _int, _int, _int, _int, _int, _int, _int, _int, _f32, _vp, _u32, _vp, _sz, _vp],
    ),
    "lk_conv3x3_shiftcorr_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "lk_conv3x3_shiftcorr_f32": (_int, [_vp, _i64, _i64, _i64, _i64, _f32, _vp, _vp, _sz, _vp]),
    "lk_conv3x3_pixgram_assemble_f32": (_int, [_vp, _i64, _i64, _i64, _f32, _vp, _vp]),
    "lk_conv3x3_pixpair_plan": (_int, [_i64, _i64, _i64, _vp, _vp, _vp]),
    "lk_conv3x3_pixpair_tables": (_int, [_i64, _i64, _i64, _vp, _vp]),
    "lk_conv3x3_pixpair_accumulate_f32": (_int, [_vp, _i64, _i64, _i64, _i64, _f32, _vp, _vp, _i64, _vp]),
    "lk_conv3x3_pixpair_accumulate_f16x2": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32, _vp, _vp, _i64, _vp, _vp]),
    "lk_conv3x3_pixpair_accumulate13_f16x2": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32, _vp, _vp, _vp, _vp]),
    "lk_conv3x3_pixpair_assemble_f32": (_int, [_vp, _vp, _i64, _i64, _i64, _f32, _vp, _vp]),
    "lk_conv3x3_pixpair_assemble2_f32": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _f32, _vp, _int, _vp]),
    "lk_nchw_to_nhwc_f32": (_int, [_vp, _i64, _i64, _i64, _vp, _vp]),
    "lk_absmax_f32": (_int, [_vp, _i64, _vp, _i64, _i64, _vp, _vp]),
    "lk_copy_absmax_f32": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "lk_split_f16x2": (_int, [_vp, _i64, _vp, _f32, _vp, _vp, _vp, _vp]),
    "lk_split_images_f16x2": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
    "lk_conv_prep_weights_f16x2": (_int, [_vp, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp, _vp]),
    "lk_conv_nhwc_f16x2": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64,
                                  _i64, _i64, _i64, _i64, _vp, _vp, _vp, _int, _vp, _int, _vp]),
    "lk_conv_nhwc_f16x2_planes": (_int, [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64,
                                         _i64, _vp, _vp, _vp, _vp, _vp, _int, _vp]),
    "lk_conv_bn_act_nhwc_f16x2": (_int, [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _i64,
                                         _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _vp,
                                         _vp, _vp, _int, _vp]),
    "lk_conv_nhwc_f16x2_vjp": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64,
                                      _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _i64, _vp, _vp, _vp, _vp, _vp,
                                      _vp, _int, _vp]),
    "lk_conv_winp_eligible": (_int, [_i64, _i64, _i64, _i64, _i64, _i64, _int]),
    "lk_conv_nhwc_f16x2_vjp_wc": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64,
                                         _i64, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _int,
                                         _vp]),
    "lk_conv_nhwc_f16x2_vjp_strided": (_int, [_vp] * 16 + [_i64] * 9 + [_vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _i64, _vp, _vp, _vp,
                                               _vp, _vp, _vp, _int, _vp]),
    "lk_vjp_nhwc_split_f16x2": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    "lk_bn_act_fwd_nhwc_f16x2": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _i64, _i64, _i64, _vp, _vp,
                                        _vp, _vp, _vp, _vp, _vp, _vp]),
    "lk_unsplit_transpose_f32": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    "lk_gram_tn_f16x2_workspace_bytes": (_sz, [_i64, _i64]),
    "lk_gram_tn_f16x2": (_int, [_vp, _vp, _vp, _i64, _i64, _f32, _vp, _vp, _vp, _sz, _vp]),
    "lk_gemm_f32": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _int, _int, _f32,
                           _int, _vp]),
    "lk_kron_pow_f32": (_int, [_vp, _i64, _vp, _i64, _vp, _f32, _int, _vp, _vp]),
    "lk_pack_upper_f32": (_int, [_vp, _i64, _vp, _vp]),
    "lk_unpack_upper_f32": (_int, [_vp, _i64, _vp, _vp]),
    "lk_symmetrize_f32": (_int, [_vp, _i64, _vp]),
    "lk_permute_sym_f32": (_int, [_vp, _i64, _i64, _vp, _int, _vp]),
    "lk_finalize_factors_f32": (_int, [_i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lk_diag_ggn_linear_f32": (_int, [_vp, _vp, _i64, _i64, _i64, _i64, _f32, _vp, _vp, _vp]),
    "lk_jac_linear_f32": (_int, [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp]),
    "lk_jac_conv_f32": (
        _int,
        [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _int, _int, _int, _int, _int, _int, _int, _int, _vp, _i64, _i64, _i64, _vp],
    ),
    "lk_jac_gconv_f32": (
        _int,
        [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _int, _int, _int, _int, _int, _int, _int, _int, _vp, _i64, _i64, _i64,
         _vp],
    ),
    "lk_jac_embed_f32": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _vp]),
    "lk_diag_embed_f32": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _vp, _vp]),
    "lk_diag_quadform_embed_f32": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp]),
    "lk_embed_variant": (_int, [_i64, _i64, _i64, _i64, _int]),
    "lk_sq_colsum_f32": (_int, [_vp, _i64, _i64, _i64, _i64, _f32, _vp, _vp]),
    "lk_jac_norm_affine_f32": (_int, [_vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _i64, _i64, _i64, _vp]),
    "lk_norm_fwd_f32": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _f32, _vp, _vp, _vp, _vp]),
    "lk_norm_vjp_f32": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _int, _vp, _vp, _vp]),
    "lk_norm_sweep_variant": (_int, [_i64, _i64, _i64, _i64, _i64, _int, _int]),
    "lk_rmsnorm_fwd_f32": (_int, [_vp, _vp, _i64, _i64, _f32, _vp, _vp, _vp]),
    "lk_rmsnorm_vjp_f32": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "lk_rmsnorm_variant": (_int, [_i64, _i64, _i64, _int]),
    "lk_attn_fwd_f32": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _f32, _int, _vp, _vp, _vp]),
    "lk_attn_vjp_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _i64]),
    "lk_attn_vjp_f32": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _int, _f32, _int, _vp, _vp, _vp, _vp,
                               _sz, _vp]),
    "lk_attn_variant": (_int, [_i64, _i64, _i64, _i64, _i64, _int, _int]),
    "lk_attn_fwd_strided_f32": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _f32, _int, _vp, _vp, _vp]),
    "lk_attn_vjp_strided_f32": (_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _f32, _int, _vp, _vp, _vp,
                                       _i64, _vp, _sz, _vp]),
    "lk_pool_fwd_nhwc_f32": (_int, [_int, _vp, _i64, _i64, _i64, _i64] + [_int] * 8 + [_vp, _vp, _vp]),
    "lk_pool_vjp_nhwc_f32": (_int, [_int, _vp, _vp, _i64, _i64, _i64, _i64, _i64] + [_int] * 8 + [_vp, _vp, _vp]),
    "lk_pool_variant": (_int, [_int, _i64, _i64, _i64, _i64, _i64] + [_int] * 7),
    "lk_cat_fwd_nhwc_f32": (_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp]),
    "lk_cat_vjp_nhwc_f32": (_int, [_int, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp]),
    "lk_cat_variant": (_int, [_int, _int, _i64, _i64, _i64, _i64, _int]),
    "lk_slice_fwd_f32": (_int, [_vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    "lk_slice_vjp_f32": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp]),
    "lk_slice_variant": (_int, [_int, _int, _vp, _vp, _i64, _i64, _int]),
    "lk_maxred_fwd_f32": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    "lk_maxred_vjp_f32": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    "lk_reduce_variant": (_int, [_int, _i64, _i64, _i64, _i64, _int, _int]),
    "lk_resample_vjp_f32": (_int, [_vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lk_resample_variant": (_int, [_i64, _i64, _i64, _i64, _i64, _int, _int, _int]),
    "lk_mul_vjp_f32": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _int, _vp, _vp, _vp]),
    "lk_mul_variant": (_int, [_i64, _i64, _i64, _int, _int, _int, _int]),
    "lk_gate_reduce_nhwc_f32": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    "lk_gate_vjp_nhwc_f32": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp]),
    "lk_gate_variant": (_int, [_int, _i64, _i64, _i64, _i64, _int]),
    "lk_softmax_vjp_f32": (_int, [_vp, _vp, _i64, _i64, _i64, _int, _vp, _vp]),
    "lk_softmax_vjp_variant": (_int, [_i64, _i64, _i64, _int, _int]),
    "lk_matmul_vjp_f32": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp]),
    "lk_matmul_vjp_variant": (_int, [_i64, _i64, _i64, _i64, _i64, _int, _int]),
    "lk_dwconv_fwd_nhwc_f32": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64] + [_int] * 6 + [_vp, _vp]),
    "lk_dwconv_bwd_nhwc_f16x2": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64] + [_int] * 6 + [_vp, _vp, _vp]),
    "lk_dwconv_variant": (_int, [_i64, _i64, _i64, _i64, _i64] + [_int] * 7),
    "lk_jac_norm_affine_nhwc_f16x2": (_int, [_vp] * 6 + [_i64] * 4 + [_vp, _i64, _i64, _i64, _vp]),
    "lk_normtap_variant": (_int, [_i64, _i64, _i64, _i64, _int, _int]),
    "lk_bn_act_fwd_f32": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _int, _vp, _vp, _vp]),
    "lk_vjp_scale_mask_f32": (_int, [_vp, _vp, _vp, _int, _vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    "lk_ll_ggn_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "lk_ll_ggn_full_f32": (_int, [_vp, _vp, _i64, _i64, _i64, _int, _f32, _vp, _vp, _sz, _vp]),
    "lk_syevj_workspace_bytes": (_sz, [_i64]),
    "lk_syevj_f32": (_int, [_vp, _i64, _vp, _vp, _int, _int, _vp, _vp, _sz, _vp]),
    "lk_syevj_batched_f32": (_int, [_i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _vp, _i64]),
    "lk_kron_logdet_workspace_bytes": (_sz, [_i64]),
    "lk_kron_logdet_f32": (_int, [_vp, _i64, _vp, _i64, _vp, _int, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "lk_kron_logdet_blocks_workspace_bytes": (_sz, [_i64, _i64]),
    "lk_kron_logdet_blocks_f32": (_int, [_i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "lk_kron_quadform_linear_f32": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
    "lk_diag_quadform_linear_f32": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    "lk_quadform_shared_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "lk_kron_quadform_shared_planes_f16x2": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64,
                                                    _vp, _vp, _vp, _sz, _vp]),
    "lk_kron_quadform_shared_seedmajor_f32": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _sz, _vp]),
    "lk_kron_quadform_shared_f32": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _sz, _vp]),
    "lk_diag_quadform_shared_f32": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _sz, _vp]),
    "lk_diag_ggn_shared_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "lk_diag_ggn_shared_f32": (_int, [_vp, _vp, _i64, _i64, _i64, _i64, _i64, ctypes.c_float, _vp, _vp, _sz, _vp]),
    "lk_diag_quadform_js_f32": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp]),
    "lk_dense_quadform_ll_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "lk_jac_last_layer_f32": (_int, [_vp, _i64, _i64, _i64, _int, _vp, _vp]),
    "lk_dense_quadform_ll_f32": (_int, [_vp, _vp, _i64, _i64, _i64, _int, _vp, _vp, _sz, _vp]),
    "lk_quadform_linear_grid_f32": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _int, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    "lk_quadform_shared_grid_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _i64]),
    "lk_quadform_shared_grid_f32": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _int, _i64, _i64, _i64, _i64, _i64, _int, _vp, _vp, _sz,
                                           _vp]),
    "lk_quadform_shared_variant": (_int, [_int, _i64, _i64, _i64, _i64, _i64, _int]),
    "lk_conv_launch_variant": (_int, [_int] + [_i64] * 14 + [ctypes.POINTER(ctypes.c_int), _i64, _int, _int, _int,
                                      ctypes.POINTER(ctypes.c_int)]),
    "lk_conv_strided_launch_variant": (_int, [_i64] * 9 + [ctypes.POINTER(ctypes.c_int), _int, ctypes.POINTER(ctypes.c_int)]),
    "lk_probit_nll_grid_f32": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp]),
    "lk_spectral_workspace_bytes": (_sz, [_int, _i64, _i64, _i64, _i64]),
    "lk_spectral_quadform_ll_f32": (_int, [_vp, _vp, _vp, _f32, _vp, _i64, _i64, _i64, _int, _vp, _vp, _sz, _vp]),
    "lk_spectral_grid_ll_f32": (_int, [_vp, _vp, _vp, _f32, _vp, _i64, _i64, _i64, _i64, _int, _vp, _vp, _sz, _vp]),
    "lk_spectral_quadform_f32": (_int, [_vp, _vp, _f32, _vp, _i64, _i64, _i64, _vp, _vp, _sz, _vp]),
    "lk_spectral_grid_f32": (_int, [_vp, _vp, _f32, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _sz, _vp]),
    "lk_spectral_variant": (_int, [_int, _i64, _i64, _i64, _i64, _int]),
}


class LaplaceHipError(RuntimeError):
    pass


class SplitTensor:
    """Two fp16 planes ``planes[0] + planes[1] ~= x * 2**sexp`` of a tensor (include/laplace_hip.h, lk_split_f16x2).
    ``sexp``: int32 ``[1]`` — one scale for the tensor (the reverse sweep's cotangents) — or ``[N]``, one per image of the
    leading dimension (the forward's activations: lk_split_images_f16x2, lk_bn_act_fwd_nhwc_f16x2)."""

    __slots__ = ("planes", "sexp", "amax", "chunked")

    def __init__(self, planes: torch.Tensor, sexp: torch.Tensor, amax: torch.Tensor | None = None, chunked: bool = False):
        #: ``amax``: device word(s) with the MEASURED max|x| (per scale entry) when the producer provides them (fused
        #: convolution epilogue, per-image forward); consumers that need a bound otherwise use 2**(15 - sexp)
        #: ``chunked``: the planes of a position-contiguous ``[N, D, L]`` tensor stored CHUNK-major, ``planes [2, N, L / 16, D, 16]``
        #: (lk_conv_nhwc_f16x2_planes -> lk_kron_quadform_shared_planes_f16x2: a staged block of 16 positions x 32 rows is one
        #: contiguous kilobyte); ``shape`` and ``float()`` stay the logical ``[N, D, L]``
        self.planes, self.sexp, self.amax, self.chunked = planes, sexp, amax, bool(chunked)

    @property
    def shape(self):
        if self.chunked:
            _, N, nch, D, w = self.planes.shape
            return torch.Size((N, D, nch * w))
        return self.planes.shape[1:]

    def chunk_major(self) -> "SplitTensor":
        """the same ``[N, D, L]`` tensor with chunk-major planes (a copy unless it already is; ``L % 16 == 0``)"""
        if self.chunked:
            return self
        _, N, D, L = self.planes.shape
        pl = self.planes.view(2, N, D, L // 16, 16).permute(0, 1, 3, 2, 4).contiguous()
        return SplitTensor(pl, self.sexp, self.amax, chunked=True)

    @property
    def per_image(self) -> bool:
        return self.sexp.numel() > 1

    def float(self) -> torch.Tensor:
        """fp32 reconstruction (tests / fallbacks)"""
        s = self.sexp.float()
        pl = self.planes
        if self.chunked:
            _, N, nch, D, w = pl.shape
            pl = pl.permute(0, 1, 3, 2, 4).reshape(2, N, D, nch * w)
        if s.numel() > 1:
            s = s.reshape(-1, *([1] * (pl.dim() - 2)))
        return (pl[0].float() + pl[1].float()) * torch.exp2(-s)


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise LaplaceHipError(
            f"HIP extension not built: {path} is missing. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C laplace_amd/csrc`). There is no CPU fallback."
        )
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is missing
        fn.restype = res
        fn.argtypes = args
    return lib


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda idx: torch.cuda.current_stream(idx).cuda_stream)


def _ptr(t: Optional[torch.Tensor]):
    """device address for a ``c_void_p`` argument (a plain int: ctypes converts it; ~1000 of these per fit step)"""
    return None if t is None else t.data_ptr()


def _check(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise LaplaceHipError(f"{name}: expected a tensor, got {type(t)}")
    if not t.is_cuda:
        raise LaplaceHipError(f"{name}: tensor is on {t.device}; the HIP backend needs a ROCm device (no CPU path)")
    if t.dtype != dtype:
        raise LaplaceHipError(f"{name}: dtype {t.dtype} not supported (need {dtype})")
    if not t.is_contiguous():
        raise LaplaceHipError(f"{name}: tensor must be contiguous")
    return t


def _one_scale(x: "SplitTensor", what: str) -> "SplitTensor":
    """consumers whose GEMM rows or reductions run ACROSS images (the reverse sweep's kernels) take one scale per tensor"""
    if x is not None and x.sexp.numel() != 1:
        raise LaplaceHipError(f"{what}: a split tensor with one scale per image is a forward operand (lk_conv_nhwc_f16x2); "
                              "this kernel reduces across images and needs one scale for the tensor")
    return x


def _split_half(x: "SplitTensor", what: str, name: str, chunked: Optional[str]):
    """``(hi, lo, sexp)`` addresses of a one-scale split operand.  ``chunked``: what a chunk-major one is to the caller, for its
    refusal (``None``: the caller refuses it itself, with its shape)"""
    _one_scale(x, what)
    if chunked is not None and x.chunked:
        raise LaplaceHipError(f"{what}: a chunk-major split tensor is {chunked}")
    _check(x.planes, f"{name}.planes", torch.float16)
    _check(x.sexp, f"{name}.sexp", torch.int32)
    return x.planes[0].data_ptr(), x.planes[1].data_ptr(), x.sexp.data_ptr()


def _split_operand(x, what: str, name: str, chunked: str):
    """``(f32, hi, lo, sexp), shape, device`` of an operand that is an fp32 tensor or a one-scale :class:`SplitTensor` read as it
    lies: the addresses of the form it has, ``None`` for the other"""
    if isinstance(x, SplitTensor):
        return (None, *_split_half(x, what, name, chunked)), x.shape, x.planes.device
    _check(x, name)
    return (x.data_ptr(), None, None, None), x.shape, x.device


def _amax_word(amax, what: str):
    if amax is not None and (amax.numel() != 1 or amax.element_size() != 4):
        raise LaplaceHipError(f"{what}: amax is one 32-bit device word")


def is_channels_last(x) -> bool:
    """logical [B, C, H, W] tensor whose memory is dense NHWC (and not also dense NCHW)"""
    return torch.is_tensor(x) and x.dim() == 4 and not x.is_contiguous() and x.permute(0, 2, 3, 1).is_contiguous()


def keep_layout(x):
    """``x`` as the kernels' wrappers want it: dense NCHW, or left alone when it is dense NHWC (no transposing copy)"""
    return x if is_channels_last(x) else x.contiguous()


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


class HipKernels:
    """Tensor-level wrappers; every method enqueues on torch's current stream and returns at once."""

    name = "hip"
    conv_config = 2  # lk_conv_nhwc_f16x2: bit 0 = 64-deep K chunks, bit 1 = never use the patch form (default: measured faster inside
    # the step, 12.2 vs 13.0 ms), bit 2 = 16-deep chunks in four LDS stages
    softmax_chol_max_c = 2000  # LK_SOFTMAX_CHOL_MAX_C (include/laplace_hip.h): wider outputs use the symmetric root

    def __init__(self, lib: Optional[ctypes.CDLL] = None):
        self.lib = lib if lib is not None else load_library()
        self._ws: dict = {}
        # optional per-launch timing (bench.py's roofline leg): name -> list of (start_evt, end_evt, work)
        self.profile: Optional[dict] = None
        # 3x3/stride-1 conv A factors through the shift-correlation identity (lk_conv3x3_shiftcorr_f32)
        self.use_shiftcorr = True

    def _timed(self, name: str, work: float, dev, call, nbytes: float | None = None):
        """Run ``call()``; when profiling is on, bracket it with HIP events on the launch stream.  ``work``: algorithmic flop
        (matrix families) or bytes (streaming families) of the launch; ``nbytes``: algorithmic HBM bytes of a matrix-family
        launch — every operand read once, every result written once (what bench.py prices its measured traffic against)."""
        if self.profile is None:
            return call()
        st = torch.cuda.current_stream(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        rc = call()
        e1.record(st)
        self.profile.setdefault(name, []).append((e0, e1, work, nbytes))
        return rc

    # ---- plumbing -----------------------------------------------------------------------------
    def _stream(self, dev) -> int:
        """raw handle of torch's current stream on ``dev`` (the C call behind ``torch.cuda.current_stream(dev).cuda_stream``
        without the Stream object and its device look-ups: ~170 of these per fit step)"""
        idx = dev.index if isinstance(dev, torch.device) else torch.device(dev).index
        return _raw_stream(torch.cuda.current_device() if idx is None else idx)

    def _workspace(self, nbytes: int, dev) -> torch.Tensor:
        key = (dev.index, self._stream(dev))
        buf = self._ws.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=dev)
            self._ws[key] = buf
        return buf

    def _rc(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.lk_last_error()
            raise LaplaceHipError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")

    # ---- likelihood ---------------------------------------------------------------------------
    def softmax_hess_sqrt(self, f, y=None, loss_accum=None, cholesky=False):
        """Columns of a root of ``diag(p) - p p^T`` as backward seeds ``[S, B, C]``: the symmetric root
        (``S = C``) or, with ``cholesky=True``, the rank-revealing Cholesky root (``S = C - 1``)."""
        _check(f, "f")
        B, C = f.shape
        ws = None
        if y is not None and loss_accum is not None:
            ws = torch.empty(max(1024, (B + 3) // 4 + 1), dtype=torch.float32, device=f.device)  # per-block partials
        if cholesky and 2 <= C <= self.softmax_chol_max_c:
            S = torch.empty(C - 1, B, C, dtype=torch.float32, device=f.device)
            if y is not None:
                _check(y, "y", torch.int64)
            if loss_accum is not None:
                _check(loss_accum, "loss_accum")
            self._rc(
                self.lib.lk_softmax_hess_chol_f32(_ptr(f), _ptr(y), B, C, _ptr(S), _ptr(loss_accum), _ptr(ws),
                                                  self._stream(f.device)),
                "lk_softmax_hess_chol_f32",
            )
            return S
        S = torch.empty(C, B, C, dtype=torch.float32, device=f.device)
        if y is not None:
            _check(y, "y", torch.int64)
        if loss_accum is not None:
            _check(loss_accum, "loss_accum")
        self._rc(
            self.lib.lk_softmax_hess_sqrt_f32(_ptr(f), _ptr(y), B, C, _ptr(S), _ptr(loss_accum), _ptr(ws),
                                              self._stream(f.device)),
            "lk_softmax_hess_sqrt_f32",
        )
        return S

    def sq_err_sum(self, f, y, scale, loss_accum):
        _check(f, "f"), _check(y, "y"), _check(loss_accum, "loss_accum")
        if f.shape != y.shape:
            raise LaplaceHipError(f"sq_err_sum: shape mismatch {tuple(f.shape)} vs {tuple(y.shape)}")
        self._rc(
            self.lib.lk_sq_err_sum_f32(_ptr(f), _ptr(y), f.numel(), float(scale), _ptr(loss_accum),
                                       _ptr(torch.empty(1024, dtype=torch.float32, device=f.device)),
                                       self._stream(f.device)),
            "lk_sq_err_sum_f32",
        )

    # ---- Gram family --------------------------------------------------------------------------
    def gram_tn(self, X, alpha, out, upper_only=False):
        _check(X, "X"), _check(out, "out")
        K, n = X.shape
        assert out.shape == (n, n)
        nb = self.lib.lk_gram_workspace_bytes(n, max(K, 1))
        ws = self._workspace(nb, X.device)
        self._rc(
            self._timed("gram_tn", float(K) * n * (n + 1), X.device, lambda: self.lib.lk_gram_tn_f32(
                _ptr(X), K, n, n, float(alpha), _ptr(out), LK_GRAM_UPPER_ONLY if upper_only else 0, _ptr(ws), ws.numel(),
                self._stream(X.device))),
            "lk_gram_tn_f32",
        )
        return out

    #: ``entry`` of :meth:`gram_launch_variant` (LK_GRAM_* of include/laplace_hip.h)
    GRAM_TN, GRAM_NT, GRAM_CONV, GRAM_XCORR_FULL, GRAM_XCORR_STRIPS = range(5)
    GRAM_UPPER_ONLY, GRAM_SLABS_PERSIST = 1, 2
    _GRAM_MODES = {0: "TN", 1: "NT", 2: "CONV", 3: "XCORR", 5: "NTB"}
    _GRAM_CFGS = ("SMALL", "BIG", "WIDE")
    _GRAM_EPILOGUES = ("slabs", "direct", "persist")

    def gram_launch_variant(self, entry, n, K, L=0, vec4_ok=True, flags=0):
        """lk_gram_launch_variant: loader, VEC, tile configuration, split of K, epilogue and reduction a launch of the fp32 Gram
        engine takes (host only, no device), or ``None`` for what the entry point refuses or launches nothing for.  ``vec4_ok``:
        what of the 16-byte-load rule the arguments do not show (pointer alignment; TN: ``ldx % 4 == 0``; CONV: ``Cin % 4 == 0``)."""
        o = (ctypes.c_int * 12)()
        rc = self.lib.lk_gram_launch_variant(int(entry), int(n), int(K), int(L), int(bool(vec4_ok)), int(flags), o)
        if rc < 0:
            return None
        return {"mode": self._GRAM_MODES[o[0]], "vec": o[1], "cfg": self._GRAM_CFGS[o[2]], "T": o[3], "BK": o[4], "npairs": o[5],
                "nchunks": o[6], "nsplit": o[7], "chunks_per_split": o[8], "epilogue": self._GRAM_EPILOGUES[o[9]],
                "two_level": bool(o[10]), "rpw": o[11]}

    def gram_nt_slab_bytes(self, nb_total, n, L) -> int:
        return int(self.lib.lk_gram_nt_workspace_bytes(int(nb_total), int(n), int(L)))

    def gram_slabs_reduce(self, slabs, n, L, alpha, out, upper_only=False):
        """``out += alpha * sum(persistent slabs)`` — the one-off reduction of ``gram_nt(..., persist=slabs)``."""
        _check(out, "out")
        self._rc(self.lib.lk_gram_slabs_reduce_f32(_ptr(slabs), slabs.numel(), int(n), int(L), float(alpha), _ptr(out),
                                                   LK_GRAM_UPPER_ONLY if upper_only else 0, self._stream(out.device)),
                 "lk_gram_slabs_reduce_f32")
        return out

    def gram_nt(self, X, alpha, out, upper_only=False, persist=None):
        """``out += alpha * sum_b X_b X_b^T``; ``X`` is ``[nb, n, L]`` or a list of up to 16 such tensors
        (per-seed gradients, consumed in place through a pointer table).  ``persist``: a zero-initialised uint8 buffer
        of at least ``gram_nt_slab_bytes`` that accumulates the split-K partial tiles across calls instead of ``out``
        (reduce once with :meth:`gram_slabs_reduce`; ``alpha`` is then applied there)."""
        segs = list(X) if isinstance(X, (list, tuple)) else [X]
        for t in segs:
            _check(t, "X")
        _check(out, "out")
        nbat, n, L = segs[0].shape
        assert all(t.shape == segs[0].shape for t in segs) and out.shape == (n, n)
        if len(segs) > 16:
            segs = [torch.cat(segs)]
            nbat = segs[0].shape[0]
        nb = self.lib.lk_gram_nt_workspace_bytes(len(segs) * nbat, n, L)
        dev = segs[0].device
        flags = LK_GRAM_UPPER_ONLY if upper_only else 0
        if persist is not None:
            if persist.numel() < nb:
                raise LaplaceHipError("gram_nt: persistent slab buffer too small")
            ws, flags = persist, flags | LK_GRAM_SLABS_PERSIST
        else:
            ws = self._workspace(nb, dev)
        ptrs = (ctypes.c_void_p * len(segs))(*[t.data_ptr() for t in segs])
        self._rc(
            self._timed("gram_nt", float(len(segs) * nbat * L) * n * (n + 1), dev, lambda: self.lib.lk_gram_nt_seg_f32(
                ptrs, len(segs), nbat, n, L, float(alpha), _ptr(out), flags, _ptr(ws),
                ws.numel(), self._stream(dev))),
            "lk_gram_nt_seg_f32",
        )
        return out

    is_channels_last = staticmethod(lambda x: is_channels_last(x))

    def nchw_to_nhwc(self, x, out=None):
        if self.is_channels_last(x):  # already NHWC in memory (the sweep's own forward): a view, no pass over the data
            v = x.permute(0, 2, 3, 1)
            if out is None:
                return v
            out.copy_(v)
            return out
        _check(x, "x")
        B, C, H, W = x.shape
        if out is None:
            out = torch.empty(B, H, W, C, dtype=torch.float32, device=x.device)
        else:
            _check(out, "out")
            assert tuple(out.shape) == (B, H, W, C)
        if B:
            self._rc(self.lib.lk_nchw_to_nhwc_f32(_ptr(x), B, C, H * W, _ptr(out), self._stream(x.device)),
                     "lk_nchw_to_nhwc_f32")
        return out

    # ---- split-fp16 convolution (lk_conv.hip) ---------------------------------------------------------
    def absmax(self, x, out=None):
        """device word holding the bit pattern of ``max |x|`` (a [1] float32 tensor: the bits ARE that float)"""
        _check(x, "x")
        if out is None:
            out = torch.empty(1, dtype=torch.float32, device=x.device)
        self._rc(self.lib.lk_absmax_f32(_ptr(x), x.numel(), None, 1, 1, _ptr(out), self._stream(x.device)), "lk_absmax_f32")
        return out

    #: ``False``: the stacked pixel-pair inputs are copied by the runtime and measured in a pass of their own before they
    #: are split (measured: no difference in the step; one pass less at the end of a fit)
    use_copy_absmax = True

    def copy_absmax(self, x, out, amax):
        """``out[...] = x`` and ``amax[0] = max(amax[0], max|x|)`` in one pass (lk_copy_absmax_f32); ``amax`` is not reset"""
        _check(x, "x"), _check(out, "out"), _check(amax, "amax")
        if not (x.is_contiguous() and out.is_contiguous() and x.numel() == out.numel() and x.numel() % 4 == 0
                and x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0):
            raise LaplaceHipError("copy_absmax: contiguous 16-byte aligned tensors of the same size, numel % 4 == 0")
        self._rc(self.lib.lk_copy_absmax_f32(_ptr(x), _ptr(out), x.numel(), _ptr(amax), self._stream(x.device)), "lk_copy_absmax_f32")
        return out

    def split_f16x2(self, x, amax=None, bound_mul=1.0, out=None):
        """fp32 tensor -> :class:`SplitTensor` of the same shape (scale from ``amax[0] * bound_mul``, measured if absent).
        ``out``: fp16 ``[2, *x.shape]`` workspace for the planes (each plane contiguous), allocated if absent"""
        _check(x, "x")
        if x.numel() % 8:
            raise LaplaceHipError("split_f16x2: numel % 8 != 0")
        if amax is None:
            amax = self.absmax(x)
        planes = out if out is not None else torch.empty((2,) + tuple(x.shape), dtype=torch.float16, device=x.device)
        if (planes.dtype != torch.float16 or tuple(planes.shape) != (2,) + tuple(x.shape) or planes.device != x.device
                or not planes[0].is_contiguous() or not planes[1].is_contiguous()):
            raise LaplaceHipError("split_f16x2: out must be fp16 [2, *x.shape] with contiguous planes on x's device")
        sexp = torch.empty(1, dtype=torch.int32, device=x.device)
        self._rc(self.lib.lk_split_f16x2(_ptr(x), x.numel(), _ptr(amax), float(bound_mul), _ptr(planes[0]), _ptr(planes[1]),
                                         _ptr(sexp), self._stream(x.device)), "lk_split_f16x2")
        return SplitTensor(planes, sexp)

    #: ``False``: the A factors of strided / stem convolutions stay on the exact-fp32 MFMA kernel (lk_gram_conv_nhwc_f32)
    use_gram_conv16 = True

    def im2col_split(self, x, kernel_size, stride, padding, Kp, amax=None):
        """lk_im2col_split_f16x2: the patch matrix of a convolution over ``x`` (logical ``[B, C, H, W]`` over NHWC memory, fp32) as a
        :class:`SplitTensor` ``[B * Ho * Wo, Kp]`` with one scale — columns in the kernels' native order ``(kh, kw, ci)``, zero
        padded to ``Kp`` columns"""
        if x.dim() != 4:
            raise LaplaceHipError("im2col_split: a [B, C, H, W] tensor")
        if not self.is_channels_last(x):
            _check(x, "x")
        B, C, H, W = x.shape
        xh = self.nchw_to_nhwc(x)  # (a view when x is NHWC in memory already)
        (KH, KW), s, p = kernel_size, int(stride), int(padding)
        Ho, Wo = (H + 2 * p - KH) // s + 1, (W + 2 * p - KW) // s + 1
        if amax is None:
            amax = self.absmax(xh)
        rows = B * Ho * Wo
        planes = torch.empty((2, rows, Kp), dtype=torch.float16, device=x.device)
        sexp = torch.empty(1, dtype=torch.int32, device=x.device)
        self._rc(self._timed("im2col16", 4.0 * xh.numel() + 4.0 * rows * Kp, x.device, lambda: self.lib.lk_im2col_split_f16x2(
            _ptr(xh), B, H, W, C, KH, KW, s, p, Ho, Wo, int(Kp), _ptr(amax), _ptr(planes[0]), _ptr(planes[1]), _ptr(sexp),
            self._stream(x.device))), "lk_im2col_split_f16x2")
        return SplitTensor(planes, sexp)

    def split_images_f16x2(self, x):
        """fp32 ``[N, ...]`` -> :class:`SplitTensor` with ONE SCALE PER IMAGE (lk_split_images_f16x2): ``sexp [N]`` from
        each image's own ``max|x_n|``, which rides along as ``amax [N]``"""
        _check(x, "x")
        N = x.shape[0]
        per = x.numel() // max(N, 1)
        if per % 8:
            raise LaplaceHipError("split_images_f16x2: elements per image % 8 != 0")
        planes = torch.empty((2,) + tuple(x.shape), dtype=torch.float16, device=x.device)
        sexp = torch.empty(N, dtype=torch.int32, device=x.device)
        amax = torch.empty(N, dtype=torch.float32, device=x.device)
        for i in range(0, max(N, 1), self.MAX_IMAGES_PER_LAUNCH):  # (the image index is a grid dimension: 65535 per launch)
            n = min(self.MAX_IMAGES_PER_LAUNCH, N - i)
            self._rc(self.lib.lk_split_images_f16x2(_ptr(x[i:i + n]), n, per, _ptr(planes[0][i:i + n]), _ptr(planes[1][i:i + n]),
                                                    _ptr(sexp[i:i + n]), _ptr(amax[i:i + n]), self._stream(x.device)),
                     "lk_split_images_f16x2")
        return SplitTensor(planes, sexp, amax)

    MAX_IMAGES_PER_LAUNCH = 65535

    def conv_prep_weights(self, W, transpose, cscale=None):
        """conv weight ``[Co, Ci, KH, KW]`` -> (planes ``[2, T, N, K]`` fp16, sexp); see lk_conv_prep_weights_f16x2"""
        _check(W, "W")
        Co, Ci = W.shape[0], W.shape[1]
        T = W[0, 0].numel()
        N, Kd = (Ci, Co) if transpose else (Co, Ci)
        planes = torch.empty(2, T, N, Kd, dtype=torch.float16, device=W.device)
        sexp = torch.empty(1, dtype=torch.int32, device=W.device)
        ws = torch.empty(1, dtype=torch.int32, device=W.device)
        if cscale is not None:
            _check(cscale, "cscale")
        self._rc(self.lib.lk_conv_prep_weights_f16x2(_ptr(W), Co, Ci, T, 1 if transpose else 0, _ptr(cscale), _ptr(ws),
                                                     _ptr(planes), _ptr(sexp), self._stream(W.device)),
                 "lk_conv_prep_weights_f16x2")
        return planes, sexp

    def _zero16(self, dev):
        z = self._zeros.get(dev.index) if hasattr(self, "_zeros") else None
        if z is None:
            if not hasattr(self, "_zeros"):
                self._zeros = {}
            z = self._zeros[dev.index] = torch.zeros(64, dtype=torch.uint8, device=dev)
        return z

    @staticmethod
    def conv_valid_pairs(Hc, Wc, in_mul, Hi, Wi, taps) -> int:
        """(output pixel, tap) pairs of one image whose input pixel ``(i * in_mul + dh, j * in_mul + dw)`` lies INSIDE the
        ``Hi x Wi`` map: the multiply-adds the convolution has to do (zero-padding taps are no work, and the kernels
        skip them where a tile holds none) — the flop figure behind the roofline numbers."""
        def inside(n_out, n_in, d):
            lo = 0 if d >= 0 else (-d + in_mul - 1) // in_mul          # first i with i * in_mul + d >= 0
            hi = min(n_out - 1, (n_in - 1 - d) // in_mul) if n_in - 1 - d >= 0 else -1
            return max(hi - lo + 1, 0)

        return sum(inside(Hc, Hi, t[0]) * inside(Wc, Wi, t[1]) for t in taps)

    def conv_nhwc_f16x2(self, x, wplanes, wsexp, Hc, Wc, in_mul, out, out_step, oh0, ow0, taps, accumulate=False,
                        amax_out=None, config=None):
        """one launch of lk_conv_nhwc_f16x2; ``x``: SplitTensor [N, Hi, Wi, Ci]; ``wplanes`` [2, T, Co, Ci];
        ``out`` fp32 [N, Ho, Wo, Co]; ``taps``: list of (dh, dw, weight slice)"""
        N, Hi, Wi, Ci = x.planes.shape[1:]
        _check(out, "out")
        Co = wplanes.shape[2]
        assert wplanes.shape[3] == Ci and out.shape[0] == N and out.shape[3] == Co
        flat = (ctypes.c_int * (3 * len(taps)))(*[int(v) for t in taps for v in t])
        cfg = self.conv_config if config is None else config
        z = self._zero16(out.device)
        # algorithmic work: the fp32 multiply-adds of the convolution (each is three fp16 MFMA multiply-adds on the chip)
        work = 2.0 * N * Co * Ci * self.conv_valid_pairs(Hc, Wc, in_mul, Hi, Wi, taps) if self.profile is not None else 0.0
        self._rc(self._timed("conv16", work, out.device, lambda: self.lib.lk_conv_nhwc_f16x2(
            _ptr(x.planes[0]), _ptr(x.planes[1]), _ptr(x.sexp), x.sexp.numel(), N, Hi, Wi, Ci, _ptr(wplanes[0]), _ptr(wplanes[1]),
            _ptr(wsexp), Co, Hc, Wc, in_mul, out.shape[1], out.shape[2], out_step, oh0, ow0, len(taps), flat, _ptr(z),
            _ptr(out), 1 if accumulate else 0, _ptr(amax_out), int(cfg), self._stream(out.device))), "lk_conv_nhwc_f16x2")
        return out

    def conv_nhwc_f16x2_planes(self, x, wplanes, wsexp, w_l1, Ho, Wo, in_mul, taps, config=None):
        """lk_conv_nhwc_f16x2_planes: the convolution of SplitTensor ``x [N, Hi, Wi, Ci]`` with ``wplanes [2, T, Co, Ci]``,
        position-contiguous and ALREADY SPLIT: SplitTensor ``[N, Co, Ho * Wo]`` with the scales of ``x``'s granularity
        (one for the tensor or one per image), each from the bound ``max|x_n| * w_l1`` (no pass over the output)"""
        N, Hi, Wi, Ci = x.planes.shape[1:]
        Co = wplanes.shape[2]
        dev = x.planes.device
        assert wplanes.shape[3] == Ci and (Ho * Wo) % 16 == 0
        planes = torch.empty((2, N, (Ho * Wo) // 16, Co, 16), dtype=torch.float16, device=dev)  # chunk-major (SplitTensor.chunked)
        sexp = torch.empty(x.sexp.numel(), dtype=torch.int32, device=dev)
        flat = (ctypes.c_int * (3 * len(taps)))(*[int(v) for t in taps for v in t])
        cfg = self.conv_config if config is None else config
        amax = x.amax if (x.amax is not None and x.amax.numel() == x.sexp.numel()) else None
        work = 2.0 * N * Co * Ci * self.conv_valid_pairs(Ho, Wo, in_mul, Hi, Wi, taps) if self.profile is not None else 0.0
        self._rc(self._timed("conv16", work, dev, lambda: self.lib.lk_conv_nhwc_f16x2_planes(
            _ptr(x.planes[0]), _ptr(x.planes[1]), _ptr(x.sexp), x.sexp.numel(), _ptr(amax), N, Hi, Wi, Ci, _ptr(wplanes[0]),
            _ptr(wplanes[1]), _ptr(wsexp), _ptr(w_l1), Co, Ho, Wo, in_mul, len(taps), flat, _ptr(self._zero16(dev)),
            _ptr(planes[0]), _ptr(planes[1]), _ptr(sexp), int(cfg), self._stream(dev))), "lk_conv_nhwc_f16x2_planes")
        return SplitTensor(planes, sexp, chunked=True)

    #: ``False``: the forward's convolutions and their BatchNorm / add / ReLU stay two launches (lk_conv_nhwc_f16x2 +
    #: lk_bn_act_fwd_nhwc_f16x2) instead of one (lk_conv_bn_act_nhwc_f16x2); the results are the same to the bit
    use_conv_bn_act = True

    def conv_bn_act_nhwc(self, x, wplanes, wsexp, w_l1, Ho, Wo, in_mul, taps, scale, shift, scale_amax, shift_amax, act,
                         addend=None, addend_bound=None, want_mask=True, want_split=True, amax_words=None, config=None,
                         y_out=None):
        """(``y_out``: where ``y`` is written — an fp32 NHWC tensor of its shape, e.g. a slot of the consumer's pixel-pair stack)
        lk_conv_bn_act_nhwc_f16x2: ``act(conv(x, W) * scale[c] + shift[c] + addend)`` for the per-image SplitTensor
        ``x [N, Hi, Wi, Ci]`` (``x.amax``: the measured per-image maxima) -> ``(y, mask, split, bound)`` exactly as
        :meth:`conv_nhwc_f16x2` followed by :meth:`bn_act_forward_nhwc` returns them (``y`` fp32 NHWC ``[N, Ho, Wo, Co]``)"""
        N, Hi, Wi, Ci = x.planes.shape[1:]
        Co = wplanes.shape[2]
        dev = x.planes.device
        if x.amax is None or x.amax.numel() not in (1, N) or wplanes.shape[3] != Ci or Co % 8:
            raise LaplaceHipError("conv_bn_act_nhwc: per-image maxima of the input, matching channels, Co % 8 == 0")
        if N > self.MAX_IMAGES_PER_LAUNCH:
            raise LaplaceHipError("conv_bn_act_nhwc: at most %d images per launch" % self.MAX_IMAGES_PER_LAUNCH)
        if y_out is not None and (tuple(y_out.shape) != (N, Ho, Wo, Co) or y_out.dtype != torch.float32 or not y_out.is_contiguous()
                                  or y_out.device != dev):
            raise LaplaceHipError("conv_bn_act_nhwc: y_out must be a contiguous fp32 [N, Ho, Wo, Co] tensor on the input's device")
        y = y_out if y_out is not None else torch.empty((N, Ho, Wo, Co), dtype=torch.float32, device=dev)
        mask = torch.empty(y.shape, dtype=torch.uint8, device=dev) if (act == 1 and want_mask) else None
        planes = torch.empty((2,) + tuple(y.shape), dtype=torch.float16, device=dev) if want_split else None
        sexp = torch.empty(N, dtype=torch.int32, device=dev)
        bound = torch.empty(N, dtype=torch.float32, device=dev)
        amax = amax_words if amax_words is not None else torch.zeros(N, dtype=torch.float32, device=dev)
        if addend is not None:
            _check(addend, "addend")
            if tuple(addend.shape) != tuple(y.shape) or addend_bound is None or addend_bound.numel() not in (1, N):
                raise LaplaceHipError("conv_bn_act_nhwc: the addend has the output's shape and a bound of 1 or N entries")
        if amax.numel() != N:
            raise LaplaceHipError("conv_bn_act_nhwc: amax_words has N entries")
        flat = (ctypes.c_int * (3 * len(taps)))(*[int(v) for t in taps for v in t])
        cfg = self.conv_config if config is None else config
        work = 2.0 * N * Co * Ci * self.conv_valid_pairs(Ho, Wo, in_mul, Hi, Wi, taps) if self.profile is not None else 0.0
        self._rc(self._timed("conv16", work, dev, lambda: self.lib.lk_conv_bn_act_nhwc_f16x2(
            _ptr(x.planes[0]), _ptr(x.planes[1]), _ptr(x.sexp), x.sexp.numel(), _ptr(x.amax), x.amax.numel(), N, Hi, Wi, Ci,
            _ptr(wplanes[0]), _ptr(wplanes[1]), _ptr(wsexp), _ptr(w_l1), Co, Ho, Wo, in_mul, len(taps), flat,
            _ptr(self._zero16(dev)), _ptr(scale), _ptr(shift), _ptr(scale_amax), _ptr(shift_amax), _ptr(addend),
            _ptr(addend_bound), 1 if addend_bound is None else addend_bound.numel(), int(act), _ptr(y), _ptr(mask),
            None if planes is None else _ptr(planes[0]), None if planes is None else _ptr(planes[1]), _ptr(sexp), _ptr(bound),
            _ptr(amax), int(cfg), self._stream(dev))), "lk_conv_bn_act_nhwc_f16x2")
        return y, mask, (SplitTensor(planes, sexp, amax) if planes is not None else None), bound

    #: ``False``: fused 64-channel launches stay on the generic kernel (see :meth:`conv_winp_eligible`)
    use_winp = True

    #: ``entry`` of :meth:`conv_launch_variant` (LK_CONV_* of include/laplace_hip.h)
    CONV_PLAIN, CONV_PLANES, CONV_BN_ACT, CONV_VJP = range(4)
    _CONV_KERNELS = ("generic", "window-256", "window-512", "strided")
    _CONV_EPILOGUES = ("plain", "planes", "vjp", "forward")

    @classmethod
    def _conv_variant(cls, rc, o):
        if rc < 0:
            return None
        return {"kernel": cls._CONV_KERNELS[o[0]], "bm": o[1], "bn": o[2], "epilogue": cls._CONV_EPILOGUES[o[3]], "pmajor": bool(o[4]),
                "dense": bool(o[5]), "grid": o[6], "nb_m": o[7], "nb_n": o[8], "coloc": o[9], "split_S": o[10], "split_L": o[11],
                "wg_per_cu": o[12], "n_tiles": o[13], "out_nchw": bool(o[14]), "ncls": o[15]}

    def conv_launch_variant(self, entry, N, Hi, Wi, Ci, Co, Ho, Wo, taps, Hc=None, Wc=None, in_mul=1, out_step=1, oh0=0, ow0=0,
                            in_nsexp=1, have_wc=False, mask_is_float=False, config=None):
        """lk_conv_launch_variant: kernel, tile, epilogue, row order and grid the launch takes (host only; ``grid`` and what follows
        from it depend on the device's CU count, 256 without a device), or ``None`` for a refused shape.  ``taps``: rows
        ``(dh, dw, weight slice)``; ``config``: as the launch would carry it (default: ``conv_config``)."""
        flat = (ctypes.c_int * max(3 * len(taps), 1))(*[int(v) for t in taps for v in t])
        out = (ctypes.c_int * 16)()
        cfg = self.conv_config if config is None else config
        rc = self.lib.lk_conv_launch_variant(int(entry), int(N), int(Hi), int(Wi), int(Ci), int(Co), int(Ho if Hc is None else Hc),
                                             int(Wo if Wc is None else Wc), int(in_mul), int(Ho), int(Wo), int(out_step), int(oh0),
                                             int(ow0), len(taps), flat, int(in_nsexp), int(bool(have_wc)), int(bool(mask_is_float)),
                                             int(cfg), out)
        return self._conv_variant(rc, out)

    def conv_strided_launch_variant(self, N, Hi, Wi, Ci, Co, Ho, Wo, os, taps, two_sources=False):
        """lk_conv_strided_launch_variant: the same for lk_conv_nhwc_f16x2_vjp_strided (``taps``: rows of six)"""
        flat = (ctypes.c_int * max(6 * len(taps), 1))(*[int(v) for t in taps for v in t])
        out = (ctypes.c_int * 16)()
        rc = self.lib.lk_conv_strided_launch_variant(int(N), int(Hi), int(Wi), int(Ci), int(Co), int(Ho), int(Wo), int(os), len(taps),
                                                     flat, int(bool(two_sources)), out)
        return self._conv_variant(rc, out)

    def conv_winp_eligible(self, N, Hi, Wi, Ci, Co, T, mask_is_float=False) -> bool:
        """does a fused 3 x 3 / stride-1 launch of this shape run the persistent window form (lk_conv_nhwc_f16x2_vjp_wc)?  The
        caller then hands over chunk-major weights (``wplanes_chunked``)"""
        return bool(self.use_winp and self.lib.lk_conv_winp_eligible(int(N), int(Hi), int(Wi), int(Ci), int(Co), int(T),
                                                                     1 if mask_is_float else 0))

    def conv_nhwc_f16x2_vjp(self, x, wplanes, wsexp, w_l1, Ho, Wo, taps, add=None, mult=None, mult_amax=None, scale=None,
                            scale_amax=None, config=None, amax_word=None, wplanes_chunked=None):
        """one dense launch of the convolution with the element-wise VJP fused into its epilogue (lk_conv_nhwc_f16x2_vjp):
        ``(conv(x) + add) * mult * scale[channel]`` -> SplitTensor [N, Ho, Wo, Co] carrying its measured ``amax``.
        ``mult``: [B, Ho, Wo, Co] uint8 / bool mask or fp32 multiplier (``mult_amax``: its bound, fp32 only), shared by
        the N / B seeds; ``add``: SplitTensor of the output's shape; ``w_l1``: device word, see conv.PreparedConv."""
        N, Hi, Wi, Ci = x.planes.shape[1:]
        Co = wplanes.shape[2]
        dev = x.planes.device
        assert wplanes.shape[3] == Ci
        _one_scale(x, "conv_nhwc_f16x2_vjp"), _one_scale(add, "conv_nhwc_f16x2_vjp")
        planes = torch.empty((2, N, Ho, Wo, Co), dtype=torch.float16, device=dev)
        sexp = torch.empty(1, dtype=torch.int32, device=dev)
        amax = amax_word if amax_word is not None else torch.zeros(1, dtype=torch.float32, device=dev)
        m_is_float, mask_rows = 0, 0
        if mult is not None:
            if mult.dtype == torch.bool:
                mult = mult.view(torch.uint8)
            m_is_float = 1 if mult.dtype == torch.float32 else 0
            if (not mult.is_contiguous() or mult.dtype not in (torch.uint8, torch.float32) or mult.dim() != 4
                    or tuple(mult.shape[1:]) != (Ho, Wo, Co) or N % mult.shape[0]):
                raise LaplaceHipError("conv_nhwc_f16x2_vjp: multiplier must be a contiguous [B, Ho, Wo, Co] uint8 / float32 tensor")
            mask_rows = mult.shape[0] * Ho * Wo
        if add is not None and tuple(add.shape) != (N, Ho, Wo, Co):
            raise LaplaceHipError("conv_nhwc_f16x2_vjp: addend shape")
        flat = (ctypes.c_int * (3 * len(taps)))(*[int(v) for t in taps for v in t])
        cfg = self.conv_config if config is None else config
        z = self._zero16(dev)
        work = 2.0 * N * Co * Ci * self.conv_valid_pairs(Ho, Wo, 1, Hi, Wi, taps) if self.profile is not None else 0.0
        # algorithmic bytes: cotangent planes in, result planes out, the addend's planes, the multiplier once per sample, weights
        nbytes = (4.0 * N * Hi * Wi * Ci + 4.0 * N * Ho * Wo * Co * (2 if add is not None else 1)
                  + (mult.numel() * mult.element_size() if mult is not None else 0) + 4.0 * wplanes[0].numel())
        if wplanes_chunked is not None:
            # [2, T, Ci / 16, Co, 16]: the persistent window form where the library finds the launch eligible
            assert wplanes_chunked.shape == (2, wplanes.shape[1], Ci // 16, Co, 16) and wplanes_chunked.is_contiguous()
            # (profile family: the persistent window kernel unless config bit 27 sends the launch to the generic one)
            self._rc(self._timed("conv16" if int(cfg) & (1 << 27) else "convp16", work, dev, lambda: self.lib.lk_conv_nhwc_f16x2_vjp_wc(
                _ptr(x.planes[0]), _ptr(x.planes[1]), _ptr(x.sexp), _ptr(x.amax), N, Hi, Wi, Ci, _ptr(wplanes[0]),
                _ptr(wplanes[1]), _ptr(wsexp), _ptr(w_l1), _ptr(wplanes_chunked[0]), _ptr(wplanes_chunked[1]), Co, Ho, Wo,
                len(taps), flat, _ptr(z), None if add is None else _ptr(add.planes[0]),
                None if add is None else _ptr(add.planes[1]), None if add is None else _ptr(add.sexp), _ptr(mult), m_is_float,
                _ptr(mult_amax), mask_rows, _ptr(scale), _ptr(scale_amax), _ptr(planes[0]), _ptr(planes[1]), _ptr(sexp),
                _ptr(amax), int(cfg), self._stream(dev)), nbytes=nbytes), "lk_conv_nhwc_f16x2_vjp_wc")
            return SplitTensor(planes, sexp, amax)
        self._rc(self._timed("conv16", work, dev, lambda: self.lib.lk_conv_nhwc_f16x2_vjp(
            _ptr(x.planes[0]), _ptr(x.planes[1]), _ptr(x.sexp), _ptr(x.amax), N, Hi, Wi, Ci, _ptr(wplanes[0]), _ptr(wplanes[1]),
            _ptr(wsexp), _ptr(w_l1), Co, Ho, Wo, len(taps), flat, _ptr(z),
            None if add is None else _ptr(add.planes[0]), None if add is None else _ptr(add.planes[1]),
            None if add is None else _ptr(add.sexp), _ptr(mult), m_is_float, _ptr(mult_amax), mask_rows, _ptr(scale),
            _ptr(scale_amax), _ptr(planes[0]), _ptr(planes[1]), _ptr(sexp), _ptr(amax), int(cfg), self._stream(dev)), nbytes=nbytes),
            "lk_conv_nhwc_f16x2_vjp")
        return SplitTensor(planes, sexp, amax)

    def conv_nhwc_f16x2_vjp_strided(self, sources, Ho, Wo, os, taps, add=None, mult=None, mult_amax=None, scale=None,
                                    scale_amax=None, amax_word=None):
        """lk_conv_nhwc_f16x2_vjp_strided: the backward-data of one or two stride-``os`` convolutions that read the same
        input, every residue class in one launch, with the element-wise VJP fused: ``(dX [+ dX2] + add) * mult * scale``
        -> SplitTensor [N, Ho, Wo, Co] carrying its measured ``amax``.  ``sources``: one or two
        ``(g SplitTensor [N, Ho/os, Wo/os, Ci], wplanes [2, T_w, Co, Ci], wsexp, w_l1)``; ``taps``: rows
        ``(dh, dw, weight slice, source, oh0, ow0)``."""
        x, wplanes, wsexp, w_l1 = sources[0]
        N, Hi, Wi, Ci = x.planes.shape[1:]
        Co = wplanes.shape[2]
        dev = x.planes.device
        if len(sources) not in (1, 2) or any(tuple(s_[0].planes.shape) != tuple(x.planes.shape) or s_[1].shape[2:] != wplanes.shape[2:]
                                             for s_ in sources):
            raise LaplaceHipError("conv_nhwc_f16x2_vjp_strided: one or two sources of the same shapes")
        for s_ in sources:
            _one_scale(s_[0], "conv_nhwc_f16x2_vjp_strided")
        _one_scale(add, "conv_nhwc_f16x2_vjp_strided")
        planes = torch.empty((2, N, Ho, Wo, Co), dtype=torch.float16, device=dev)
        sexp = torch.empty(1, dtype=torch.int32, device=dev)
        amax = amax_word if amax_word is not None else torch.zeros(1, dtype=torch.float32, device=dev)
        m_is_float, mask_rows = 0, 0
        if mult is not None:
            if mult.dtype == torch.bool:
                mult = mult.view(torch.uint8)
            m_is_float = 1 if mult.dtype == torch.float32 else 0
            if (not mult.is_contiguous() or mult.dtype not in (torch.uint8, torch.float32) or mult.dim() != 4
                    or tuple(mult.shape[1:]) != (Ho, Wo, Co) or N % mult.shape[0]):
                raise LaplaceHipError("conv_nhwc_f16x2_vjp_strided: multiplier must be a contiguous [B, Ho, Wo, Co] uint8 / float32 tensor")
            mask_rows = mult.shape[0] * Ho * Wo
        if add is not None and tuple(add.shape) != (N, Ho, Wo, Co):
            raise LaplaceHipError("conv_nhwc_f16x2_vjp_strided: addend shape")
        flat = (ctypes.c_int * (6 * len(taps)))(*[int(v) for t in taps for v in t])
        work = 0.0
        if self.profile is not None:
            classes = {}
            for t in taps:
                classes.setdefault((t[4], t[5]), []).append(t)
            work = 2.0 * N * Co * Ci * sum(self.conv_valid_pairs(Ho // os, Wo // os, 1, Hi, Wi, ts) for ts in classes.values())
        src = []
        for i in range(2):
            if i < len(sources):
                g_, wp_, ws_, l1_ = sources[i]
                src += [_ptr(g_.planes[0]), _ptr(g_.planes[1]), _ptr(g_.sexp), _ptr(g_.amax), _ptr(wp_[0]), _ptr(wp_[1]), _ptr(ws_), _ptr(l1_)]
            else:
                src += [None] * 8
        self._rc(self._timed("convs16", work, dev, lambda: self.lib.lk_conv_nhwc_f16x2_vjp_strided(
            *src, N, Hi, Wi, Ci, Co, Ho, Wo, os, len(taps), flat, _ptr(self._zero16(dev)),
            None if add is None else _ptr(add.planes[0]), None if add is None else _ptr(add.planes[1]),
            None if add is None else _ptr(add.sexp), _ptr(mult), m_is_float, _ptr(mult_amax), mask_rows, _ptr(scale),
            _ptr(scale_amax), _ptr(planes[0]), _ptr(planes[1]), _ptr(sexp), _ptr(amax), int(self.conv_config),
            self._stream(dev))), "lk_conv_nhwc_f16x2_vjp_strided")
        return SplitTensor(planes, sexp, amax)

    def vjp_nhwc_split(self, g, g_amax, g2, mult, mult_amax, scale, scale_amax, S, out_shape):
        """``(g + g2) * mult * scale[channel]`` for all ``S`` seeds -> SplitTensor of ``out_shape`` ([S*B, H, W, C]).
        ``g``: fp32 NHWC with ``g_amax`` (device word, lk_absmax / conv epilogue) or None; ``g2``: SplitTensor or None;
        ``mult``: [B, H, W, C] uint8 / bool mask or fp32 multiplier (``mult_amax`` for fp32) or None."""
        dev = (g if g is not None else g2.planes).device
        _one_scale(g2, "vjp_nhwc_split")
        planes = torch.empty((2,) + tuple(out_shape), dtype=torch.float16, device=dev)
        sexp = torch.empty(1, dtype=torch.int32, device=dev)
        n = planes[0].numel()
        per = n // S
        C = out_shape[-1]
        m_is_float = 0
        if mult is not None:
            if mult.dtype == torch.bool:
                mult = mult.view(torch.uint8)
            m_is_float = 1 if mult.dtype == torch.float32 else 0
            if not mult.is_contiguous() or mult.numel() != per or mult.dtype not in (torch.uint8, torch.float32):
                raise LaplaceHipError("vjp_nhwc_split: multiplier must be a contiguous [B, H, W, C] uint8 / float32 tensor")
        if g is not None:
            _check(g, "g")
        # HBM-bound: algorithmic bytes = every addend read once, the planes written once, the multiplier once per sample
        nbytes = 4.0 * n * ((g is not None) + (g2 is not None) + 1) + (per * (4 if m_is_float else 1) if mult is not None else 0)
        self._rc(self._timed("vjp16", nbytes, dev, lambda: self.lib.lk_vjp_nhwc_split_f16x2(
            _ptr(g), _ptr(g_amax), None if g2 is None else _ptr(g2.planes[0]), None if g2 is None else _ptr(g2.planes[1]),
            None if g2 is None else _ptr(g2.sexp), _ptr(mult), m_is_float, _ptr(mult_amax), _ptr(scale), _ptr(scale_amax),
            C, S, per, _ptr(planes[0]), _ptr(planes[1]), _ptr(sexp), self._stream(dev))), "lk_vjp_nhwc_split_f16x2")
        return SplitTensor(planes, sexp)

    def bn_act_forward_nhwc(self, x, x_amax, scale, shift, scale_amax, shift_amax, act, addend=None, addend_bound=None,
                            want_mask=True, want_split=True, x_mul=None, x_add=None, amax_words=None):
        """``y = act(x * scale[c] + shift[c] + addend)`` on fp32 NHWC ``x [B, H, W, C]`` -> ``(y, mask, split, bound)``:
        ``mask`` NHWC uint8 (ReLU only), ``split`` the SplitTensor of ``y`` with ONE SCALE PER IMAGE and its measured
        per-image maxima as ``split.amax`` (``[B]``), ``bound [B]`` the guaranteed bounds the scales were derived from.
        ``x_amax``: 1 or B words bounding ``x`` per image after ``* x_mul[0] + x_add[0]`` (device words; a convolution's
        output: the measured maxima of its input images, the l1 norm of its weights, max|bias|); ``addend_bound``: 1 or B
        floats; ``amax_words``: zeroed ``[B]`` float32 buffer for the measured maxima (allocated if absent)."""
        _check(x, "x")
        C = x.shape[-1]
        B = x.shape[0]
        y = torch.empty_like(x)
        mask = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if (act == 1 and want_mask) else None
        planes = torch.empty((2,) + tuple(x.shape), dtype=torch.float16, device=x.device) if want_split else None
        sexp = torch.empty(B, dtype=torch.int32, device=x.device)
        bound = torch.empty(B, dtype=torch.float32, device=x.device)
        amax = amax_words if amax_words is not None else torch.zeros(B, dtype=torch.float32, device=x.device)
        if addend is not None:
            _check(addend, "addend")
        if x_amax.numel() not in (1, B) or (addend is not None and addend_bound.numel() not in (1, B)) or amax.numel() != B:
            raise LaplaceHipError("bn_act_forward_nhwc: x_amax / addend_bound have 1 or B entries, amax_words B")
        nbytes = x.numel() * (4.0 + 4.0 + (4.0 if addend is not None else 0.0) + (4.0 if want_split else 0.0)
                              + (1.0 if mask is not None else 0.0))
        per = x.numel() // max(B, 1)
        sl = lambda t, i, n: None if t is None else (t if t.numel() == 1 else t[i:i + n])  # a per-image vector, or one word

        def launch(i, n):
            return self.lib.lk_bn_act_fwd_nhwc_f16x2(
                _ptr(x[i:i + n]), _ptr(sl(x_amax, i, n)), min(x_amax.numel(), n), _ptr(x_mul), _ptr(x_add), _ptr(scale), _ptr(shift),
                _ptr(scale_amax), _ptr(shift_amax), None if addend is None else _ptr(addend[i:i + n]), _ptr(sl(addend_bound, i, n)),
                1 if addend_bound is None else min(addend_bound.numel(), n), int(act), C, n, per, _ptr(y[i:i + n]),
                None if mask is None else _ptr(mask[i:i + n]), None if planes is None else _ptr(planes[0][i:i + n]),
                None if planes is None else _ptr(planes[1][i:i + n]), _ptr(sexp[i:i + n]), _ptr(bound[i:i + n]), _ptr(amax[i:i + n]),
                self._stream(x.device))

        if B <= self.MAX_IMAGES_PER_LAUNCH:
            self._rc(self._timed("bnact16", nbytes, x.device, lambda: launch(0, B)), "lk_bn_act_fwd_nhwc_f16x2")
        else:  # (the image index is a grid dimension: 65535 per launch)
            for i in range(0, B, self.MAX_IMAGES_PER_LAUNCH):
                self._rc(launch(i, min(self.MAX_IMAGES_PER_LAUNCH, B - i)), "lk_bn_act_fwd_nhwc_f16x2")
        return y, mask, (SplitTensor(planes, sexp, amax) if planes is not None else None), bound

    def unsplit_transpose(self, x, S, B):
        """SplitTensor ``[S*B, H, W, C]`` (seed-major) -> fp32 ``[B, S, C, H*W]``"""
        N, H, W, C = x.shape
        assert N == S * B
        _one_scale(x, "unsplit_transpose")
        out = torch.empty(B, S, C, H * W, dtype=torch.float32, device=x.planes.device)
        self._rc(self.lib.lk_unsplit_transpose_f32(_ptr(x.planes[0]), _ptr(x.planes[1]), _ptr(x.sexp), S, B, H * W, C,
                                                   _ptr(out), self._stream(out.device)), "lk_unsplit_transpose_f32")
        return out

    def gram_tn_f16x2(self, x, alpha, out):
        """``out[upper tiles] += alpha * X^T X`` for a SplitTensor ``x`` viewed as ``[rows, C]``"""
        _check(out, "out")
        _one_scale(x, "gram_tn_f16x2")
        C = x.planes.shape[-1]
        R = x.planes[0].numel() // C
        nbytes = int(self.lib.lk_gram_tn_f16x2_workspace_bytes(R, C))
        if nbytes == 0 and R:
            raise LaplaceHipError(f"gram_tn_f16x2: C = {C} not supported (64 or a multiple of 128)")
        ws = self._workspace(nbytes, out.device)
        z = self._zero16(out.device)
        self._rc(self._timed("gram16", float(R) * C * (C + 1), out.device, lambda: self.lib.lk_gram_tn_f16x2(
            _ptr(x.planes[0]), _ptr(x.planes[1]), _ptr(x.sexp), R, C, float(alpha), _ptr(out), _ptr(z), _ptr(ws),
            ws.numel(), self._stream(out.device))), "lk_gram_tn_f16x2")
        return out

    # ---- packed upper triangles (lk_pack.hip) ---------------------------------------------------------------
    def pack_upper(self, A, packed):
        """upper triangle of the square ``A`` -> ``packed [n (n + 1) / 2]`` (a slice of the exchange buffer)"""
        _check(A, "A"), _check(packed, "packed")
        self._rc(self.lib.lk_pack_upper_f32(_ptr(A), A.shape[0], _ptr(packed), self._stream(A.device)), "lk_pack_upper_f32")

    def unpack_upper(self, packed, A):
        _check(A, "A"), _check(packed, "packed")
        self._rc(self.lib.lk_unpack_upper_f32(_ptr(packed), A.shape[0], _ptr(A), self._stream(A.device)), "lk_unpack_upper_f32")

    # ---- eigenbasis algebra of KronDecomposed (lk_gemm.hip) ------------------------------------------------
    def gemm(self, A, B, C, batch, M, N, Kd, lda, ldb, ldc, sa=0, sb=0, sc=0, ta=False, tb=False, E=None, lde=0,
             alpha=1.0, accumulate=False):
        """raw batched ``C[b] = alpha op(A[b]) op(B[b]) (.) E`` on device pointers / offsets of fp32 tensors (see
        lk_gemm_f32); ``A``, ``B``, ``C``, ``E`` are tensors whose ``data_ptr()`` is the first element"""
        self._rc(self.lib.lk_gemm_f32(_ptr(A), _ptr(B), _ptr(E), _ptr(C), batch, M, N, Kd, lda, ldb, ldc, lde, sa, sb, sc,
                                      1 if ta else 0, 1 if tb else 0, float(alpha), 1 if accumulate else 0,
                                      self._stream(C.device)), "lk_gemm_f32")

    def kron_pow(self, l1, l2, delta, exponent, damping=False):
        """``(l1 (x) l2 + delta) ** exponent`` as an ``[n1, n2]`` table (``l2`` None: ``[n1]``)"""
        _check(l1, "l1")
        n1 = l1.numel()
        n2 = 0 if l2 is None else l2.numel()
        lam = torch.empty((n1, n2) if l2 is not None else (n1,), dtype=torch.float32, device=l1.device)
        d = delta.detach().reshape(-1)[:1].to(torch.float32).contiguous()
        self._rc(self.lib.lk_kron_pow_f32(_ptr(l1), n1, _ptr(l2), n2, _ptr(d), float(exponent), 1 if damping else 0,
                                          _ptr(lam), self._stream(l1.device)), "lk_kron_pow_f32")
        return lam

    def kron_sandwich(self, W, col0, P, R, Q1, Q2, lam, out):
        """``out[r, col0:col0+p] = vec(Q1 ((Q1^T W_r Q2) (.) lam) Q2^T)`` for the ``R`` rows of ``W [R, P]`` (block of
        ``p = p_in * p_out`` columns at ``col0``); ``Q2`` None: the single-factor block ``((W_r Q1) (.) lam) Q1^T``.
        Operands are read and written in place (leading dimension ``P``)."""
        _check(W, "W"), _check(out, "out"), _check(Q1, "Q1"), _check(lam, "lam")
        Wv, Ov = W.reshape(-1)[col0:], out.reshape(-1)[col0:]
        if Q2 is None:
            p = Q1.shape[0]
            T = torch.empty(R, p, dtype=torch.float32, device=W.device)
            self.gemm(Wv, Q1, T, 1, R, p, p, P, p, p, E=lam, lde=0)
            self.gemm(T, Q1, Ov, 1, R, p, p, p, p, P, tb=True)
            return out
        _check(Q2, "Q2")
        pi, po = Q1.shape[0], Q2.shape[0]
        T = torch.empty(R, pi, po, dtype=torch.float32, device=W.device)
        U = torch.empty(R, pi, po, dtype=torch.float32, device=W.device)
        self.gemm(Wv, Q2, T, R, pi, po, po, po, po, po, sa=P, sc=pi * po)                       # T_r = W_r Q2
        self.gemm(Q1, T, U, R, pi, po, pi, pi, po, po, sb=pi * po, sc=pi * po, ta=True, E=lam, lde=po)  # (Q1^T T_r) . lam
        self.gemm(Q1, U, T, R, pi, po, pi, pi, po, po, sb=pi * po, sc=pi * po)                  # Q1 M_r
        self.gemm(T, Q2, Ov, R, pi, po, po, po, po, po, sa=pi * po, sc=P, tb=True)              # ... Q2^T -> out
        return out

    def gram_conv(self, x, kernel_size, stride, padding, dilation, alpha, out, upper_only=False, native=False):
        """``out += alpha * unfold(x)^T unfold(x)`` for an NCHW input ``x`` — without materialising unfold.

        ``native=True`` leaves ``out`` in the kernel's (kh, kw, ci) column order (fused accumulation);
        otherwise the result is delivered in F.unfold's (ci, kh, kw) order.
        """
        _check(out, "out")
        if not self.is_channels_last(x):
            _check(x, "x")
        B, Cin, H, W = x.shape
        kh, kw = _pair(kernel_size)
        sh, sw = _pair(stride)
        ph, pw = _pair(padding)
        dh, dw = _pair(dilation)
        n = Cin * kh * kw
        assert out.shape == (n, n)
        OH = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1
        OW = (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
        xh = self.nchw_to_nhwc(x)
        direct = native or kh * kw == 1
        tgt = out if direct else torch.zeros(n, n, dtype=torch.float32, device=x.device)
        if self.use_shiftcorr and (kh, kw, sh, sw, ph, pw, dh, dw) == (3, 3, 1, 1, 1, 1, 1, 1) and H * W >= 256 and B > 0:
            # 3x3 / stride 1 / pad 1 on maps >= 16x16: 13 shift correlations + boundary strips instead of 81 patch
            # blocks (measured 1.7x at 32x32, 1.2x at 16x16, a loss at 8x8: profiles/r01_microbench_gram_v4.txt)
            nb = self.lib.lk_conv3x3_shiftcorr_workspace_bytes(B, H, W, Cin)
            ws = self._workspace(nb, x.device)
            self._rc(
                self._timed("shiftcorr", float(B * H * W) * n * (n + 1), x.device, lambda: self.lib.lk_conv3x3_shiftcorr_f32(
                    _ptr(xh), B, H, W, Cin, float(alpha), _ptr(tgt), _ptr(ws), ws.numel(), self._stream(x.device))),
                "lk_conv3x3_shiftcorr_f32",
            )
            if not direct:
                self._rc(self.lib.lk_permute_sym_f32(_ptr(tgt), Cin, kh * kw, _ptr(out), 1, self._stream(x.device)),
                         "lk_permute_sym_f32")
            return out
        nb = self.lib.lk_gram_workspace_bytes(n, max(B * OH * OW, 1))
        ws = self._workspace(nb, x.device)
        self._rc(
            self._timed("gram_conv", float(B * OH * OW) * n * (n + 1), x.device, lambda: self.lib.lk_gram_conv_nhwc_f32(
                _ptr(xh), B, H, W, Cin, kh, kw, sh, sw, ph, pw, dh, dw, float(alpha), _ptr(tgt),
                LK_GRAM_UPPER_ONLY if upper_only else 0, _ptr(ws), ws.numel(), self._stream(x.device))),
            "lk_gram_conv_nhwc_f32",
        )
        if not direct:
            self._rc(self.lib.lk_permute_sym_f32(_ptr(tgt), Cin, kh * kw, _ptr(out), 1, self._stream(x.device)),
                     "lk_permute_sym_f32")
        return out

    # ---- pixel-pair form of the 3x3/s1/p1 conv A factor on small maps (see lk_gram.hip) --------------------------
    #: largest H*W for which KronAccumulator keeps a pixel-pair accumulator instead of calling gram_conv per step
    pixgram_max_hw = 16

    def pixgram_accumulate(self, x, alpha, Cp):
        """``Cp += alpha * X^T X`` with ``X`` the NHWC images flattened to rows ``[B, H*W*Cin]`` (upper tiles only)."""
        _check(Cp, "Cp")
        B = x.shape[0]
        xh = self.nchw_to_nhwc(x)
        return self.gram_tn(xh.reshape(B, -1), alpha, Cp, upper_only=True)

    def pixgram_assemble(self, Cp, H, W, Cin, alpha, A_native):
        """``A_native += alpha * assemble(Cp)`` (native (kh,kw,ci) order); symmetrises ``Cp`` in place first."""
        _check(Cp, "Cp"), _check(A_native, "A")
        self.symmetrize(Cp)
        self._rc(self.lib.lk_conv3x3_pixgram_assemble_f32(_ptr(Cp), int(H), int(W), int(Cin), float(alpha), _ptr(A_native),
                                                          self._stream(Cp.device)), "lk_conv3x3_pixgram_assemble_f32")
        return A_native

    # ---- banded pixel-pair form (any map size, Cin % 64 == 0) -------------------------------------------------------
    def pixpair_plan(self, H, W, Cin, dev):
        """(n_blocks, tiles_dev, slots_dev) for a geometry; tables are built by the library on the host and uploaded
        once per (geometry, device).  None if the geometry is not eligible (Cin % 64 != 0 or too large)."""
        key = (int(H), int(W), int(Cin), str(dev))
        cache = self.__dict__.setdefault("_pixpair_cache", {})
        if key not in cache:
            T, nt, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
            plan = None
            if Cin >= 64 and Cin % 64 == 0 and self.lib.lk_conv3x3_pixpair_plan(
                    int(H), int(W), int(Cin), ctypes.byref(T), ctypes.byref(nt), ctypes.byref(nb)) == 0:
                tiles = torch.empty(nt.value, 3, dtype=torch.int32)
                slots = torch.empty(int(H) * int(W), 13, dtype=torch.int32)
                self._rc(self.lib.lk_conv3x3_pixpair_tables(int(H), int(W), int(Cin), ctypes.c_void_p(tiles.data_ptr()),
                                                            ctypes.c_void_p(slots.data_ptr())), "lk_conv3x3_pixpair_tables")
                plan = (nb.value, tiles.to(dev), slots.to(dev))
            cache[key] = plan
        return cache[key]

    def pixpair_accumulate(self, x, alpha, blocks, plan):
        """``Blk[q, D] += alpha * sum_b x[b,q,:]^T x[b,q+D,:]`` for an NCHW input ``x``."""
        return self.pixpair_accumulate_nhwc(self.nchw_to_nhwc(x), alpha, blocks, plan)

    def pixpair_accumulate_nhwc(self, xh, alpha, blocks, plan):
        """Same for an NHWC input ``xh [B, H, W, Cin]`` (several minibatches may be stacked along ``B``: the blocks
        are read-modified-written once per launch, whatever the number of rows)."""
        _check(xh, "xh"), _check(blocks, "blocks")
        B, H, W, Cin = xh.shape
        nb, tiles, _ = plan
        assert blocks.numel() == nb * Cin * Cin
        x = xh
        # HBM-bound (each block is read-modified-written once per launch): work = algorithmic BYTES
        self._rc(self._timed("pixpair", 8.0 * blocks.numel() + 4.0 * x.numel(), x.device,
                             lambda: self.lib.lk_conv3x3_pixpair_accumulate_f32(
                                 _ptr(xh), B, H, W, Cin, float(alpha), _ptr(blocks), ctypes.c_void_p(tiles.data_ptr()),
                                 tiles.shape[0], self._stream(x.device))), "lk_conv3x3_pixpair_accumulate_f32")
        return blocks

    #: ``False``: the pixel-pair products stay on the exact-fp32 MFMA kernel.  The split-fp16 kernel
    #: requests the block it read-modify-writes at the START of its (short) tile: 0.87 vs 1.39 ms per c4 step — the
    #: dependent 16 KB read at the end of every 8-stage tile, not traffic or the matrix pipe, was what bound the product
    use_pixpair16 = True
    #: 64-channel maps: one workgroup per pixel with all 13 shifts (`lk_conv3x3_pixpair_accumulate13_f16x2`: the pixel's panel is
    #: staged once instead of 13 times); ``False``: one workgroup per (pixel, shift) block as for the wider maps
    use_pixpair13 = True

    def pixpair_accumulate_split(self, xs, alpha, blocks, plan):
        """:meth:`pixpair_accumulate_nhwc` on a SplitTensor ``xs [B, H, W, Cin]`` (three fp16 MFMAs per product block)."""
        _check(blocks, "blocks")
        _one_scale(xs, "pixpair_accumulate_split")
        B, H, W, Cin = xs.shape
        nb, tiles, slots = plan
        assert blocks.numel() == nb * Cin * Cin
        dev = blocks.device
        z = self._zero16(dev)
        if Cin == 64 and self.use_pixpair13:
            self._rc(self._timed("pixpair16", 8.0 * blocks.numel() + 4.0 * xs.planes[0].numel(), dev,
                                 lambda: self.lib.lk_conv3x3_pixpair_accumulate13_f16x2(
                                     _ptr(xs.planes[0]), _ptr(xs.planes[1]), _ptr(xs.sexp), B, H, W, Cin, float(alpha), _ptr(blocks),
                                     ctypes.c_void_p(slots.data_ptr()), _ptr(z), self._stream(dev))),
                     "lk_conv3x3_pixpair_accumulate13_f16x2")
            return blocks
        self._rc(self._timed("pixpair16", 8.0 * blocks.numel() + 4.0 * xs.planes[0].numel(), dev,
                             lambda: self.lib.lk_conv3x3_pixpair_accumulate_f16x2(
                                 _ptr(xs.planes[0]), _ptr(xs.planes[1]), _ptr(xs.sexp), B, H, W, Cin, float(alpha), _ptr(blocks),
                                 ctypes.c_void_p(tiles.data_ptr()), tiles.shape[0], _ptr(z), self._stream(dev))),
                 "lk_conv3x3_pixpair_accumulate_f16x2")
        return blocks

    def pixpair_assemble(self, blocks, plan, H, W, Cin, alpha, A_native, blocks2=None, upper_only=False):
        """``A_native += alpha * assemble(blocks [+ blocks2])``: ``blocks2`` is a second accumulator set of the same geometry
        (the other lane of a fit), summed on the fly; ``upper_only``: only the upper triangle of ``A_native`` is written (what
        :meth:`finalize_factors` and the packed exchange read)"""
        _check(blocks, "blocks"), _check(A_native, "A")
        if blocks2 is not None:
            _check(blocks2, "blocks2")
            assert blocks2.numel() == blocks.numel()
        self._rc(self.lib.lk_conv3x3_pixpair_assemble2_f32(_ptr(blocks), _ptr(blocks2), ctypes.c_void_p(plan[2].data_ptr()),
                                                           int(H), int(W), int(Cin), float(alpha), _ptr(A_native),
                                                           1 if upper_only else 0, self._stream(blocks.device)),
                 "lk_conv3x3_pixpair_assemble2_f32")
        return A_native

    def permute_native_to_unfold(self, src, Cin, KK, dst, accumulate=False):
        _check(src, "src"), _check(dst, "dst")
        self._rc(self.lib.lk_permute_sym_f32(_ptr(src), Cin, KK, _ptr(dst), 1 if accumulate else 0, self._stream(src.device)),
                 "lk_permute_sym_f32")
        return dst

    def finalize_factors(self, items):
        """The once-per-fit layout pass of many factors in one launch.  ``items``: ``(src, dst, scale, cin, kk)`` per
        factor — ``kk <= 1``: mirror the upper triangle (in place when ``dst`` is None), after ``diag(scale) C diag(scale)``
        when ``scale`` is given; ``kk > 1``: ``dst`` = the full matrix in unfold order from the native-order upper triangle
        of ``src`` (what :meth:`symmetrize` + :meth:`permute_native_to_unfold` do with two launches per factor)."""
        items = [it for it in items if it[0].numel()]
        if not items:
            return
        n = len(items)
        dev = items[0][0].device
        src = (ctypes.c_void_p * n)()
        dst = (ctypes.c_void_p * n)()
        scl = (ctypes.c_void_p * n)()
        ns = (ctypes.c_int64 * n)()
        cins = (ctypes.c_int64 * n)()
        kks = (ctypes.c_int64 * n)()
        for i, (s_, d_, sc_, cin, kk) in enumerate(items):
            _check(s_, "src")
            assert s_.dim() == 2 and s_.shape[0] == s_.shape[1] and s_.device == dev
            src[i] = s_.data_ptr()
            if d_ is not None:
                _check(d_, "dst")
                assert d_.shape == s_.shape
                dst[i] = d_.data_ptr()
            if sc_ is not None:
                _check(sc_, "scale")
                assert sc_.numel() == s_.shape[0]
                scl[i] = sc_.data_ptr()
            ns[i], cins[i], kks[i] = s_.shape[0], int(cin), int(kk)
        self._rc(self.lib.lk_finalize_factors_f32(n, src, dst, scl, ns, cins, kks, self._stream(dev)), "lk_finalize_factors_f32")

    def symmetrize(self, C):
        _check(C, "C")
        self._rc(self.lib.lk_symmetrize_f32(_ptr(C), C.shape[0], self._stream(C.device)), "lk_symmetrize_f32")
        return C

    # ---- diag / Jacobians ---------------------------------------------------------------------
    def diag_ggn_linear(self, a, g, alpha, h_w, h_b=None):
        _check(a, "a"), _check(g, "g"), _check(h_w, "h_w")
        Cc, B, Do = g.shape
        Di = a.shape[1]
        assert a.shape[0] == B and h_w.numel() == Do * Di
        if h_b is not None:
            _check(h_b, "h_b")
        self._rc(
            self.lib.lk_diag_ggn_linear_f32(_ptr(a), _ptr(g), B, Cc, Di, Do, float(alpha), _ptr(h_w), _ptr(h_b),
                                            self._stream(a.device)),
            "lk_diag_ggn_linear_f32",
        )

    def jac_linear(self, a, g, Js, col0, bcol0=-1):
        _check(a, "a"), _check(g, "g"), _check(Js, "Js")
        Cc, B, Do = g.shape
        Di = a.shape[1]
        P = Js.shape[-1]
        self._rc(
            self.lib.lk_jac_linear_f32(_ptr(a), _ptr(g), B, Cc, Di, Do, _ptr(Js), P, int(col0), int(bcol0),
                                       self._stream(a.device)),
            "lk_jac_linear_f32",
        )

    def jac_conv(self, x, g, kernel_size, stride, padding, dilation, Js, col0, bcol0=-1):
        _check(x, "x"), _check(g, "g"), _check(Js, "Js")
        B, Cin, H, W = x.shape
        Cc, _, Do = g.shape[:3]
        kh, kw = _pair(kernel_size)
        sh, sw = _pair(stride)
        ph, pw = _pair(padding)
        dh, dw = _pair(dilation)
        P = Js.shape[-1]
        self._rc(
            self.lib.lk_jac_conv_f32(_ptr(x), _ptr(g), B, Cc, Cin, H, W, Do, kh, kw, sh, sw, ph, pw, dh, dw, _ptr(Js), P,
                                     int(col0), int(bcol0), self._stream(x.device)),
            "lk_jac_conv_f32",
        )

    def jac_gconv(self, x, g, kernel_size, stride, padding, dilation, groups, Js, col0, bcol0=-1):
        """the weight (and bias) Jacobian columns of a grouped convolution: ``x [B, Cin, H, W]``, ``g [S, B, Do, OH, OW]``,
        ``Js [B, S, P]`` (csrc/lk_gconv.hip)"""
        _check(x, "x"), _check(g, "g"), _check(Js, "Js")
        B, Cin, H, W = x.shape
        Cc, _, Do = g.shape[:3]
        if g.shape[1] != B or Js.shape[:2] != (B, Cc):
            raise LaplaceHipError("jac_gconv: x [B, Cin, H, W], g [S, B, Do, ...] and Js [B, S, P] do not match")
        kh, kw = _pair(kernel_size)
        sh, sw = _pair(stride)
        ph, pw = _pair(padding)
        dh, dw = _pair(dilation)
        self._rc(
            self.lib.lk_jac_gconv_f32(_ptr(x), _ptr(g), B, Cc, Cin, H, W, Do, int(groups), kh, kw, sh, sw, ph, pw, dh, dw,
                                      _ptr(Js), Js.shape[-1], int(col0), int(bcol0), self._stream(x.device)),
            "lk_jac_gconv_f32",
        )

    # ---- nn.Embedding weights (csrc/lk_embed.hip) ----
    @staticmethod
    def _embed_operands(g, ids, what):
        """``(S, B, T, D)`` of a cotangent ``g [S, B, ..., D]`` and token ids ``ids [B, ...]`` (int64)"""
        _check(g, "g"), _check(ids, "ids", torch.int64)
        if g.dim() < 3 or ids.dim() < 1 or tuple(g.shape[1:-1]) != tuple(ids.shape):
            raise LaplaceHipError(f"{what}: g [S, B, ..., D] and ids [B, ...] do not match")
        T = 1
        for n in ids.shape[1:]:
            T *= int(n)
        return g.shape[0], ids.shape[0], T, g.shape[-1]

    def jac_embed(self, g, ids, V, padding_idx, Js, col0):
        """``Js[b, s, col0 + v*D + d] = sum_{t: ids[b, t] == v} g[s, b, t, d]``; every other element of ``Js [B, S, P]`` is left
        as it is.  The ids are sorted here (stable), the kernel finds the runs."""
        S, B, T, D = self._embed_operands(g, ids, "jac_embed")
        _check(Js, "Js")
        if Js.shape[:2] != (B, S):
            raise LaplaceHipError("jac_embed: Js must be [B, S, P]")
        sid, order = torch.sort(ids.reshape(-1), stable=True)
        pad = -1 if padding_idx is None else int(padding_idx)
        self._rc(self.lib.lk_jac_embed_f32(_ptr(g), _ptr(order), _ptr(sid), S, B, T, D, int(V), pad, _ptr(Js), Js.shape[-1],
                                           int(col0), self._stream(g.device)), "lk_jac_embed_f32")

    def diag_embed(self, g, ids, V, padding_idx, alpha, h):
        """``h[v*D + d] += alpha * sum_(s, b) (sum_{t: ids[b, t] == v} g[s, b, t, d])^2`` for ``h [V*D]``"""
        S, B, T, D = self._embed_operands(g, ids, "diag_embed")
        _check(h, "h")
        if h.numel() != int(V) * D:
            raise LaplaceHipError("diag_embed: h must hold V*D values")
        sid, order = torch.sort(ids.reshape(-1), stable=True)
        pad = -1 if padding_idx is None else int(padding_idx)
        self._rc(self.lib.lk_diag_embed_f32(_ptr(g), _ptr(order), _ptr(sid), S, B, T, D, int(V), pad, float(alpha), _ptr(h),
                                            self._stream(g.device)), "lk_diag_embed_f32")

    def diag_quadform_embed(self, g, ids, V, padding_idx, var, fvar):
        """``fvar[b, c, k] += sum_v sum_d r_c[d] r_k[d] var[v*D + d]`` with ``r_c`` the per-(sample, id) sum of ``g[c]``"""
        C, B, T, D = self._embed_operands(g, ids, "diag_quadform_embed")
        _check(var, "var"), _check(fvar, "fvar")
        if var.numel() != int(V) * D or tuple(fvar.shape) != (B, C, C):
            raise LaplaceHipError("diag_quadform_embed: var must hold V*D values and fvar be [B, C, C]")
        sid, order = torch.sort(ids.reshape(B, T), dim=1, stable=True)
        pad = -1 if padding_idx is None else int(padding_idx)
        self._rc(self.lib.lk_diag_quadform_embed_f32(_ptr(g), _ptr(order.contiguous()), _ptr(sid.contiguous()), C, B, T, D, int(V),
                                                     pad, _ptr(var), _ptr(fvar), self._stream(g.device)),
                 "lk_diag_quadform_embed_f32")
        return fvar

    def embed_variant(self, S, B, T, D, aligned=True):
        """lk_embed_variant: the vector class and the long-run split the embedding kernels take for a shape (host only), or
        ``None`` for a shape they refuse."""
        r = int(self.lib.lk_embed_variant(int(S), int(B), int(T), int(D), int(bool(aligned))))
        if r < 0:
            return None
        return {"vec": 4 if r & 1 else 1, "slots": (r >> 1) & 0x7FF, "lanes": (r >> 12) & 0xFF, "chunks": r >> 20}

    def jac_norm_affine(self, g, xhat, Ch, layout, Js, wcol0, bcol0=-1):
        """``Js[n, s, wcol0 + ch] = sum_l g * xhat``, ``Js[n, s, bcol0 + ch] = sum_l g`` for an affine normalisation
        layer; ``g`` is ``[S, B, Ch, ...]`` (``layout`` 0) or ``[S, B, ..., Ch]`` (``layout`` 1), ``xhat`` one sample
        batch ``[B, ...]`` in the same layout (csrc/lk_norm.hip)."""
        _check(g, "g"), _check(xhat, "xhat"), _check(Js, "Js")
        S, B = g.shape[:2]
        if xhat.numel() * S != g.numel() or xhat.shape[0] != B or Js.shape[:2] != (B, S):
            raise LaplaceHipError("jac_norm_affine: g [S, B, ...], xhat [B, ...] and Js [B, S, P] do not match")
        L = xhat.numel() // max(B * int(Ch), 1)
        if B * L * int(Ch) != xhat.numel():
            raise LaplaceHipError("jac_norm_affine: xhat is not [B, Ch, L] / [B, L, Ch]")
        self._rc(
            self.lib.lk_jac_norm_affine_f32(_ptr(g), _ptr(xhat), S, B, L, int(Ch), int(layout), _ptr(Js), Js.shape[-1],
                                            int(wcol0), int(bcol0), self._stream(g.device)),
            "lk_jac_norm_affine_f32",
        )

    def jac_norm_affine_nhwc(self, g: "SplitTensor", x, mu, rstd, S, Js, wcol0, bcol0=-1):
        """the same columns from the NHWC sweep's own cotangent (csrc/lk_normtap.hip): ``g`` the one-scale split tensor
        ``[S*B, .., Ch]``, ``x`` ``[B, .., Ch]`` fp32, ``xhat = (x - mu) * rstd`` formed in registers (``mu``, ``rstd`` ``[Ch]``, or
        both ``None``: ``x`` is ``xhat``)."""
        g_ptrs = _split_half(g, "jac_norm_affine_nhwc", "g", "an operand of the weight-sharing predictive; this kernel reads "
                             "position-major planes [S*B, .., Ch]")
        _check(x, "x"), _check(Js, "Js")
        S = int(S)
        if x.dim() < 2 or g.planes.dim() != x.dim() + 1 or S < 1 or g.planes.shape[1] != S * x.shape[0] \
                or tuple(g.planes.shape[2:]) != tuple(x.shape[1:]) or Js.dim() != 3 or tuple(Js.shape[:2]) != (x.shape[0], S):
            raise LaplaceHipError("jac_norm_affine_nhwc: g [S*B, .., Ch], x [B, .., Ch] and Js [B, S, P] do not match")
        B, Ch = x.shape[0], x.shape[-1]
        if (mu is None) != (rstd is None):
            raise LaplaceHipError("jac_norm_affine_nhwc: mu and rstd are given together or not at all")
        for name, t in (("mu", mu), ("rstd", rstd)):
            if t is not None and tuple(_check(t, name).shape) != (Ch,):
                raise LaplaceHipError(f"jac_norm_affine_nhwc: {name} must be [Ch]")
        L = x.numel() // max(B * Ch, 1)
        self._rc(
            self.lib.lk_jac_norm_affine_nhwc_f16x2(*g_ptrs, _ptr(x), _ptr(mu), _ptr(rstd),
                                                   S, B, max(L, 1), Ch, _ptr(Js), Js.shape[-1], int(wcol0), int(bcol0),
                                                   self._stream(x.device)),
            "lk_jac_norm_affine_nhwc_f16x2",
        )

    def normtap_variant(self, S, B, L, Ch, affine=True, aligned=True):
        """lk_normtap_variant: the path ``lk_jac_norm_affine_nhwc_f16x2`` takes for a shape (host only, no device call), or
        ``None`` for a shape it refuses."""
        r = int(self.lib.lk_normtap_variant(int(S), int(B), int(L), int(Ch), int(bool(affine)), int(bool(aligned))))
        if r < 0:
            return None
        return {"vec": (1, 4, 8)[r & 3], "seed_split": bool(r & 4), "affine": bool(r & 8), "seeds_per_pass": (r >> 4) & 0xF,
                "lane_rows": 1 << ((r >> 8) & 0xF), "seeds_per_slice": (r >> 12) & 0xFF, "channel_tiles": r >> 20}

    @staticmethod
    def _norm_geometry(x, B, G, layout, what):
        """``(L, Ch)`` of a per-sample normalisation over ``x`` = ``[B, Ch, L..]`` (layout 0) / ``[B, L.., Ch]`` (layout 1)"""
        if x.dim() < 2 or x.shape[0] != B:
            raise LaplaceHipError(f"{what}: expected [B, Ch, ...] / [B, ..., Ch]")
        Ch = int(x.shape[1] if layout == 0 else x.shape[-1])
        L = x.numel() // max(B * Ch, 1) if x.numel() else 1
        if G < 1 or Ch % G or layout not in (0, 1):
            raise LaplaceHipError(f"{what}: G must divide the {Ch} channels; layout is 0 or 1")
        return max(L, 1), Ch

    def norm_forward(self, x, w, b, G, layout, eps):
        """``(y, xhat, rstd)`` of a per-sample normalisation (csrc/lk_normvjp.hip): statistics over the rows ``(n, group)`` of
        ``x`` = ``[B, Ch, L..]`` (``layout`` 0) or ``[B, L.., Ch]`` (``layout`` 1), ``y = w[ch] * xhat + b[ch]`` (``w``, ``b``
        may be None), ``rstd`` ``[B, G]``.  nn.LayerNorm: ``x`` reshaped to ``[rows, D]``, layout 1, ``G = 1``."""
        _check(x, "x")
        B = x.shape[0]
        L, Ch = self._norm_geometry(x, B, int(G), int(layout), "norm_forward")
        for t, name in ((w, "w"), (b, "b")):
            if t is not None:
                _check(t, name)
                if t.numel() != Ch:
                    raise LaplaceHipError(f"norm_forward: {name} must have {Ch} elements")
        y, xhat = torch.empty_like(x), torch.empty_like(x)
        rstd = torch.empty(B, int(G), dtype=torch.float32, device=x.device)
        self._rc(self.lib.lk_norm_fwd_f32(_ptr(x), _ptr(w), _ptr(b), B, L, Ch, int(G), int(layout), float(eps), _ptr(y),
                                          _ptr(xhat), _ptr(rstd), self._stream(x.device)), "lk_norm_fwd_f32")
        return y, xhat, rstd

    def norm_vjp(self, g, xhat, rstd, w, S, G, layout, amax=None):
        """``dx`` of a per-sample normalisation for the ``S`` seeds stacked in ``g`` (``[S*B, ...]`` in the layout of ``xhat``
        ``[B, ...]``): ``t = w * g``, ``dx = rstd * (t - mean_row(t) - xhat * mean_row(t * xhat))``.  ``amax``: zeroed device
        word that receives the bit pattern of max|dx|."""
        _check(g, "g"), _check(xhat, "xhat"), _check(rstd, "rstd")
        B = xhat.shape[0]
        L, Ch = self._norm_geometry(xhat, B, int(G), int(layout), "norm_vjp")
        if g.numel() != int(S) * xhat.numel() or rstd.numel() != B * int(G):
            raise LaplaceHipError("norm_vjp: g [S*B, ...], xhat [B, ...] and rstd [B, G] do not match")
        if w is not None:
            _check(w, "w")
            if w.numel() != Ch:
                raise LaplaceHipError(f"norm_vjp: w must have {Ch} elements")
        _amax_word(amax, "norm_vjp")
        dx = torch.empty_like(g)
        self._rc(self.lib.lk_norm_vjp_f32(_ptr(g), _ptr(xhat), _ptr(rstd), _ptr(w), int(S), B, L, Ch, int(G), int(layout),
                                          _ptr(dx), _ptr(amax), self._stream(g.device)), "lk_norm_vjp_f32")
        return dx

    #: ``kernel`` of :meth:`norm_sweep_variant` (LK_NORMVJP_* of include/laplace_hip.h)
    NORMVJP_ROW, NORMVJP_TILE = 0, 1

    def norm_sweep_variant(self, S, B, L, Ch, G, layout, aligned=True):
        """lk_norm_sweep_variant: the kernel and path ``lk_norm_vjp_f32`` takes for a shape (host only, no device call), or
        ``None`` for a shape it refuses."""
        r = int(self.lib.lk_norm_sweep_variant(int(S), int(B), int(L), int(Ch), int(G), int(layout), int(bool(aligned))))
        if r < 0:
            return None
        return {"kernel": r & 1, "vec": bool(r & 2), "two_pass": bool(r & 4), "seed_split": bool(r & 8), "lanes": (r >> 4) & 0xFFF,
                "groups": r >> 16, "layout": int(layout)}

    def rmsnorm_forward(self, x2d, w, eps):
        """``(y, rstd)`` of nn.RMSNorm on ``x2d`` ``[rows, D]`` (csrc/lk_rmsnorm.hip): ``rstd = 1 / sqrt(mean_row(x^2) + eps)``
        ``[rows]``, ``y = w * x * rstd`` (``w`` ``[D]`` or None).  No ``xhat`` is stored: the VJP forms it from ``x`` and ``rstd``."""
        _check(x2d, "x")
        if x2d.dim() != 2 or x2d.shape[1] < 1:
            raise LaplaceHipError("rmsnorm_forward: x must be [rows, D] with D >= 1")
        rows, D = int(x2d.shape[0]), int(x2d.shape[1])
        if w is not None:
            _check(w, "w")
            if w.numel() != D:
                raise LaplaceHipError(f"rmsnorm_forward: w must have {D} elements")
        y = torch.empty_like(x2d)
        rstd = torch.empty(rows, dtype=torch.float32, device=x2d.device)
        if rows == 0:  # (an empty tensor has no address to hand over)
            return y, rstd
        self._rc(self.lib.lk_rmsnorm_fwd_f32(_ptr(x2d), _ptr(w), rows, D, float(eps), _ptr(y), _ptr(rstd),
                                             self._stream(x2d.device)), "lk_rmsnorm_fwd_f32")
        return y, rstd

    def rmsnorm_vjp(self, g, x2d, rstd, w, S, amax=None):
        """``dx`` of nn.RMSNorm for the ``S`` seeds stacked in ``g`` (``[S*rows, D]``, ``x2d`` ``[rows, D]``): ``t = w * g``,
        ``xh = x * rstd``, ``dx = rstd * (t - xh * mean_row(t * xh))``.  ``amax``: zeroed device word that receives the bit
        pattern of max|dx|."""
        _check(g, "g"), _check(x2d, "x"), _check(rstd, "rstd")
        if x2d.dim() != 2 or x2d.shape[1] < 1:
            raise LaplaceHipError("rmsnorm_vjp: x must be [rows, D] with D >= 1")
        rows, D = int(x2d.shape[0]), int(x2d.shape[1])
        if g.numel() != int(S) * x2d.numel() or rstd.numel() != rows:
            raise LaplaceHipError("rmsnorm_vjp: g [S*rows, D], x [rows, D] and rstd [rows] do not match")
        if w is not None:
            _check(w, "w")
            if w.numel() != D:
                raise LaplaceHipError(f"rmsnorm_vjp: w must have {D} elements")
        _amax_word(amax, "rmsnorm_vjp")
        dx = torch.empty_like(g)
        if rows == 0:
            return dx
        self._rc(self.lib.lk_rmsnorm_vjp_f32(_ptr(g), _ptr(x2d), _ptr(rstd), _ptr(w), int(S), rows, D, _ptr(dx), _ptr(amax),
                                             self._stream(g.device)), "lk_rmsnorm_vjp_f32")
        return dx

    def rmsnorm_variant(self, S, rows, D, aligned=True):
        """lk_rmsnorm_variant: the path ``lk_rmsnorm_vjp_f32`` takes for a shape (host only, no device call), or ``None`` for a
        shape it refuses."""
        r = int(self.lib.lk_rmsnorm_variant(int(S), int(rows), int(D), int(bool(aligned))))
        if r < 0:
            return None
        return {"vec": bool(r & 1), "two_pass": bool(r & 2), "seed_split": bool(r & 4), "lanes": 1 << ((r >> 3) & 7),
                "seeds_per_slice": r >> 6}

    #: largest ``T`` whose probability block stays in LDS over the seeds (LK_ATTN_RESIDENT_MAX_T of include/laplace_hip.h)
    ATTN_RESIDENT_MAX_T = 256

    @staticmethod
    def _attn_operands(what, *named):
        """``(layout, tensors)`` of attention operands ``[N, H, T, D]`` for csrc/lk_attn.hip: as they are when all lie in the
        same one of the two layouts (0: contiguous, 1: ``transpose(1, 2)`` contiguous), else contiguous copies"""
        from .sweep import attn_operands

        for t, name in named:
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4:
                raise LaplaceHipError(f"{what}: {name} must be a 4-d fp32 tensor on a ROCm device (no CPU path)")
        return attn_operands(*(t for t, _ in named))

    def attn_forward(self, q, k, v, scale, causal):
        """``(o, lse)`` of scaled dot-product self-attention (csrc/lk_attn.hip) on ``q``, ``k``, ``v`` ``[B, H, T, D]``:
        ``o = softmax(scale q k^T (+ causal mask)) v`` as a ``[B, H, T, D]`` view in the operands' layout, ``lse`` ``[B, H, T]``.
        The layout is read off the strides; operands in neither layout, or in different ones, are made contiguous."""
        layout, (q, k, v) = self._attn_operands("attn_forward", (q, "q"), (k, "k"), (v, "v"))
        if not (q.shape == k.shape == v.shape):
            raise LaplaceHipError("attn_forward: q, k and v must have equal shapes (self-attention)")
        from .sweep import attn_like

        B, H, T, D = q.shape
        o = attn_like(q.shape, layout, q)
        lse = torch.empty(B, H, T, dtype=torch.float32, device=q.device)
        self._rc(self.lib.lk_attn_fwd_f32(_ptr(q), _ptr(k), _ptr(v), B, H, T, D, layout, float(scale), int(bool(causal)),
                                          _ptr(o), _ptr(lse), self._stream(q.device)), "lk_attn_fwd_f32")
        return o, lse

    def attn_vjp(self, go, q, k, v, o, lse, S, scale, causal):
        """``(dq, dk, dv)``, each a ``[S*B, H, T, D]`` view in the operands' layout, for the ``S`` seeds stacked in ``go``
        ``[S*B, H, T, D]`` from ONE ``q``, ``k``, ``v``, ``o`` ``[B, H, T, D]`` and ``lse`` ``[B, H, T]`` per sample
        (lk_attn_vjp_f32; the wrapper allocates the workspace)."""
        layout, (q, k, v, o) = self._attn_operands("attn_vjp", (q, "q"), (k, "k"), (v, "v"), (o, "o"))
        from .sweep import attn_layout, attn_like

        B, H, T, D = q.shape
        S = int(S)
        _check(lse, "lse")
        if tuple(go.shape) != (S * B, H, T, D) or not (q.shape == k.shape == v.shape == o.shape) or lse.numel() != B * H * T:
            raise LaplaceHipError("attn_vjp: go [S*B, H, T, D], q / k / v / o [B, H, T, D] and lse [B, H, T] do not match")
        self._attn_operands("attn_vjp", (go, "go"))
        if attn_layout(go) != layout:  # (the cotangent in the operands' layout: one copy, only when it arrives otherwise)
            go = go.contiguous() if layout == 0 else go.transpose(1, 2).contiguous().transpose(1, 2)
        dq, dk, dv = (attn_like(go.shape, layout, go) for _ in range(3))
        nbytes = int(self.lib.lk_attn_vjp_workspace_bytes(S, B, H, T, D))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=go.device)
        self._rc(self.lib.lk_attn_vjp_f32(_ptr(go), _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse), S, B, H, T, D, layout,
                                          float(scale), int(bool(causal)), _ptr(dq), _ptr(dk), _ptr(dv), _ptr(ws), ws.numel(),
                                          self._stream(go.device)), "lk_attn_vjp_f32")
        return dq, dk, dv

    @staticmethod
    def _attn_strided(what, shape, *named):
        """the common row stride (in floats) of ``[N, T, H, D]`` fp32 device views whose rows of ``H D`` floats are contiguous and
        ``ld`` apart - the slices of a packed ``[N, T, 3 H D]`` projection, or contiguous tensors (``ld = H D``)"""
        N, T, H, D = shape
        lds = set()
        for t, name in named:
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
                raise LaplaceHipError(f"{what}: {name} must be a fp32 tensor {tuple(shape)} on a ROCm device (no CPU path)")
            sn, st, sh, sd = t.stride()
            if (D > 1 and sd != 1) or (H > 1 and sh != D) or (N > 1 and T > 0 and sn != T * st):
                raise LaplaceHipError(f"{what}: {name} must be a [N, T, H, D] view with contiguous rows of H * D floats and "
                                      f"a batch stride of T rows (strides {t.stride()})")
            lds.add(int(st) if T > 1 or N > 1 else H * D)
        if len(lds) != 1:
            raise LaplaceHipError(f"{what}: {', '.join(n for _, n in named)} must share one row stride (got {sorted(lds)})")
        return lds.pop()

    def attn_forward_strided(self, q, k, v, scale, causal):
        """``(o, lse)`` of lk_attn_fwd_strided_f32 on ``q``, ``k``, ``v`` ``[B, T, H, D]``: views with one row stride, such as
        ``qkv.view(B, T, 3, H, D).unbind(2)`` of a packed projection - read where they lie, no copy.  ``o``: ``[B, T, H, D]``
        contiguous (``o.view(B, T, H * D)`` feeds the output projection), ``lse``: ``[B, H, T]``."""
        B, T, H, D = q.shape
        ldq = self._attn_strided("attn_forward_strided", q.shape, (q, "q"), (k, "k"), (v, "v"))
        o = torch.empty(B, T, H, D, dtype=torch.float32, device=q.device)
        lse = torch.empty(B, H, T, dtype=torch.float32, device=q.device)
        self._rc(self.lib.lk_attn_fwd_strided_f32(_ptr(q), _ptr(k), _ptr(v), ldq, B, H, T, D, float(scale), int(bool(causal)),
                                                  _ptr(o), _ptr(lse), self._stream(q.device)), "lk_attn_fwd_strided_f32")
        return o, lse

    def attn_vjp_strided(self, go, q, k, v, o, lse, S, scale, causal, dq, dk, dv):
        """lk_attn_vjp_strided_f32: writes the cotangents of all ``S`` seeds into the caller's ``dq``, ``dk``, ``dv``
        ``[S*B, T, H, D]`` - views with one row stride, such as ``dqkv.view(S * B, T, 3, H, D).unbind(2)`` of the ``[S*B, T, 3 H D]``
        buffer that the packed projection's VJP reads (every element of the three is written).  ``go`` ``[S*B, T, H, D]`` and ``o``
        ``[B, T, H, D]`` contiguous, ``q``, ``k``, ``v`` as `attn_forward_strided` takes them, ``lse`` ``[B, H, T]``."""
        B, T, H, D = q.shape
        S = int(S)
        what = "attn_vjp_strided"
        ldq = self._attn_strided(what, q.shape, (q, "q"), (k, "k"), (v, "v"))
        ldd = self._attn_strided(what, (S * B, T, H, D), (dq, "dq"), (dk, "dk"), (dv, "dv"))
        _check(lse, "lse")
        if self._attn_strided(what, q.shape, (o, "o")) != H * D or self._attn_strided(what, (S * B, T, H, D), (go, "go")) != H * D:
            raise LaplaceHipError(f"{what}: go and o must be contiguous")
        if lse.numel() != B * H * T:
            raise LaplaceHipError(f"{what}: lse must be [B, H, T]")
        nbytes = int(self.lib.lk_attn_vjp_workspace_bytes(S, B, H, T, D))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=go.device)
        self._rc(self.lib.lk_attn_vjp_strided_f32(_ptr(go), _ptr(q), _ptr(k), _ptr(v), ldq, _ptr(o), _ptr(lse), S, B, H, T, D,
                                                  float(scale), int(bool(causal)), _ptr(dq), _ptr(dk), _ptr(dv), ldd, _ptr(ws),
                                                  ws.numel(), self._stream(go.device)), "lk_attn_vjp_strided_f32")

    def attn_variant(self, S, B, H, T, D, layout=0, causal=False):
        """lk_attn_variant: the path ``lk_attn_vjp_f32`` takes for a shape (host only, no device call), or ``None`` for a
        shape the entry points refuse."""
        r = int(self.lib.lk_attn_variant(int(S), int(B), int(H), int(T), int(D), int(layout), int(bool(causal))))
        if r < 0:
            return None
        return {"resident": bool(r & 1), "seed_split": bool(r & 2), "dp": 16 << ((r >> 2) & 3), "causal": bool(r & 16),
                "layout": (r >> 5) & 1, "seeds_per_slice": (r >> 8) & 0xFF, "owner_blocks": r >> 16}

    #: ``kind`` of the pooling entry points (LK_POOL_* of include/laplace_hip.h)
    POOL_MAX, POOL_AVG = 0, 1

    @staticmethod
    def _pool_geometry(kind, kernel, stride, padding, what):
        """``(kh, kw, sh, sw, ph, pw)`` as ints (``stride`` None / empty: the kernel size, as torch)"""
        if kind not in (0, 1):
            raise LaplaceHipError(f"{what}: kind is POOL_MAX (0) or POOL_AVG (1)")
        kh, kw = _pair(kernel)
        sh, sw = (kh, kw) if stride is None or stride == [] or stride == () else _pair(stride)
        ph, pw = _pair(padding)
        return kh, kw, sh, sw, ph, pw

    def pool_forward(self, x_nhwc, kind, kernel, stride, padding, count_include_pad=True, divisor_override=None):
        """``(y, arg)`` of a max / average pooling over the fp32 NHWC map ``x_nhwc`` ``[B, H, W, C]`` (csrc/lk_pool.hip,
        ``ceil_mode`` false): ``y`` ``[B, OH, OW, C]``; ``arg`` (max only, else None) uint8 ``[B, OH, OW, C]``, the window-local tap
        code ``dy * kw + dx`` of the first maximum in row-major order (torch's tie rule)."""
        _check(x_nhwc, "x_nhwc")
        if x_nhwc.dim() != 4:
            raise LaplaceHipError("pool_forward: expected an NHWC map [B, H, W, C]")
        kh, kw, sh, sw, ph, pw = self._pool_geometry(kind, kernel, stride, padding, "pool_forward")
        B, H, W, C = x_nhwc.shape
        if min(kh, kw, sh, sw) < 1 or H + 2 * ph < kh or W + 2 * pw < kw:
            raise LaplaceHipError(f"pool_forward: window ({kh}, {kw}) / stride ({sh}, {sw}) / padding ({ph}, {pw}) leaves no "
                                  f"output on a {H} x {W} map")
        OH, OW = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
        y = torch.empty(B, OH, OW, C, dtype=torch.float32, device=x_nhwc.device)
        arg = torch.empty(B, OH, OW, C, dtype=torch.uint8, device=x_nhwc.device) if kind == self.POOL_MAX else None
        self._rc(self.lib.lk_pool_fwd_nhwc_f32(int(kind), _ptr(x_nhwc), B, H, W, C, kh, kw, sh, sw, ph, pw,
                                               int(bool(count_include_pad)), int(divisor_override or 0), _ptr(y), _ptr(arg),
                                               self._stream(x_nhwc.device)), "lk_pool_fwd_nhwc_f32")
        return y, arg

    def pool_vjp(self, g, arg, S, in_hw, kind, kernel, stride, padding, count_include_pad=True, divisor_override=None,
                 amax=None):
        """``dx`` ``[S*B, H, W, C]`` of a pooling layer for the ``S`` seeds stacked in ``g`` ``[S*B, OH, OW, C]``; ``in_hw`` =
        ``(H, W)``; ``arg`` ``[B, OH, OW, C]`` from :meth:`pool_forward` (None for the average), shared by all seeds.  ``amax``:
        zeroed device word that receives the bit pattern of max|dx|."""
        _check(g, "g")
        kh, kw, sh, sw, ph, pw = self._pool_geometry(kind, kernel, stride, padding, "pool_vjp")
        S, (H, W) = int(S), (int(in_hw[0]), int(in_hw[1]))
        if g.dim() != 4 or S < 1 or g.shape[0] % S:
            raise LaplaceHipError("pool_vjp: g must be [S*B, OH, OW, C]")
        B, C = g.shape[0] // S, g.shape[3]
        if min(kh, kw, sh, sw) < 1 or H + 2 * ph < kh or W + 2 * pw < kw \
                or tuple(g.shape[1:3]) != ((H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1):
            raise LaplaceHipError(f"pool_vjp: g {tuple(g.shape)} is not the pooled {H} x {W} map of window ({kh}, {kw}), stride "
                                  f"({sh}, {sw}), padding ({ph}, {pw})")
        if kind == self.POOL_MAX:
            _check(arg, "arg", torch.uint8)
            if tuple(arg.shape) != (B, *g.shape[1:]):
                raise LaplaceHipError("pool_vjp: arg must be [B, OH, OW, C]")
        elif arg is not None:
            raise LaplaceHipError("pool_vjp: the average takes no arg")
        _amax_word(amax, "pool_vjp")
        dx = torch.empty(S * B, H, W, C, dtype=torch.float32, device=g.device)
        self._rc(self.lib.lk_pool_vjp_nhwc_f32(int(kind), _ptr(g), _ptr(arg), S, B, H, W, C, kh, kw, sh, sw, ph, pw,
                                               int(bool(count_include_pad)), int(divisor_override or 0), _ptr(dx), _ptr(amax),
                                               self._stream(g.device)), "lk_pool_vjp_nhwc_f32")
        return dx

    def pool_variant(self, kind, S, B, H, W, C, kernel, stride, padding, aligned=True):
        """lk_pool_variant: the path ``lk_pool_vjp_nhwc_f32`` takes for a shape (host only, no device call), or ``None`` for a
        shape it refuses."""
        kh, kw, sh, sw, ph, pw = self._pool_geometry(kind, kernel, stride, padding, "pool_variant")
        r = int(self.lib.lk_pool_variant(int(kind), int(S), int(B), int(H), int(W), int(C), kh, kw, sh, sw, ph, pw,
                                         int(bool(aligned))))
        if r < 0:
            return None
        return {"vec": bool(r & 1), "summing": bool(r & 2), "seed_split": bool(r & 4), "seeds_per_pass": (r >> 4) & 0xFF,
                "seeds_per_slice": r >> 12}

    #: most cotangent parts one launch of lk_cat_vjp_nhwc_f32 sums (LK_CAT_MAX_PARTS of include/laplace_hip.h)
    CAT_MAX_PARTS = 4

    def cat_forward(self, sources_nhwc):
        """``y`` ``[B, H, W, sum C_j]``: the fp32 NHWC maps ``[B, H, W, C_j]`` concatenated along the channels into ONE
        allocation, one launch of lk_cat_fwd_nhwc_f32 per source (csrc/lk_cat.hip)"""
        sources = list(sources_nhwc)
        if not sources:
            raise LaplaceHipError("cat_forward: no source")
        for j, x in enumerate(sources):
            _check(x, f"sources_nhwc[{j}]")
            if x.dim() != 4 or x.shape[3] < 1:
                raise LaplaceHipError("cat_forward: expected NHWC maps [B, H, W, C] with C >= 1")
            if tuple(x.shape[:3]) != tuple(sources[0].shape[:3]) or x.device != sources[0].device:
                raise LaplaceHipError(f"cat_forward: source {j} {tuple(x.shape)} does not lie on the pixels of source 0 "
                                      f"{tuple(sources[0].shape)}")
        B, H, W = (int(d) for d in sources[0].shape[:3])
        Ct = sum(int(x.shape[3]) for x in sources)
        y = torch.empty(B, H, W, Ct, dtype=torch.float32, device=sources[0].device)
        st, c0 = self._stream(y.device), 0
        for x in sources:
            Cs = int(x.shape[3])
            self._rc(self.lib.lk_cat_fwd_nhwc_f32(_ptr(x), B * H * W, Cs, _ptr(y), Ct, c0, st), "lk_cat_fwd_nhwc_f32")
            c0 += Cs
        return y

    def cat_vjp(self, parts, c0, Cs, amax=None):
        """``dx`` ``[N, H, W, Cs]``: channels ``[c0, c0 + Cs)`` of the fp32 sum, in the listed order, of 1 to ``CAT_MAX_PARTS``
        cotangent parts ``[N, H, W, Ct]`` - fp32 NHWC tensors or one-scale :class:`SplitTensor` s - in ONE launch of
        lk_cat_vjp_nhwc_f32.  ``amax``: zeroed device word that receives the bit pattern of max|dx|."""
        parts = list(parts)
        if not 1 <= len(parts) <= self.CAT_MAX_PARTS:
            raise LaplaceHipError(f"cat_vjp: 1 to {self.CAT_MAX_PARTS} parts, got {len(parts)}")
        shape, dev = tuple(parts[0].shape), None
        arrays = [(ctypes.c_void_p * len(parts))() for _ in range(4)]  # f32, hi, lo, sexp
        for j, p in enumerate(parts):
            ptrs, pshape, pdev = _split_operand(p, "cat_vjp", f"parts[{j}]", "no NHWC map")
            for a, ptr in zip(arrays, ptrs):
                a[j] = ptr
            if len(shape) != 4 or pshape != shape or (dev is not None and pdev != dev):
                raise LaplaceHipError(f"cat_vjp: part {j} {tuple(p.shape)} is not an NHWC map [N, H, W, Ct] like part 0 {shape}")
            dev = pdev
        c0, Cs = int(c0), int(Cs)
        N, H, W, Ct = (int(d) for d in shape)
        if Cs < 1 or c0 < 0 or c0 + Cs > Ct:
            raise LaplaceHipError(f"cat_vjp: channels [{c0}, {c0 + Cs}) are no slice of {Ct} channels")
        _amax_word(amax, "cat_vjp")
        dx = torch.empty(N, H, W, Cs, dtype=torch.float32, device=dev)
        self._rc(self.lib.lk_cat_vjp_nhwc_f32(len(parts), *(ctypes.addressof(a) for a in arrays), N * H * W, Ct, c0, Cs, _ptr(dx),
                                              _ptr(amax), self._stream(dev)), "lk_cat_vjp_nhwc_f32")
        return dx

    def cat_variant(self, nparts, split_mask, R, Ct, c0, Cs, aligned=True):
        """lk_cat_variant: the path ``lk_cat_vjp_nhwc_f32`` takes for a shape (host only, no device call), or ``None`` for a
        shape it refuses.  ``split_mask``: bit ``p`` set when part ``p`` is a split tensor."""
        r = int(self.lib.lk_cat_variant(int(nparts), int(split_mask), int(R), int(Ct), int(c0), int(Cs), int(bool(aligned))))
        if r < 0:
            return None
        return {"vec": bool(r & 1), "nparts": (r >> 1) & 7, "split_mask": (r >> 4) & 15, "wide_index": bool(r & 256),
                "blocks": r >> 12}

    #: most pieces one launch of lk_slice_vjp_f32 sums (LK_SLICE_MAX_PIECES of include/laplace_hip.h)
    SLICE_MAX_PIECES = 8

    def slice_forward(self, x, R, Ct, c0, Cs):
        """``y`` ``[R, Cs]``: columns ``[c0, c0 + Cs)`` of the contiguous fp32 tensor ``x`` read as the row matrix ``[R, Ct]``, in
        one launch of lk_slice_fwd_f32 (csrc/lk_slice.hip)"""
        _check(x, "x")
        R, Ct, c0, Cs = int(R), int(Ct), int(c0), int(Cs)
        if R < 0 or Ct < 1 or x.numel() != R * Ct:
            raise LaplaceHipError(f"slice_forward: x {tuple(x.shape)} is no row matrix [{R}, {Ct}]")
        if Cs < 1 or c0 < 0 or c0 + Cs > Ct:
            raise LaplaceHipError(f"slice_forward: columns [{c0}, {c0 + Cs}) are no slice of {Ct} columns")
        y = torch.empty(R, Cs, dtype=torch.float32, device=x.device)
        self._rc(self.lib.lk_slice_fwd_f32(_ptr(x), R, Ct, c0, Cs, _ptr(y), self._stream(x.device)), "lk_slice_fwd_f32")
        return y

    def slice_vjp(self, pieces, R, Ct, amax=None):
        """``dx`` ``[R, Ct]``: per column the fp32 sum, in the listed order, of the pieces ``(value, c0, cs)`` that cover it - ``value``
        a contiguous fp32 tensor or a one-scale :class:`SplitTensor` of ``R * cs`` elements, the columns ``[c0, c0 + cs)`` - and
        ``+0.0`` where none does, in ONE launch of lk_slice_vjp_f32.  ``amax``: zeroed device word that receives the bit pattern
        of max|dx|."""
        pieces = list(pieces)
        if not 1 <= len(pieces) <= self.SLICE_MAX_PIECES:
            raise LaplaceHipError(f"slice_vjp: 1 to {self.SLICE_MAX_PIECES} pieces, got {len(pieces)}")
        R, Ct, n, dev = int(R), int(Ct), len(pieces), None
        arrays = [(ctypes.c_void_p * n)() for _ in range(4)]  # f32, hi, lo, sexp
        c0s, css = (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)()
        for j, (p, c0, cs) in enumerate(pieces):
            c0, cs = int(c0), int(cs)
            if cs < 1 or c0 < 0 or c0 + cs > Ct:
                raise LaplaceHipError(f"slice_vjp: piece {j}: columns [{c0}, {c0 + cs}) are no slice of {Ct} columns")
            ptrs, pshape, pdev = _split_operand(p, "slice_vjp", f"pieces[{j}]", "no row matrix")
            for a, ptr in zip(arrays, ptrs):
                a[j] = ptr
            if pshape.numel() != R * cs or (dev is not None and pdev != dev):
                raise LaplaceHipError(f"slice_vjp: piece {j} {tuple(p.shape)} is no row matrix [{R}, {cs}]")
            c0s[j], css[j], dev = c0, cs, pdev
        _amax_word(amax, "slice_vjp")
        dx = torch.empty(R, Ct, dtype=torch.float32, device=dev)
        self._rc(self.lib.lk_slice_vjp_f32(n, *(ctypes.addressof(a) for a in arrays), ctypes.addressof(c0s), ctypes.addressof(css),
                                           R, Ct, _ptr(dx), _ptr(amax), self._stream(dev)), "lk_slice_vjp_f32")
        return dx

    def slice_variant(self, split_mask, c0, cs, R, Ct, aligned=True):
        """lk_slice_variant: the path ``lk_slice_vjp_f32`` takes for the pieces ``(c0[p], cs[p])`` (host only, no device call),
        or ``None`` for a shape it refuses.  ``split_mask``: bit ``p`` set when piece ``p`` is a split tensor."""
        n = len(c0)
        c0s, css = (ctypes.c_int64 * max(n, 1))(*[int(v) for v in c0]), (ctypes.c_int64 * max(n, 1))(*[int(v) for v in cs])
        r = int(self.lib.lk_slice_variant(n, int(split_mask), ctypes.addressof(c0s), ctypes.addressof(css), int(R), int(Ct),
                                          int(bool(aligned))))
        if r < 0:
            return None
        return {"vec": bool(r & 1), "npieces": (r >> 1) & 15, "split_mask": (r >> 5) & 255, "wide_index": bool(r & (1 << 13)),
                "blocks": r >> 14}

    def maxred_forward(self, x, outer, L, inner):
        """``(y, idx, cnt)``, each ``[outer, inner]``, of the contiguous fp32 ``x`` read as ``[outer, L, inner]``: the maximum over
        ``L``, the first position that holds it and how many positions compare equal to it (int32), in one launch of
        lk_maxred_fwd_f32 (csrc/lk_reduce.hip)"""
        _check(x, "x")
        outer, L, inner = int(outer), int(L), int(inner)
        if outer < 0 or L < 1 or inner < 1 or x.numel() != outer * L * inner:
            raise LaplaceHipError(f"maxred_forward: x {tuple(x.shape)} is no [{outer}, {L}, {inner}] operand")
        y = torch.empty(outer, inner, dtype=torch.float32, device=x.device)
        idx = torch.empty(outer, inner, dtype=torch.int32, device=x.device)
        cnt = torch.empty(outer, inner, dtype=torch.int32, device=x.device)
        if outer == 0:  # (an empty tensor has no address to hand over)
            return y, idx, cnt
        self._rc(self.lib.lk_maxred_fwd_f32(_ptr(x), outer, L, inner, _ptr(y), _ptr(idx), _ptr(cnt), self._stream(x.device)),
                 "lk_maxred_fwd_f32")
        return y, idx, cnt

    def maxred_vjp(self, g, S, outer, L, inner, idx=None, x=None, y=None, cnt=None):
        """``dx`` ``[S, outer, L, inner]`` of a maximum over ``L`` for the ``S`` seeds stacked in ``g`` ``[S, outer, inner]``, in ONE
        launch of lk_maxred_vjp_f32 that writes every element: with ``idx`` alone the cotangent goes to the first maximum
        (``max(dim)``, the adaptive max pools), with ``x``, ``y`` and ``cnt`` it is split evenly over the maxima (``amax``)"""
        _check(g, "g")
        S, outer, L, inner = int(S), int(outer), int(L), int(inner)
        even = x is not None or y is not None or cnt is not None
        if even:
            if x is None or y is None or cnt is None:
                raise LaplaceHipError("maxred_vjp: the even split needs x, y and cnt")
            _check(x, "x"), _check(y, "y"), _check(cnt, "cnt", torch.int32)
            idx = None
        else:
            if idx is None:
                raise LaplaceHipError("maxred_vjp: give idx (first maximum) or x, y and cnt (even split)")
            _check(idx, "idx", torch.int32)
        if S < 1 or outer < 0 or L < 1 or inner < 1 or g.numel() != S * outer * inner:
            raise LaplaceHipError(f"maxred_vjp: g {tuple(g.shape)} is no [{S}, {outer}, {inner}] cotangent")
        for t, n, name in ((idx, outer * inner, "idx"), (y, outer * inner, "y"), (cnt, outer * inner, "cnt"), (x, outer * L * inner, "x")):
            if t is not None and t.numel() != n:
                raise LaplaceHipError(f"maxred_vjp: {name} has {t.numel()} elements, expected {n}")
        dx = torch.empty(S, outer, L, inner, dtype=torch.float32, device=g.device)
        if outer == 0:
            return dx
        self._rc(self.lib.lk_maxred_vjp_f32(_ptr(g), _ptr(idx), _ptr(x), _ptr(y), _ptr(cnt), S, outer, L, inner, _ptr(dx),
                                            self._stream(g.device)), "lk_maxred_vjp_f32")
        return dx

    def reduce_variant(self, vjp, S, outer, L, inner, even=False, aligned=True):
        """lk_reduce_variant: the path ``lk_maxred_fwd_f32`` (``vjp`` false) or ``lk_maxred_vjp_f32`` takes for a shape (host only,
        no device call), or ``None`` for a shape they refuse."""
        r = int(self.lib.lk_reduce_variant(int(bool(vjp)), int(S), int(outer), int(L), int(inner), int(bool(even)),
                                           int(bool(aligned))))
        if r < 0:
            return None
        return {"vjp": bool(vjp), "row": bool(r & 1), "vec": bool(r & 2), "even": bool(r & 4), "wide_index": bool(r & 8),
                "lanes": 1 << ((r >> 4) & 7), "seed_split": bool(r & 128), "blocks": r >> 8}

    RESAMPLE_MAX_TAPS = 16  # (LK_RESAMPLE_MAX_TAPS of the header)

    def resample_pack(self, ptr, idx, w, L, OL):
        """the transposed tap lists of ONE axis of a static resampling (``sweep.resample_tables``: ``ptr`` ``[L + 1]`` int32, ``idx``
        int32, ``w`` float32) as lk_resample_vjp_f32 reads them, validated here ONCE - the entry point does not look into device
        tables: ``ptr`` rises from 0 to ``nnz``, at most ``RESAMPLE_MAX_TAPS`` taps per input, every ``idx`` an output ``0 <= idx <
        OL``, ascending within a list.  Returns ``(ptr, idx, w, L, OL, longest list)`` with contiguous device tensors (an axis with
        no tap at all carries one unused entry: an empty tensor has no address to hand over)."""
        L, OL = int(L), int(OL)
        for t, name, dt in ((ptr, "ptr", torch.int32), (idx, "idx", torch.int32), (w, "w", torch.float32)):
            _check(t, name, dt)
        p = ptr.to("cpu", torch.int64)
        nnz = int(idx.numel())
        if L < 1 or OL < 1 or p.numel() != L + 1 or w.numel() != nnz:
            raise LaplaceHipError(f"resample_pack: ptr [{p.numel()}], idx [{nnz}], w [{w.numel()}] are no tap lists of {L} inputs")
        cnt = p[1:] - p[:-1]
        if int(p[0]) != 0 or int(p[-1]) != nnz or bool((cnt < 0).any()):
            raise LaplaceHipError("resample_pack: ptr must rise from 0 to the number of taps")
        taps = int(cnt.max())
        if taps > self.RESAMPLE_MAX_TAPS:
            raise LaplaceHipError(f"resample_pack: {taps} taps for one input exceed LK_RESAMPLE_MAX_TAPS = {self.RESAMPLE_MAX_TAPS}")
        if nnz:
            i = idx.to("cpu", torch.int64)
            first = torch.zeros(nnz, dtype=torch.bool)
            first[p[:-1][cnt > 0]] = True
            if bool((i < 0).any()) or bool((i >= OL).any()) or bool(((i[1:] <= i[:-1]) & ~first[1:]).any()):
                raise LaplaceHipError(f"resample_pack: idx must lie in [0, {OL}) and ascend within the list of an input")
        else:
            idx, w = idx.new_zeros(1), w.new_zeros(1)
        return ptr, idx, w, L, OL, taps

    def resample_vjp(self, g, axis_h, axis_w):
        """``dx`` ``[P, H, W]`` of a static separable resampling for the ``P = S B C`` planes of the contiguous fp32 cotangent ``g``
        ``[P, OH, OW]``, in ONE launch of lk_resample_vjp_f32 (csrc/lk_resample.hip) that writes every element: ``axis_h`` /
        ``axis_w`` are what :meth:`resample_pack` returned for the two axes"""
        _check(g, "g")
        (ph, ih, wh, H, OH, _), (pw, iw, ww, W, OW, _) = axis_h, axis_w
        if g.dim() != 3 or tuple(g.shape[1:]) != (OH, OW) or g.shape[0] < 1:
            raise LaplaceHipError(f"resample_vjp: g {tuple(g.shape)} is no [P >= 1, {OH}, {OW}] cotangent")
        if any(t.device != g.device for t in (ph, ih, wh, pw, iw, ww)):
            raise LaplaceHipError("resample_vjp: the tap lists are on another device than g")
        P = int(g.shape[0])
        dx = torch.empty(P, H, W, dtype=torch.float32, device=g.device)
        self._rc(self.lib.lk_resample_vjp_f32(_ptr(g), P, OH, OW, H, W, _ptr(ph), _ptr(ih), _ptr(wh), _ptr(pw), _ptr(iw), _ptr(ww),
                                              _ptr(dx), self._stream(g.device)), "lk_resample_vjp_f32")
        return dx

    def resample_variant(self, P, OH, OW, H, W, taps_h, taps_w, aligned=True):
        """lk_resample_variant: the path ``lk_resample_vjp_f32`` takes for a shape and the longest tap list of each axis (host only,
        no device call), or ``None`` for what it refuses."""
        r = int(self.lib.lk_resample_variant(int(P), int(OH), int(OW), int(H), int(W), int(taps_h), int(taps_w), int(bool(aligned))))
        if r < 0:
            return None
        return {"vec": bool(r & 1), "taps_in_registers": bool(r & 2), "wide_index": bool(r & 4), "plane_split": bool(r & 8),
                "grid_stride": bool(r & 16), "packed_slices": bool(r & 32), "blocks": r >> 8}

    def mul_vjp(self, g, a, b, S, b_row, want=(True, True)):
        """``(da, db)`` of ``out = a * b`` for the ``S`` seeds stacked in the cotangent ``g`` (``S * a.numel()`` elements, seed-major)
        from ONE ``a`` and ``b`` per sample, in ONE launch of lk_mul_vjp_f32 (csrc/lk_mul.hip).  ``b_row`` false: ``b`` has the
        shape of ``a``, ``da = g * b`` and ``db = g * a``, both of the shape of ``g``.  ``b_row`` true: ``b`` is a row gate with one
        value per row of ``a`` read as ``[R = b.numel(), L]``; ``da = g * b[r]`` and ``db[s, r] = sum_l g[s, r, l] * a[r, l]``, of
        shape ``[S * b.shape[0], *b.shape[1:]]``.  ``want``: which of the two to compute (``None`` stands for the other)."""
        _check(g, "g"), _check(a, "a"), _check(b, "b")
        S, b_row, want_da, want_db = int(S), bool(b_row), bool(want[0]), bool(want[1])
        R = b.numel() if b_row else (a.shape[0] if a.dim() else 1)  # (full form: any split of a.numel() into rows serves)
        L = a.numel() // R if R else 1
        if S < 1 or not (want_da or want_db) or g.numel() != S * a.numel() or R * L != a.numel() or (not b_row and b.numel() != a.numel()):
            raise LaplaceHipError(f"mul_vjp: g {tuple(g.shape)}, a {tuple(a.shape)}, b {tuple(b.shape)} do not belong together for "
                                  f"S = {S}, b_row = {b_row}, want = {tuple(want)}")
        if a.device != g.device or b.device != g.device:
            raise LaplaceHipError("mul_vjp: g, a and b are on different devices")
        da = torch.empty_like(g) if want_da else None
        db = None
        if want_db:
            db = torch.empty((S * b.shape[0], *b.shape[1:]), dtype=torch.float32, device=g.device) if b_row else torch.empty_like(g)
        self._rc(self.lib.lk_mul_vjp_f32(_ptr(g), _ptr(a), _ptr(b), S, R, L, int(b_row), _ptr(da), _ptr(db),
                                         self._stream(g.device)), "lk_mul_vjp_f32")
        return da, db

    def mul_variant(self, S, R, L, b_row, want=(True, True), aligned=True):
        """lk_mul_variant: the path ``lk_mul_vjp_f32`` takes for a shape (host only, no device call), or ``None`` for a shape it
        refuses"""
        r = int(self.lib.lk_mul_variant(int(S), int(R), int(L), int(b_row), int(bool(want[0])), int(bool(want[1])), int(bool(aligned))))
        if r < 0:
            return None
        return {"row": bool(r & 1), "vec": bool(r & 2), "lanes_per_row": 1 << ((r >> 2) & 7), "resident": bool(r & 32),
                "seed_split": bool(r & 64), "wide_index": bool(r & 128), "da": bool(r & 256), "db": bool(r & 512), "blocks": r >> 10}

    @staticmethod
    def _gate_g(g, what):
        """the four pointer arguments ``(g, g_h, g_l, sexp)`` of the gate kernels for a cotangent ``[N, H, W, C]`` - an fp32 NHWC
        tensor or a one-scale :class:`SplitTensor` read as it lies - with its shape and device"""
        ptrs, shape, dev = _split_operand(g, what, "g", "no NHWC map")
        if len(shape) != 4:
            raise LaplaceHipError(f"{what}: g {tuple(shape)} is no NHWC map [N, H, W, C]")
        return ptrs, tuple(int(d) for d in shape), dev

    def gate_reduce(self, g, x, S):
        """``ds`` ``[S * B, C]``: ``ds[s B + b, c] = sum_hw g[s B + b, h, w, c] * x[b, h, w, c]`` for the ``S`` seeds stacked in the
        NHWC cotangent ``g`` ``[S * B, H, W, C]`` - an fp32 tensor or a one-scale :class:`SplitTensor` read as it lies - from ONE
        fp32 NHWC map ``x`` ``[B, H, W, C]`` per sample, in ONE launch of lk_gate_reduce_nhwc_f32 (csrc/lk_gate.hip)"""
        ptrs, (N, H, W, C), dev = self._gate_g(g, "gate_reduce")
        _check(x, "x")
        S = int(S)
        if S < 1 or x.dim() != 4 or N != S * x.shape[0] or tuple(x.shape[1:]) != (H, W, C) or x.device != dev:
            raise LaplaceHipError(f"gate_reduce: g {(N, H, W, C)} and x {tuple(x.shape)} do not belong together for S = {S}")
        ds = torch.empty(N, C, dtype=torch.float32, device=dev)
        self._rc(self.lib.lk_gate_reduce_nhwc_f32(*ptrs, _ptr(x), S, N // S, H * W, C, _ptr(ds), self._stream(dev)),
                 "lk_gate_reduce_nhwc_f32")
        return ds

    def gate_vjp(self, g, gate, r, S, amax=None):
        """``dx`` ``[S * B, H, W, C]`` fp32: ``g[s B + b, h, w, c] * gate[b, c] + r[s B + b, c]`` for the ``S`` seeds stacked in the
        NHWC cotangent ``g`` (an fp32 tensor or a one-scale :class:`SplitTensor` read as it lies), ``gate`` ``[B, C]`` fp32 and
        ``r`` ``[S * B, C]`` fp32 or ``None``, in ONE launch of lk_gate_vjp_nhwc_f32.  ``amax``: zeroed device word that receives
        the bit pattern of max|dx|."""
        ptrs, (N, H, W, C), dev = self._gate_g(g, "gate_vjp")
        _check(gate, "gate")
        S = int(S)
        if S < 1 or gate.dim() != 2 or N != S * gate.shape[0] or gate.shape[1] != C or gate.device != dev:
            raise LaplaceHipError(f"gate_vjp: g {(N, H, W, C)} and gate {tuple(gate.shape)} do not belong together for S = {S}")
        if r is not None:
            _check(r, "r")
            if tuple(r.shape) != (N, C) or r.device != dev:
                raise LaplaceHipError(f"gate_vjp: r {tuple(r.shape)} is not [{N}, {C}]")
        _amax_word(amax, "gate_vjp")
        dx = torch.empty(N, H, W, C, dtype=torch.float32, device=dev)
        self._rc(self.lib.lk_gate_vjp_nhwc_f32(*ptrs, _ptr(gate), _ptr(r), S, N // S, H * W, C, _ptr(dx), _ptr(amax),
                                               self._stream(dev)), "lk_gate_vjp_nhwc_f32")
        return dx

    def gate_variant(self, vjp, S, B, P, C, aligned=True):
        """lk_gate_variant: the path ``lk_gate_reduce_nhwc_f32`` (``vjp`` false) or ``lk_gate_vjp_nhwc_f32`` (true) takes for a
        shape (host only, no device call), or ``None`` for a shape they refuse"""
        r = int(self.lib.lk_gate_variant(int(bool(vjp)), int(S), int(B), int(P), int(C), int(bool(aligned))))
        if r < 0:
            return None
        return {"vec": bool(r & 1), "resident": bool(r & 2), "seed_split": bool(r & 4), "wide_index": bool(r & 8),
                "lanes": 1 << ((r >> 4) & 7), "blocks": r >> 8}

    def softmax_vjp(self, g, y, S, is_log=False):
        """``dx`` (the shape of ``g``) of ``y = softmax(x, -1)`` / ``log_softmax(x, -1)`` for the ``S`` seeds stacked in the
        cotangent ``g`` (``S * y.numel()`` elements, seed-major) from ONE output ``y`` ``[..., L]`` per sample, in ONE launch of
        lk_softmax_vjp_f32 (csrc/lk_softmax.hip): ``y * (g - sum(g y))`` or ``g - exp(y) sum(g)`` along the last dim."""
        _check(g, "g"), _check(y, "y")
        S = int(S)
        L = int(y.shape[-1]) if y.dim() else 1
        R = y.numel() // L if L else 0
        if S < 1 or L < 1 or g.numel() != S * y.numel():
            raise LaplaceHipError(f"softmax_vjp: g {tuple(g.shape)} and y {tuple(y.shape)} do not belong together for S = {S}")
        if y.device != g.device:
            raise LaplaceHipError("softmax_vjp: g and y are on different devices")
        dx = torch.empty_like(g)
        self._rc(self.lib.lk_softmax_vjp_f32(_ptr(g), _ptr(y), S, R, L, int(bool(is_log)), _ptr(dx), self._stream(g.device)),
                 "lk_softmax_vjp_f32")
        return dx

    def softmax_vjp_variant(self, S, R, L, is_log=False, aligned=True):
        """lk_softmax_vjp_variant: the path ``lk_softmax_vjp_f32`` takes for a shape (host only, no device call), or ``None`` for a
        shape it refuses"""
        r = int(self.lib.lk_softmax_vjp_variant(int(S), int(R), int(L), int(is_log), int(bool(aligned))))
        if r < 0:
            return None
        return {"vec": bool(r & 1), "lanes_per_row": 1 << ((r >> 1) & 7), "resident": bool(r & 16), "seed_split": bool(r & 32),
                "wide_index": bool(r & 64), "log": bool(r & 128), "blocks": r >> 8}

    def matmul_vjp(self, g, a, b, S, want=(True, True)):
        """``(da, db)`` of ``out = a @ b`` for the ``S`` seeds stacked in the cotangent ``g`` ``[S * B, ..., M, N]`` (seed-major) from
        ONE ``a`` ``[B, ..., M, K]`` and ``b`` ``[B, ..., K, N]`` per sample (equal leading dims), one launch of lk_matmul_vjp_f32's
        kernel per output (csrc/lk_matmul.hip): ``da = g b^T`` ``[S * B, ..., M, K]``, ``db = a^T g`` ``[S * B, ..., K, N]``.
        ``want``: which of the two to compute (``None`` stands for the other)."""
        _check(g, "g"), _check(a, "a"), _check(b, "b")
        S, want_da, want_db = int(S), bool(want[0]), bool(want[1])
        ok = a.dim() >= 2 and a.dim() == b.dim() == g.dim() and a.shape[:-2] == b.shape[:-2] and a.shape[-1] == b.shape[-2]
        if ok:
            M, K, N = int(a.shape[-2]), int(a.shape[-1]), int(b.shape[-1])
            NB = a.numel() // (M * K) if M * K else 0
            ok = S >= 1 and (want_da or want_db) and min(M, K, N) >= 1 and g.numel() == S * NB * M * N and tuple(g.shape[-2:]) == (M, N)
        if not ok:
            raise LaplaceHipError(f"matmul_vjp: g {tuple(g.shape)}, a {tuple(a.shape)}, b {tuple(b.shape)} do not belong together for "
                                  f"S = {S}, want = {tuple(want)}")
        if a.device != g.device or b.device != g.device:
            raise LaplaceHipError("matmul_vjp: g, a and b are on different devices")
        lead = (S * a.shape[0], *a.shape[1:-2]) if a.dim() > 2 else ()
        da = torch.empty((*lead, M, K) if a.dim() > 2 else (S * M, K), dtype=torch.float32, device=g.device) if want_da else None
        db = torch.empty((*lead, K, N) if a.dim() > 2 else (S * K, N), dtype=torch.float32, device=g.device) if want_db else None
        self._rc(self.lib.lk_matmul_vjp_f32(_ptr(g), _ptr(a), _ptr(b), S, NB, M, K, N, _ptr(da), _ptr(db), self._stream(g.device)),
                 "lk_matmul_vjp_f32")
        return da, db

    def matmul_vjp_variant(self, S, NB, M, K, N, want=(True, True)):
        """lk_matmul_vjp_variant: the path ``lk_matmul_vjp_f32`` takes for a shape (host only, no device call), or ``None`` for a
        shape it refuses"""
        r = int(self.lib.lk_matmul_vjp_variant(int(S), int(NB), int(M), int(K), int(N), int(bool(want[0])), int(bool(want[1]))))
        if r < 0:
            return None
        return {"da": bool(r & 1), "db": bool(r & 2), "resident_da": bool(r & 4), "resident_db": bool(r & 8),
                "seed_split": bool(r & 16), "wide_index": bool(r & 32), "blocks": r >> 6}

    @staticmethod
    def _dwconv_geometry(x_hw, kernel, stride, padding, what):
        """``(kh, kw, sh, sw, ph, pw, OH, OW)`` as ints, or an error when the window leaves no output on the map"""
        (H, W), (kh, kw), (sh, sw), (ph, pw) = x_hw, _pair(kernel), _pair(stride), _pair(padding)
        if min(kh, kw, sh, sw) < 1 or H + 2 * ph < kh or W + 2 * pw < kw:
            raise LaplaceHipError(f"{what}: window ({kh}, {kw}) / stride ({sh}, {sw}) / padding ({ph}, {pw}) leaves no output "
                                  f"on a {H} x {W} map")
        return kh, kw, sh, sw, ph, pw, (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1

    def dwconv_forward(self, x_nhwc, w_tap, bias, kernel, stride, padding):
        """``y`` ``[B, OH, OW, C]`` of a depthwise convolution over the fp32 NHWC map ``x_nhwc`` ``[B, H, W, C]`` (csrc/lk_dwconv.hip);
        ``w_tap`` ``[kh * kw, C]`` fp32 with ``w_tap[dy * kw + dx, c] = weight[c, 0, dy, dx]``; ``bias`` ``[C]`` or None."""
        _check(x_nhwc, "x_nhwc"), _check(w_tap, "w_tap")
        if x_nhwc.dim() != 4:
            raise LaplaceHipError("dwconv_forward: expected an NHWC map [B, H, W, C]")
        B, H, W, C = x_nhwc.shape
        kh, kw, sh, sw, ph, pw, OH, OW = self._dwconv_geometry((H, W), kernel, stride, padding, "dwconv_forward")
        if tuple(w_tap.shape) != (kh * kw, C):
            raise LaplaceHipError(f"dwconv_forward: w_tap {tuple(w_tap.shape)} is not [kh * kw, C] = [{kh * kw}, {C}]")
        if bias is not None and tuple(_check(bias, "bias").shape) != (C,):
            raise LaplaceHipError("dwconv_forward: bias must be [C]")
        y = torch.empty(B, OH, OW, C, dtype=torch.float32, device=x_nhwc.device)
        self._rc(self.lib.lk_dwconv_fwd_nhwc_f32(_ptr(x_nhwc), _ptr(w_tap), _ptr(bias), B, H, W, C, kh, kw, sh, sw, ph, pw, _ptr(y),
                                                 self._stream(x_nhwc.device)), "lk_dwconv_fwd_nhwc_f32")
        return y

    def dwconv_backward(self, g: "SplitTensor", w_tap, S, in_hw, kernel, stride, padding, amax=None):
        """``dx`` ``[S*B, H, W, C]`` (fp32) of a depthwise convolution for the ``S`` seeds stacked in the one-scale split cotangent
        ``g`` ``[S*B, OH, OW, C]``; ``in_hw`` = ``(H, W)``.  ``amax``: zeroed device word that receives the bit pattern of max|dx|."""
        g_ptrs = _split_half(g, "dwconv_backward", "g", None)  # (a chunk-major g is refused below, with its shape)
        _check(w_tap, "w_tap")
        S, (H, W) = int(S), (int(in_hw[0]), int(in_hw[1]))
        if g.chunked or g.planes.dim() != 5 or S < 1 or g.planes.shape[1] % S:
            raise LaplaceHipError("dwconv_backward: g must be a split tensor [S*B, OH, OW, C]")
        B, C = g.planes.shape[1] // S, g.planes.shape[4]
        kh, kw, sh, sw, ph, pw, OH, OW = self._dwconv_geometry((H, W), kernel, stride, padding, "dwconv_backward")
        if tuple(g.planes.shape[2:4]) != (OH, OW):
            raise LaplaceHipError(f"dwconv_backward: g {tuple(g.shape)} is not the output of window ({kh}, {kw}), stride "
                                  f"({sh}, {sw}), padding ({ph}, {pw}) on a {H} x {W} map")
        if tuple(w_tap.shape) != (kh * kw, C):
            raise LaplaceHipError(f"dwconv_backward: w_tap {tuple(w_tap.shape)} is not [kh * kw, C] = [{kh * kw}, {C}]")
        _amax_word(amax, "dwconv_backward")
        dx = torch.empty(S * B, H, W, C, dtype=torch.float32, device=g.planes.device)
        self._rc(self.lib.lk_dwconv_bwd_nhwc_f16x2(*g_ptrs, _ptr(w_tap), S, B, H, W, C,
                                                   kh, kw, sh, sw, ph, pw, _ptr(dx), _ptr(amax), self._stream(dx.device)),
                 "lk_dwconv_bwd_nhwc_f16x2")
        return dx

    def dwconv_variant(self, S, B, H, W, C, kernel, stride, padding, aligned=True):
        """lk_dwconv_variant: the path ``lk_dwconv_bwd_nhwc_f16x2`` takes for a shape (host only, no device call), or ``None`` for
        a shape it refuses."""
        (kh, kw), (sh, sw), (ph, pw) = _pair(kernel), _pair(stride), _pair(padding)
        r = int(self.lib.lk_dwconv_variant(int(S), int(B), int(H), int(W), int(C), kh, kw, sh, sw, ph, pw, int(bool(aligned))))
        if r < 0:
            return None
        return {"vec": bool(r & 1), "strided": bool(r & 2), "seed_split": bool(r & 4), "tap_class": (r >> 3) & 1,
                "seeds_per_pass": (r >> 4) & 0xFF, "seeds_per_slice": r >> 12}

    def sq_colsum(self, Js, col0, width, alpha, h):
        _check(Js, "Js"), _check(h, "h")
        P = Js.shape[-1]
        rows = Js.numel() // P
        self._rc(self.lib.lk_sq_colsum_f32(_ptr(Js), rows, P, int(col0), int(width), float(alpha), _ptr(h),
                                           self._stream(Js.device)), "lk_sq_colsum_f32")

    def bn_act_forward(self, x, scale, shift, relu, addend=None, want_mask=True):
        """``(y, mask)``: ``y = act(x * scale[c] + shift[c] + addend)`` for ``x`` [B, C, ...]; ``mask = y > 0`` (bool) if
        ``relu``."""
        _check(x, "x")
        if addend is not None:
            _check(addend, "addend")
            if addend.shape != x.shape:
                raise ValueError("bn_act_forward: addend must have the shape of x")
        C = x.shape[1]
        hw = x.numel() // (x.shape[0] * C) if x.numel() else 1
        y = torch.empty_like(x)
        mask = torch.empty(x.shape, dtype=torch.bool, device=x.device) if (relu and want_mask) else None
        self._rc(self.lib.lk_bn_act_fwd_f32(_ptr(x), _ptr(scale.to(torch.float32).contiguous()),
                                            _ptr(shift.to(torch.float32).contiguous()), _ptr(addend), x.numel(), C, max(hw, 1),
                                            1 if relu else 0, _ptr(y), _ptr(mask), self._stream(x.device)),
                 "lk_bn_act_fwd_f32")
        return y, mask

    def vjp_scale_mask(self, g, S, mult, scale, hw, g2=None):
        """``out[s, e] = (g[s, e] + g2[s, e]) * mult[e] * scale[channel(e)]`` for the ``S`` seeds stacked in ``g``
        ([S*B, ...]); ``g2``, ``mult`` ([B, ...], bool or float32) and ``scale`` ([C]) may be None."""
        _check(g, "g")
        if g2 is not None:
            _check(g2, "g2")
            if g2.shape != g.shape:
                raise ValueError("vjp_scale_mask: g2 must have the shape of g")
        per = g.numel() // S
        out = torch.empty_like(g)
        m_is_float = 0
        if mult is not None:
            if mult.dtype == torch.bool:
                mult = mult.contiguous()
            else:
                mult, m_is_float = mult.to(torch.float32).contiguous(), 1
            if mult.numel() != per:
                raise ValueError("vjp_scale_mask: multiplier must have the per-seed shape")
        C = 1
        if scale is not None:
            scale = scale.to(torch.float32).contiguous()
            C = scale.numel()
        self._rc(self.lib.lk_vjp_scale_mask_f32(_ptr(g), _ptr(g2), _ptr(mult), m_is_float,
                                                _ptr(scale), int(S), per, C, int(hw),
                                                _ptr(out), self._stream(g.device)), "lk_vjp_scale_mask_f32")
        return out

    # ---- dense last-layer GGN -----------------------------------------------------------------
    def ll_ggn_full(self, phi, probs, has_bias, alpha, H):
        _check(phi, "phi"), _check(H, "H")
        B, D = phi.shape
        if probs is not None:
            _check(probs, "probs")
            C = probs.shape[1]
        else:
            C = (H.shape[0]) // (D + (1 if has_bias else 0))
        nb = self.lib.lk_ll_ggn_workspace_bytes(B, C, D)
        ws = self._workspace(nb, phi.device)
        Dt = D + (1 if has_bias else 0)
        # structured form: C block-diagonal Grams of sqrt(p_j sum_{k != j} p_k) phi~ minus the off-diagonal blocks of the Gram of
        # Y = [p_j phi~]_j — about 2 C^2 Dt^2 flop per sample against the 2 C^3 Dt^2 of J^T Lambda J as the reference writes it
        # (curvature.py:375-411)
        self._rc(self._timed("llggn", 2.0 * B * C * C * Dt * Dt, phi.device, lambda: self.lib.lk_ll_ggn_full_f32(
            _ptr(phi), _ptr(probs), B, C, D, 1 if has_bias else 0, float(alpha), _ptr(H), _ptr(ws), ws.numel(),
            self._stream(phi.device)), nbytes=4.0 * (B * D + B * C + (C * Dt) ** 2)), "lk_ll_ggn_full_f32")
        return H

    # ---- eigensolver --------------------------------------------------------------------------
    def syevj(self, A, clamp=True, max_sweeps=0):
        _check(A, "A")
        n = A.shape[0]
        assert A.shape == (n, n)
        w = torch.empty(n, dtype=torch.float32, device=A.device)
        Q = torch.empty(n, n, dtype=torch.float32, device=A.device)
        info = torch.zeros(2, dtype=torch.int32, device=A.device)
        nb = self.lib.lk_syevj_workspace_bytes(n)
        # the solve is long-running and asynchronous: give it a private workspace
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=A.device)
        self._rc(
            self.lib.lk_syevj_f32(_ptr(A), n, _ptr(w), _ptr(Q), 1 if clamp else 0, int(max_sweeps), _ptr(info), _ptr(ws),
                                  ws.numel(), self._stream(A.device)),
            "lk_syevj_f32",
        )
        ws.record_stream(torch.cuda.current_stream(A.device))
        return w, Q, info

    def syevj_batched(self, mats, clamp=True, max_sweeps=0, streams=None):
        """Eigendecompose a list of symmetric matrices (largest first is best) -> list of (w, Q, info).

        ``streams``: torch side streams for the solve — with three or more, the matrices iterate in two lanes of rounds
        (``streams[0]``, ``streams[1]``: the pivot solves of one beside the tile updates of the other) and finished
        matrices are refined on ``streams[2]``; with two, one lane + the refinements; further streams are only made to
        wait.  The caller orders them against its own stream (``wait_stream`` before / after).  ``None`` = the current
        stream."""
        if not mats:
            return []
        dev = mats[0].device
        cur = torch.cuda.current_stream(dev)
        streams = list(streams) if streams else [cur]
        count = len(mats)
        outs, keep = [], []
        arr = lambda ctype, vals: (ctype * count)(*vals)  # noqa: E731
        ns = []
        for i, A in enumerate(mats):
            _check(A, "A")
            n = A.shape[0]
            assert A.shape == (n, n) and A.device == dev
            w = torch.empty(n, dtype=torch.float32, device=dev)
            Q = torch.empty(n, n, dtype=torch.float32, device=dev)
            info = torch.zeros(2, dtype=torch.int32, device=dev)
            ws = torch.empty(max(self.lib.lk_syevj_workspace_bytes(n), 1), dtype=torch.uint8, device=dev)
            outs.append((w, Q, info))
            keep.append(ws)
            ns.append(n)
        nstreams = min(len(streams), count)
        used = streams[:nstreams]
        # `info` was zero-filled on the current stream: the side streams must see that (and the inputs) first
        for st in used:
            if st != cur:
                st.wait_stream(cur)
        rc = self.lib.lk_syevj_batched_f32(
            count, arr(ctypes.c_void_p, [A.data_ptr() for A in mats]), arr(ctypes.c_int64, ns),
            arr(ctypes.c_void_p, [o[0].data_ptr() for o in outs]), arr(ctypes.c_void_p, [o[1].data_ptr() for o in outs]),
            arr(ctypes.c_void_p, [o[2].data_ptr() for o in outs]), arr(ctypes.c_void_p, [w_.data_ptr() for w_ in keep]),
            arr(ctypes.c_size_t, [w_.numel() for w_ in keep]), 1 if clamp else 0, int(max_sweeps),
            arr(ctypes.c_void_p, [st.cuda_stream for st in used]), nstreams)
        self._rc(rc, "lk_syevj_batched_f32")
        for st in used[:3]:
            if st != cur:  # allocated on `cur`, used on `st`
                for A, o, ws in zip(mats, outs, keep):
                    for t in (A, ws) + o:
                        t.record_stream(st)
        return outs

    # ---- logdet -------------------------------------------------------------------------------
    def kron_logdet(self, l1, l2, delta, damping=False, want_grads=False):
        """Returns (value[1], d_l1, d_l2, d_delta[1]); derivative tensors are None unless requested."""
        _check(l1, "l1"), _check(delta, "delta")
        n1 = l1.numel()
        n2 = 0 if l2 is None else l2.numel()
        if l2 is not None:
            _check(l2, "l2")
        dev = l1.device
        out = torch.zeros(1, dtype=torch.float32, device=dev)
        d1 = d2 = dd = None
        if want_grads:
            d1 = torch.zeros(n1, dtype=torch.float32, device=dev)
            d2 = torch.zeros(n2, dtype=torch.float32, device=dev) if n2 else None
            dd = torch.zeros(1, dtype=torch.float32, device=dev)
        nb = self.lib.lk_kron_logdet_workspace_bytes(n1)
        ws = self._workspace(nb, dev)
        self._rc(
            self.lib.lk_kron_logdet_f32(_ptr(l1), n1, _ptr(l2), n2, _ptr(delta), 1 if damping else 0, _ptr(out), _ptr(d1),
                                        _ptr(d2), _ptr(dd), _ptr(ws), ws.numel(), self._stream(dev)),
            "lk_kron_logdet_f32",
        )
        return out, d1, d2, dd

    def kron_logdet_blocks(self, blocks, deltas, scale=None, want_grads=False):
        """``blocks``: list of ``(l1,)`` / ``(l1, l2)`` eigenvalue vectors; ``deltas [len(blocks)]``; ``scale [1]`` or
        None.  Returns ``(value[1], d_deltas or None, d_scale or None)`` -- the whole posterior in three launches."""
        nb = len(blocks)
        _check(deltas, "deltas")
        if deltas.numel() != nb:
            raise ValueError("kron_logdet_blocks: one delta per block")
        dev = deltas.device
        for ls in blocks:
            for l in ls:
                _check(l, "eigenvalues")
        if scale is not None:
            _check(scale, "scale")
        PA, LA = ctypes.c_void_p * nb, ctypes.c_int64 * nb
        l1 = PA(*[ls[0].data_ptr() for ls in blocks])
        l2 = PA(*[(ls[1].data_ptr() if len(ls) == 2 else None) for ls in blocks])
        n1 = LA(*[ls[0].numel() for ls in blocks])
        n2 = LA(*[(ls[1].numel() if len(ls) == 2 else 0) for ls in blocks])
        out = torch.zeros(1, dtype=torch.float32, device=dev)
        dd = torch.zeros(nb, dtype=torch.float32, device=dev) if want_grads else None
        ds = torch.zeros(1, dtype=torch.float32, device=dev) if want_grads and scale is not None else None
        nbytes = self.lib.lk_kron_logdet_blocks_workspace_bytes(sum(n1), nb)
        ws = self._workspace(nbytes, dev)
        self._rc(
            self.lib.lk_kron_logdet_blocks_f32(nb, l1, n1, l2, n2, _ptr(deltas), _ptr(scale), _ptr(out), _ptr(dd), _ptr(ds),
                                               _ptr(ws), ws.numel(), self._stream(dev)),
            "lk_kron_logdet_blocks_f32",
        )
        return out, dd, ds

    # ---- predictive ---------------------------------------------------------------------------
    def kron_quadform_linear(self, u, v, l1, l2, delta, fvar, ub=None, lb=None, delta_b=None):
        for t, nm in ((u, "u"), (v, "v"), (l1, "l1"), (l2, "l2"), (delta, "delta"), (fvar, "fvar")):
            _check(t, nm)
        Cc, B, Do = u.shape
        Di = v.shape[1]
        if ub is not None:
            _check(ub, "ub"), _check(lb, "lb"), _check(delta_b, "delta_b")
        self._rc(
            self.lib.lk_kron_quadform_linear_f32(_ptr(u), _ptr(v), _ptr(l1), _ptr(l2), _ptr(delta), B, Cc, Do, Di, _ptr(ub),
                                                 _ptr(lb), _ptr(delta_b), _ptr(fvar), self._stream(u.device)),
            "lk_kron_quadform_linear_f32",
        )
        return fvar

    #: most outputs the fused weight-sharing predictive holds in accumulators at once
    quadform_shared_max_outputs = 10

    def kron_quadform_shared(self, u, v, l1, l2, delta, fvar, seed_major=False):
        """``u [B, C, Do, L]`` (``seed_major``: ``[C, B, Do, L]``), ``v [B, Dk, L]`` (eigenbasis projections), fp32;
        ``fvar [B, C, C] +=`` (three-piece bf16 products; operands that arrive split: :meth:`kron_quadform_shared_planes`)"""
        for t, nm in ((u, "u"), (v, "v"), (l1, "l1"), (l2, "l2"), (delta, "delta"), (fvar, "fvar")):
            _check(t, nm)
        if seed_major:
            C, B, Do, L = u.shape
        else:
            B, C, Do, L = u.shape
        Dk = v.shape[1]
        ws = self._workspace(self.lib.lk_quadform_shared_workspace_bytes(B, C, Do, Dk), u.device)
        if seed_major:
            self._rc(
                self._timed("quadconv", 2.0 * B * C * L * Do * Dk, u.device, lambda: self.lib.lk_kron_quadform_shared_seedmajor_f32(
                    _ptr(u), _ptr(v), _ptr(l1), _ptr(l2), _ptr(delta), B, C, Do, Dk, L, _ptr(fvar), _ptr(ws), ws.numel(),
                    self._stream(u.device))),
                "lk_kron_quadform_shared_seedmajor_f32",
            )
            return fvar
        self._rc(
            self._timed("quadconv", 2.0 * B * C * L * Do * Dk, u.device, lambda: self.lib.lk_kron_quadform_shared_f32(
                _ptr(u), _ptr(v), _ptr(l1), _ptr(l2), _ptr(delta), B, C, Do, Dk, L, _ptr(fvar), _ptr(ws), ws.numel(),
                self._stream(u.device))),
            "lk_kron_quadform_shared_f32",
        )
        return fvar

    #: ``False``: the Kron predictive's rotations emit fp32 and the quadratic-form kernel splits in flight (three bf16 pieces)
    use_quad_planes = True

    def kron_quadform_shared_planes(self, u, v, l1, l2, delta, fvar, C):
        """lk_kron_quadform_shared_planes_f16x2: ``u`` SplitTensor ``[C * B, Do, L]`` (seed-major, one scale), ``v`` SplitTensor
        ``[B, Dk, L]`` (one scale per sample or one) — the outputs of :meth:`conv_nhwc_f16x2_planes`; ``fvar [B, C, C] +=``"""
        for t, nm in ((l1, "l1"), (l2, "l2"), (delta, "delta"), (fvar, "fvar")):
            _check(t, nm)
        _one_scale(u, "kron_quadform_shared_planes (u)")
        CB, Do, L = u.shape
        B, Dk = v.shape[0], v.shape[1]
        if CB != C * B or v.shape[2] != L or L % 16 or Do % 32:
            raise LaplaceHipError("kron_quadform_shared_planes: u [C * B, Do, L], v [B, Dk, L], L % 16 == 0, Do % 32 == 0")
        u, v = u.chunk_major(), v.chunk_major()  # (what the rotation convolutions emit; a copy for operands split elsewhere)
        ws = self._workspace(self.lib.lk_quadform_shared_workspace_bytes(B, C, Do, Dk), fvar.device)
        # (its own profile tag: three fp16 MFMAs per product block — bench.py prices the fp32-operand forms, six bf16 MFMAs, apart)
        self._rc(self._timed("quadconv16", 2.0 * B * C * L * Do * Dk, fvar.device, lambda: self.lib.lk_kron_quadform_shared_planes_f16x2(
            _ptr(u.planes[0]), _ptr(u.planes[1]), _ptr(u.sexp), _ptr(v.planes[0]), _ptr(v.planes[1]), _ptr(v.sexp), v.sexp.numel(),
            _ptr(l1), _ptr(l2), _ptr(delta), B, C, Do, Dk, L, _ptr(self._zero16(fvar.device)), _ptr(fvar), _ptr(ws), ws.numel(),
            self._stream(fvar.device))), "lk_kron_quadform_shared_planes_f16x2")
        return fvar

    def diag_quadform_shared(self, u, v, var_w, fvar):
        """``u [B, C, Do, L]`` output gradients, ``v [B, Dk, L]`` unfolded inputs, ``var_w [Do, Dk]``."""
        for t, nm in ((u, "u"), (v, "v"), (var_w, "var_w"), (fvar, "fvar")):
            _check(t, nm)
        B, C, Do, L = u.shape
        Dk = v.shape[1]
        ws = self._workspace(self.lib.lk_quadform_shared_workspace_bytes(B, C, Do, Dk), u.device)
        self._rc(
            self.lib.lk_diag_quadform_shared_f32(_ptr(u), _ptr(v), _ptr(var_w), B, C, Do, Dk, L, _ptr(fvar), _ptr(ws),
                                                 ws.numel(), self._stream(u.device)),
            "lk_diag_quadform_shared_f32",
        )
        return fvar

    def diag_ggn_shared(self, u, v, alpha, h):
        """``h[Do*Dk] += alpha * sum_{n,s} (u[n,s] v[n]^T)^2``; ``u [B, S, Do, L]``, ``v [B, Dk, L]``, ``S <= 10``."""
        for t, nm in ((u, "u"), (v, "v"), (h, "h")):
            _check(t, nm)
        B, S, Do, L = u.shape
        Dk = v.shape[1]
        ws = self._workspace(self.lib.lk_diag_ggn_shared_workspace_bytes(B, Do, Dk), u.device)
        self._rc(
            self.lib.lk_diag_ggn_shared_f32(_ptr(u), _ptr(v), B, S, Do, Dk, L, float(alpha), _ptr(h), _ptr(ws), ws.numel(),
                                            self._stream(u.device)),
            "lk_diag_ggn_shared_f32",
        )
        return h

    def diag_quadform_linear(self, a, g, var_w, var_b, fvar):
        for t, nm in ((a, "a"), (g, "g"), (var_w, "var_w"), (fvar, "fvar")):
            _check(t, nm)
        Cc, B, Do = g.shape
        Di = a.shape[1]
        if var_b is not None:
            _check(var_b, "var_b")
        self._rc(
            self.lib.lk_diag_quadform_linear_f32(_ptr(a), _ptr(g), _ptr(var_w), _ptr(var_b), B, Cc, Do, Di, _ptr(fvar),
                                                 self._stream(a.device)),
            "lk_diag_quadform_linear_f32",
        )
        return fvar

    # ---- prior-precision grid (csrc/lk_grid.hip): var [G, B, C] of all grid points in one pass ----------------------------
    #: weight forms of the grid kernels: Kron, damped Kron, diagonal
    GRID_KRON, GRID_KRON_DAMPED, GRID_DIAG = 0, 1, 2

    def quadform_linear_grid(self, u, v, w0, w1, deltas, mode, var, ub=None, wb=None):
        """nn.Linear layer, ``u [C, B, Do]``, ``v [B, Di]``; ``w0, w1`` = ``l1 [Do], l2 [Di]`` (Kron modes) or ``h [Do, Di], None``
        (diagonal); optional bias block ``ub [C, B, Do]`` with ``wb [Do]``; ``var [G, B, C] +=``"""
        for t, nm in ((u, "u"), (v, "v"), (w0, "w0"), (deltas, "deltas"), (var, "var")):
            _check(t, nm)
        if w1 is not None:
            _check(w1, "w1")
        if ub is not None:
            _check(ub, "ub"), _check(wb, "wb")
        C, B, Do = u.shape
        Di = v.shape[1]
        G = deltas.numel()
        if v.shape[0] != B or var.shape != (G, B, C):
            raise LaplaceHipError("quadform_linear_grid: u [C, B, Do], v [B, Di], var [G, B, C]")
        self._rc(self.lib.lk_quadform_linear_grid_f32(_ptr(u), _ptr(v), _ptr(w0), _ptr(w1), _ptr(deltas), G, int(mode), B, C, Do,
                                                      Di, _ptr(ub), _ptr(wb), _ptr(var), self._stream(u.device)),
                 "lk_quadform_linear_grid_f32")
        return var

    def quadform_shared_grid(self, u, v, w0, w1, deltas, mode, var, seed_major=False):
        """weight-sharing layer, ``u [B, C, Do, L]`` (``seed_major``: ``[C, B, Do, L]``), ``v [B, Dk, L]``; weights as
        :meth:`quadform_linear_grid` (``h [Do, Dk]`` for the diagonal form); ``var [G, B, C] +=``"""
        for t, nm in ((u, "u"), (v, "v"), (w0, "w0"), (deltas, "deltas"), (var, "var")):
            _check(t, nm)
        if w1 is not None:
            _check(w1, "w1")
        if seed_major:
            C, B, Do, L = u.shape
        else:
            B, C, Do, L = u.shape
        Dk = v.shape[1]
        G = deltas.numel()
        if v.shape != (B, Dk, L) or var.shape != (G, B, C):
            raise LaplaceHipError("quadform_shared_grid: v [B, Dk, L], var [G, B, C]")
        ws = self._workspace(self.lib.lk_quadform_shared_grid_workspace_bytes(B, C, Do, Dk, G), u.device)
        self._rc(self._timed("quadgrid", 2.0 * B * C * L * Do * Dk + 2.0 * B * C * Do * Dk * G, u.device,
                             lambda: self.lib.lk_quadform_shared_grid_f32(
                                 _ptr(u), _ptr(v), _ptr(w0), _ptr(w1), _ptr(deltas), G, int(mode), B, C, Do, Dk, L,
                                 int(bool(seed_major)), _ptr(var), _ptr(ws), ws.numel(), self._stream(u.device))),
                 "lk_quadform_shared_grid_f32")
        return var

    #: ``form`` of :meth:`quadform_shared_variant` (LK_QF_* of include/laplace_hip.h)
    QF_KRON, QF_KRON_SEEDMAJOR, QF_DIAG, QF_PLANES, QF_DIAG_GGN, QF_GRID = range(6)

    def quadform_shared_variant(self, form, B, C, Do, Dk, L, aligned16=True):
        """lk_quadform_shared_variant: the instantiation of the weight-sharing kernels the shape launches (host only, no
        device call), or ``None`` for a shape the form does not serve.  ``ct`` and ``split`` always; the planes form adds
        ``occ``, ``sub``, ``w_in_lds``, the others ``arith``."""
        r = int(self.lib.lk_quadform_shared_variant(int(form), int(B), int(C), int(Do), int(Dk), int(L), int(bool(aligned16))))
        if r < 0:
            return None
        out = {"ct": r & 15, "split": r >> 8}
        flags = (r >> 4) & 15
        if form == self.QF_PLANES:
            out.update(occ=2 if flags & 1 else 1, sub=bool(flags & 2), w_in_lds=bool(flags & 4))
        else:
            out["arith"] = flags & 1
        return out

    def probit_nll_grid(self, f_mu, var, y, loss_sum):
        """``loss_sum [G] (float64) +=`` the probit-link NLL of the batch at every grid point; ``f_mu [B, C]``,
        ``var [G, B, C]``, ``y [B]`` (int64)"""
        _check(f_mu, "f_mu"), _check(var, "var"), _check(y, "y", torch.int64), _check(loss_sum, "loss_sum", torch.float64)
        B, C = f_mu.shape
        G = loss_sum.numel()
        if var.shape != (G, B, C) or y.shape != (B,):
            raise LaplaceHipError("probit_nll_grid: f_mu [B, C], var [G, B, C], y [B], loss_sum [G]")
        self._rc(self.lib.lk_probit_nll_grid_f32(_ptr(f_mu), _ptr(var), _ptr(y), G, B, C, _ptr(loss_sum),
                                                 self._stream(f_mu.device)), "lk_probit_nll_grid_f32")
        return loss_sum

    def diag_quadform_js(self, Js, var):
        _check(Js, "Js"), _check(var, "var")
        B, C, P = Js.shape
        fvar = torch.empty(B, C, C, dtype=torch.float32, device=Js.device)
        self._rc(self.lib.lk_diag_quadform_js_f32(_ptr(Js), _ptr(var), B, C, P, _ptr(fvar), self._stream(Js.device)),
                 "lk_diag_quadform_js_f32")
        return fvar

    def jac_last_layer(self, phi, C, has_bias):
        """Js [B, C, P] = e_c (x) [phi_n, 1] (curvature.py:131-167 for a Linear head)."""
        _check(phi, "phi")
        B, D = phi.shape
        Js = torch.empty(B, C, C * D + (C if has_bias else 0), dtype=torch.float32, device=phi.device)
        self._rc(self.lib.lk_jac_last_layer_f32(_ptr(phi), B, C, D, 1 if has_bias else 0, _ptr(Js), self._stream(phi.device)),
                 "lk_jac_last_layer_f32")
        return Js

    def dense_quadform_ll(self, phi, Sigma, C, has_bias):
        _check(phi, "phi"), _check(Sigma, "Sigma")
        B, D = phi.shape
        fvar = torch.empty(B, C, C, dtype=torch.float32, device=phi.device)
        nb = self.lib.lk_dense_quadform_ll_workspace_bytes(B, C, D)
        ws = self._workspace(nb, phi.device)
        Dt = D + (1 if has_bias else 0)
        # phi~^T Sigma_ck phi~ for the C (C + 1) / 2 class pairs: C (C + 1) Dt^2 flop per sample (as written in the reference,
        # baselaplace.py:1683-1684 through [B, C, P] Jacobians: 2 C P^2)
        self._rc(self._timed("llquad", float(B) * C * (C + 1) * Dt * Dt, phi.device, lambda: self.lib.lk_dense_quadform_ll_f32(
            _ptr(phi), _ptr(Sigma), B, C, D, 1 if has_bias else 0, _ptr(fvar), _ptr(ws), ws.numel(), self._stream(phi.device)),
            nbytes=4.0 * (B * D + (C * Dt) ** 2 + B * C * C)), "lk_dense_quadform_ll_f32")
        return fvar

    # ---- dense Laplace in the eigenbasis of the curvature (lk_spectral.hip) ---------------------------------
    SP_QUAD_LL, SP_GRID_LL, SP_QUAD_R, SP_GRID_R, SP_BIAS = 0, 1, 2, 3, 4
    SP_TILE_N, SP_TILE_J = 32, 128

    def spectral_quadform_ll(self, phi, Q, lam, hfac, delta, C, has_bias):
        """``fvar [B, C, C] = sum_j R_c R_k / (hfac lam_j + delta)`` with ``R = (I (x) [phi, 1]) Q`` formed per tile;
        ``phi [B, D]``, ``Q [P, P]`` (eigenvectors in columns), ``lam [P]``, ``delta`` a device scalar"""
        _check(phi, "phi"), _check(Q, "Q"), _check(lam, "lam"), _check(delta, "delta")
        B, D = phi.shape
        P = C * D + (C if has_bias else 0)
        if Q.shape != (P, P) or lam.shape != (P,) or delta.numel() != 1:
            raise LaplaceHipError("spectral_quadform_ll: phi [B, D], Q [P, P], lam [P], P = C D (+ C), delta a scalar tensor")
        fvar = torch.empty(B, C, C, dtype=torch.float32, device=phi.device)
        form = self.SP_QUAD_LL | (self.SP_BIAS if has_bias else 0)
        ws = self._workspace(self.lib.lk_spectral_workspace_bytes(form, B, C, D, 1), phi.device)
        self._rc(self._timed("spectral", 2.0 * B * P * P, phi.device, lambda: self.lib.lk_spectral_quadform_ll_f32(
            _ptr(phi), _ptr(Q), _ptr(lam), float(hfac), _ptr(delta), B, C, D, 1 if has_bias else 0, _ptr(fvar), _ptr(ws),
            ws.numel(), self._stream(phi.device)), nbytes=4.0 * (B * D + P * P + B * C * C)), "lk_spectral_quadform_ll_f32")
        return fvar

    def spectral_grid_ll(self, phi, Q, lam, hfac, deltas, C, has_bias, var):
        """``var [G, B, C] +=`` the diagonal of :meth:`spectral_quadform_ll` at every prior precision of ``deltas [G]``"""
        _check(phi, "phi"), _check(Q, "Q"), _check(lam, "lam"), _check(deltas, "deltas"), _check(var, "var")
        B, D = phi.shape
        P = C * D + (C if has_bias else 0)
        G = deltas.numel()
        if Q.shape != (P, P) or lam.shape != (P,) or var.shape != (G, B, C):
            raise LaplaceHipError("spectral_grid_ll: phi [B, D], Q [P, P], lam [P], P = C D (+ C), var [G, B, C]")
        form = self.SP_GRID_LL | (self.SP_BIAS if has_bias else 0)
        ws = self._workspace(self.lib.lk_spectral_workspace_bytes(form, B, C, D, G), phi.device)
        self._rc(self.lib.lk_spectral_grid_ll_f32(_ptr(phi), _ptr(Q), _ptr(lam), float(hfac), _ptr(deltas), G, B, C, D,
                                                  1 if has_bias else 0, _ptr(var), _ptr(ws), ws.numel(),
                                                  self._stream(phi.device)), "lk_spectral_grid_ll_f32")
        return var

    def spectral_quadform(self, R, lam, hfac, delta):
        """``fvar [N, C, C] = sum_j R[n, c, j] R[n, k, j] / (hfac lam_j + delta)``; ``R [N, C, P]`` = ``Js Q``"""
        _check(R, "R"), _check(lam, "lam"), _check(delta, "delta")
        N, C, P = R.shape
        if lam.shape != (P,) or delta.numel() != 1:
            raise LaplaceHipError("spectral_quadform: R [N, C, P], lam [P], delta a scalar tensor")
        fvar = torch.empty(N, C, C, dtype=torch.float32, device=R.device)
        ws = self._workspace(self.lib.lk_spectral_workspace_bytes(self.SP_QUAD_R, N, C, P, 1), R.device)
        self._rc(self.lib.lk_spectral_quadform_f32(_ptr(R), _ptr(lam), float(hfac), _ptr(delta), N, C, P, _ptr(fvar), _ptr(ws),
                                                   ws.numel(), self._stream(R.device)), "lk_spectral_quadform_f32")
        return fvar

    def spectral_grid(self, R, lam, hfac, deltas, var):
        """``var [G, N, C] += sum_j R[n, c, j]^2 / (hfac lam_j + deltas[g])``"""
        _check(R, "R"), _check(lam, "lam"), _check(deltas, "deltas"), _check(var, "var")
        N, C, P = R.shape
        G = deltas.numel()
        if lam.shape != (P,) or var.shape != (G, N, C):
            raise LaplaceHipError("spectral_grid: R [N, C, P], lam [P], var [G, N, C]")
        ws = self._workspace(self.lib.lk_spectral_workspace_bytes(self.SP_GRID_R, N, C, P, G), R.device)
        self._rc(self.lib.lk_spectral_grid_f32(_ptr(R), _ptr(lam), float(hfac), _ptr(deltas), G, N, C, P, _ptr(var), _ptr(ws),
                                               ws.numel(), self._stream(R.device)), "lk_spectral_grid_f32")
        return var

    def spectral_variant(self, form, N, C, D_or_P, G=1, aligned=True):
        """what a shape launches (host only): ``dict(ct, grid, pairs, ll, split, gc)`` or None for a refused shape"""
        r = self.lib.lk_spectral_variant(int(form), N, C, D_or_P, G, 1 if aligned else 0)
        if r < 0:
            return None
        return {"ct": r & 15, "grid": bool(r & 16), "pairs": bool(r & 32), "ll": bool(r & 64), "split": (r >> 8) & 4095,
                "gc": r >> 20}


_KERNELS = None


def get_kernels():
    """The process-wide kernel provider (loads the HIP library on first use; raises if absent)."""
    global _KERNELS
    if _KERNELS is None:
        _KERNELS = HipKernels()
    return _KERNELS


def set_kernels_for_testing(impl):
    """Install a stand-in provider (CPU emulation of the kernels, used only by the `not gpu` tests
    of the host logic).  Returns the previous provider."""
    global _KERNELS
    prev = _KERNELS
    _KERNELS = impl
    return prev
