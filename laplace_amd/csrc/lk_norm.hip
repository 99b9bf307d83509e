// Per-sample Jacobian of an affine normalisation layer y = w * xhat + b (BatchNorm1d/2d in eval mode, LayerNorm,
// GroupNorm) with respect to w and b, for all seeds of a reverse sweep:
//   Js[n][s][wcol0 + ch] = sum_l g[s][n][l, ch] * xhat[n][l, ch]        Js[n][s][bcol0 + ch] = sum_l g[s][n][l, ch]
// Replaces the norm-parameter columns of the jacrev materialisation of CurvatureInterface.jacobians
// (laplace/curvature/curvature.py:88-129) and of GGNInterface.diag / EFInterface.diag (curvature.py:413-433, 494-505).
//
// A streaming reduction bound by the single read of g (S times the size of xhat).  Both layouts read fp32 (the
// channels-last one too: it takes fp32 NHWC / [.., D] cotangents, not the sweep's split fp16 planes) with 16-byte loads
// per lane where the reduced / channel extent is a multiple of 4 floats and the pointers are 16-byte aligned, 4-byte
// loads otherwise.  A lane keeps its tile of xhat in registers across the seed loop, so xhat is read once per pass of
// NORM_SC seeds and not once per seed.  Deterministic: no atomics, every output element has ONE owner (a lane group
// of W lanes, reduced with a fixed xor-shuffle tree, or a column of the workgroup, reduced through LDS with a fixed
// halving tree); plain vector stores.  Parallelism comes from the rows (n, ch) and, when those are few, from splitting
// the SEEDS over grid.y (every split re-reads xhat, 1/s_per of its cotangent traffic) - not from splitting L, so no
// second stage is needed.
#include "lk_stream.h"

namespace lk {

constexpr int NORM_SC = 16;    // seeds per pass of the channels-first kernel (2 accumulators each, in registers)
constexpr int NORM_NV = 4;     // vectors of xhat a lane holds per tile of the reduced extent
constexpr int NORM_SC_CL = 8;  // seeds per pass of the channels-last kernel (2 * VEC accumulators each)

// Channels first: g [S][R][L], xhat [R][L] with R = B * Ch rows (n, ch).  A group of W lanes (W a power of two <= 64,
// W * VEC >= min(L, 64 * VEC)) owns one row; a workgroup of 256 lanes owns 256 / W consecutive rows; grid.y splits seeds.
template <int VEC>
__global__ __launch_bounds__(256) void jac_norm_cf_kernel(const float* __restrict__ g, const float* __restrict__ xhat,
                                                          int S, int64_t R, int Ch, int L, int W, int s_per,
                                                          float* __restrict__ Js, int64_t P, int64_t wcol0,
                                                          int64_t bcol0) {
  const int64_t row = (int64_t)blockIdx.x * (256 / W) + threadIdx.x / W;
  const int lane = threadIdx.x & (W - 1);
  const bool live = row < R;  // (dead groups stay in the shuffles and touch no memory)
  const int s_begin = blockIdx.y * s_per;
  const int s_end = min(S, s_begin + s_per);
  const int64_t seed_stride = R * L;
  const int64_t row_off = row * L;
  const int tile = W * VEC * NORM_NV;
  for (int s0 = s_begin; s0 < s_end; s0 += NORM_SC) {
    float aw[NORM_SC], ab[NORM_SC];
#pragma unroll
    for (int k = 0; k < NORM_SC; ++k) aw[k] = ab[k] = 0.f;
    for (int l0 = 0; l0 < L; l0 += tile) {
      float xv[NORM_NV][VEC];
#pragma unroll
      for (int v = 0; v < NORM_NV; ++v) {
        const int l = l0 + (v * W + lane) * VEC;
#pragma unroll
        for (int e = 0; e < VEC; ++e) xv[v][e] = 0.f;
        if (live && l < L) ld<VEC>(xhat + row_off + l, xv[v]);
      }
#pragma unroll
      for (int k = 0; k < NORM_SC; ++k) {
        if (s0 + k < s_end) {  // (wave-uniform)
          const float* gr = g + (int64_t)(s0 + k) * seed_stride + row_off;
#pragma unroll
          for (int v = 0; v < NORM_NV; ++v) {
            const int l = l0 + (v * W + lane) * VEC;
            if (live && l < L) {
              float gv[VEC];
              ld<VEC>(gr + l, gv);
#pragma unroll
              for (int e = 0; e < VEC; ++e) {
                aw[k] += gv[e] * xv[v][e];
                ab[k] += gv[e];
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < NORM_SC; ++k) {
      if (s0 + k < s_end) {
        for (int off = W >> 1; off > 0; off >>= 1) {
          aw[k] += __shfl_xor(aw[k], off, 64);
          ab[k] += __shfl_xor(ab[k], off, 64);
        }
        if (live && lane == 0) {
          const int64_t n = row / Ch;
          const int ch = (int)(row - n * Ch);
          float* out = Js + (n * S + (s0 + k)) * P;
          if (wcol0 >= 0) out[wcol0 + ch] = aw[k];
          if (bcol0 >= 0) out[bcol0 + ch] = ab[k];
        }
      }
    }
  }
}

// Channels last: g [S][B][L][Ch], xhat [B][L][Ch].  A workgroup owns CXW channel vectors (a power of two <= 64) of one
// sample; its 256 / CXW lane rows stride over the positions l and are summed through LDS, one seed at a time.
template <int VEC>
__global__ __launch_bounds__(256) void jac_norm_cl_kernel(const float* __restrict__ g, const float* __restrict__ xhat,
                                                          int S, int B, int L, int Ch, int CXW, int s_per,
                                                          float* __restrict__ Js, int64_t P, int64_t wcol0,
                                                          int64_t bcol0) {
  __shared__ float red[256 * 2 * VEC];
  const int CV = Ch / VEC;
  const int tiles = (CV + CXW - 1) / CXW;
  const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
  const int tx = threadIdx.x & (CXW - 1), ty = threadIdx.x / CXW, TL = 256 / CXW;
  const int cv = tile * CXW + tx;
  const bool live = cv < CV;
  const int s_begin = blockIdx.y * s_per;
  const int s_end = min(S, s_begin + s_per);
  const float* xn = xhat + (int64_t)n * L * Ch + (int64_t)cv * VEC;
  float* mine = red + (size_t)threadIdx.x * 2 * VEC;
  for (int s0 = s_begin; s0 < s_end; s0 += NORM_SC_CL) {
    float aw[NORM_SC_CL][VEC], ab[NORM_SC_CL][VEC];
#pragma unroll
    for (int k = 0; k < NORM_SC_CL; ++k)
#pragma unroll
      for (int e = 0; e < VEC; ++e) aw[k][e] = ab[k][e] = 0.f;
    if (live) {
      for (int l = ty; l < L; l += TL) {
        float xv[VEC];
        ld<VEC>(xn + (int64_t)l * Ch, xv);
#pragma unroll
        for (int k = 0; k < NORM_SC_CL; ++k) {
          if (s0 + k < s_end) {
            float gv[VEC];
            ld<VEC>(g + (((int64_t)(s0 + k) * B + n) * L + l) * Ch + (int64_t)cv * VEC, gv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              aw[k][e] += gv[e] * xv[e];
              ab[k][e] += gv[e];
            }
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < NORM_SC_CL; ++k) {
      if (s0 + k < s_end) {  // (uniform over the workgroup: the barriers below are reached by all or none)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          mine[e] = aw[k][e];
          mine[VEC + e] = ab[k][e];
        }
        __syncthreads();
        for (int st = TL >> 1; st > 0; st >>= 1) {
          if (ty < st) {
            const float* other = red + (size_t)(threadIdx.x + st * CXW) * 2 * VEC;
#pragma unroll
            for (int e = 0; e < 2 * VEC; ++e) mine[e] += other[e];
          }
          __syncthreads();
        }
        if (ty == 0 && live) {
          float* out = Js + ((int64_t)n * S + (s0 + k)) * P;
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            if (wcol0 >= 0) out[wcol0 + cv * VEC + e] = mine[e];
            if (bcol0 >= 0) out[bcol0 + cv * VEC + e] = mine[VEC + e];
          }
        }
        __syncthreads();
      }
    }
  }
}

}  // namespace lk

using namespace lk;

extern "C" int lk_jac_norm_affine_f32(const float* g, const float* xhat, int64_t S, int64_t B, int64_t L, int64_t Ch,
                                      int layout, float* Js, int64_t P, int64_t wcol0, int64_t bcol0, void* stream) {
  LK_REQUIRE(g && xhat && Js && S >= 1 && B >= 0 && L >= 1 && Ch >= 1 && (layout == 0 || layout == 1),
             "lk_jac_norm_affine_f32: bad arguments");
  LK_REQUIRE(S < (1ll << 31) && B < (1ll << 31) && L < (1ll << 30) && Ch < (1ll << 30) && B * Ch < (1ll << 40),
             "lk_jac_norm_affine_f32: extent too large");
  LK_REQUIRE((wcol0 < 0 || wcol0 + Ch <= P) && (bcol0 < 0 || bcol0 + Ch <= P),
             "lk_jac_norm_affine_f32: column range outside Js");
  LK_REQUIRE(wcol0 < 0 || bcol0 < 0 || wcol0 + Ch <= bcol0 || bcol0 + Ch <= wcol0,
             "lk_jac_norm_affine_f32: weight and bias columns overlap");
  if (B == 0 || (wcol0 < 0 && bcol0 < 0)) return LK_OK;
  const bool aligned = (((uintptr_t)g | (uintptr_t)xhat) & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  if (layout == 0 || L == 1) {  // (one position: both layouts are [S][B][Ch], a row per element, a lane per row)
    const int64_t R = B * Ch;
    const bool vec = aligned && L % 4 == 0;
    const int W = pow2_ceil(vec ? L / 4 : L, 64);
    const int64_t blocks = (R * W + 255) / 256;
    LK_REQUIRE(blocks < (1ll << 31), "lk_jac_norm_affine_f32: too many rows for one launch");
    const int s_per = seeds_per_slice(S, blocks * 4);
    dim3 grid((unsigned)blocks, (unsigned)((S + s_per - 1) / s_per));
    if (vec)
      hipLaunchKernelGGL(jac_norm_cf_kernel<4>, grid, dim3(256), 0, st, g, xhat, (int)S, R, (int)Ch, (int)L, W, s_per,
                         Js, P, wcol0, bcol0);
    else
      hipLaunchKernelGGL(jac_norm_cf_kernel<1>, grid, dim3(256), 0, st, g, xhat, (int)S, R, (int)Ch, (int)L, W, s_per,
                         Js, P, wcol0, bcol0);
    return check_launch("jac_norm_cf_kernel");
  }
  const bool vec = aligned && Ch % 4 == 0;
  const int CXW = pow2_ceil(vec ? Ch / 4 : Ch, 64);
  const int64_t tiles = ((vec ? Ch / 4 : Ch) + CXW - 1) / CXW;
  const int64_t blocks = B * tiles;
  LK_REQUIRE(blocks < (1ll << 31), "lk_jac_norm_affine_f32: too many channel tiles for one launch");
  const int s_per = seeds_per_slice(S, blocks * 4);
  dim3 grid((unsigned)blocks, (unsigned)((S + s_per - 1) / s_per));
  if (vec)
    hipLaunchKernelGGL(jac_norm_cl_kernel<4>, grid, dim3(256), 0, st, g, xhat, (int)S, (int)B, (int)L, (int)Ch, CXW,
                       s_per, Js, P, wcol0, bcol0);
  else
    hipLaunchKernelGGL(jac_norm_cl_kernel<1>, grid, dim3(256), 0, st, g, xhat, (int)S, (int)B, (int)L, (int)Ch, CXW,
                       s_per, Js, P, wcol0, bcol0);
  return check_launch("jac_norm_cl_kernel");
}
