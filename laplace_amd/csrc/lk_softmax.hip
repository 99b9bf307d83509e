// Softmax / log-softmax along the last dim (hand-written attention p = softmax(q k^T / sqrt(d)), attention pooling, soft mixture
// gates, log-softmax head features) for the seed-batched reverse sweep.  With the cotangent g of y = softmax(x) for all S seeds
// stacked, g [S][R][L], and ONE y [R][L] per sample row shared by all seeds:
//   softmax      dx[s][r][l] = y[r][l] * (g[s][r][l] - sum_j g[s][r][j] y[r][j])
//   log-softmax  dx[s][r][l] = g[s][r][l] - exp(y[r][l]) * sum_j g[s][r][j]
// Replaces, in the reverse pass of laplace/curvature/curvlinops.py:87-100 and curvature.py:88-129 through a softmax as stock torch
// runs it once per seed: `_softmax_backward_data` / `_log_softmax_backward_data` on [B, ...], S launches that each read y again.
// Here one launch serves all seeds and y (for the log form exp(y), computed ONCE) of a row stays in registers across the seed loop.
//
// One kernel template (lk_stream.h; the ROW body of lk_mul.hip): a group of W lanes (a power of two <= 64, so a group never
// leaves its wave) owns one row; the row sum is a fixed xor-shuffle tree over the group.  While the row fits (SMX_NV vectors per
// lane: RESIDENT) y and the seed's g stay in registers between the sum and the store; longer rows re-read both per seed.  16-byte
// loads and stores where L % 4 == 0 and every pointer is 16-byte aligned, 4-byte ones otherwise.  Few rows: the seeds are split
// over grid.y.  Every output element has one owner, stores are plain vector stores, there is no atomic: repeated runs give the same
// bits.  A probability that is exactly zero (a masked key) gives dx = 0 * (finite) = 0 exactly.  Nothing assumes packed fp32.
// Minimal traffic: g once and dx once (8 S R L bytes), y once.
#include "lk_stream.h"

namespace lk {

constexpr int SMX_NV = 8;  // vectors of a row a lane keeps in registers (RESIDENT)

// what the row sum adds (g y / g) and what the element gets from it
template <bool LOG>
__device__ __forceinline__ float smx_term(float g, float p) {
  return LOG ? g : g * p;
}
template <bool LOG>
__device__ __forceinline__ float smx_out(float g, float p, float sum) {
  return LOG ? g - p * sum : p * (g - sum);
}

template <int VEC, bool LOG, bool RESIDENT>
__global__ __launch_bounds__(256) void softmax_vjp_kernel(const float* __restrict__ g, const float* __restrict__ y, int64_t S,
                                                          int64_t R, int L, int W, int64_t s_per, float* __restrict__ dx) {
  const int64_t seed_stride = R * (int64_t)L;
  const int64_t s_begin = (int64_t)blockIdx.y * s_per;
  const int64_t s_end = s_begin + s_per < S ? s_begin + s_per : S;
  const int rpb = 256 / W;  // rows per workgroup
  const int lane = threadIdx.x & (W - 1);
  const int nvec_row = L / VEC;
  // (the trip count is uniform over the workgroup: dead groups stay in the shuffles and touch no memory)
  for (int64_t row0 = (int64_t)blockIdx.x * rpb; row0 < R; row0 += (int64_t)gridDim.x * rpb) {
    const int64_t row = row0 + threadIdx.x / W;
    const bool live = row < R;
    const int nvec = live ? nvec_row : 0;
    const int64_t base = (live ? row : 0) * (int64_t)L;
    if constexpr (RESIDENT) {
      float pv[SMX_NV][VEC];
#pragma unroll
      for (int k = 0; k < SMX_NV; ++k) {
        const int i = k * W + lane;
#pragma unroll
        for (int e = 0; e < VEC; ++e) pv[k][e] = 0.f;
        if (i < nvec) {
          ld<VEC>(y + base + (int64_t)i * VEC, pv[k]);
          if constexpr (LOG) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) pv[k][e] = expf(pv[k][e]);
          }
        }
      }
      for (int64_t s = s_begin; s < s_end; ++s) {
        const float* gs = g + s * seed_stride + base;
        float gv[SMX_NV][VEC];
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < SMX_NV; ++k) {
          const int i = k * W + lane;
#pragma unroll
          for (int e = 0; e < VEC; ++e) gv[k][e] = 0.f;
          if (i < nvec) {
            ld<VEC>(gs + (int64_t)i * VEC, gv[k]);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc += smx_term<LOG>(gv[k][e], pv[k][e]);
          }
        }
        for (int o = W >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
#pragma unroll
        for (int k = 0; k < SMX_NV; ++k) {
          const int i = k * W + lane;
          if (i < nvec) {
            float d[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) d[e] = smx_out<LOG>(gv[k][e], pv[k][e], acc);
            st<VEC>(dx + s * seed_stride + base + (int64_t)i * VEC, d);
          }
        }
      }
    } else {
      for (int64_t s = s_begin; s < s_end; ++s) {
        const float* gs = g + s * seed_stride + base;
        float acc = 0.f;
        for (int i = lane; i < nvec; i += W) {  // (nvec < 2^30 and W <= 64: no overflow)
          float gv[VEC], pv[VEC];
          ld<VEC>(gs + (int64_t)i * VEC, gv);
#pragma unroll
          for (int e = 0; e < VEC; ++e) pv[e] = 0.f;
          if constexpr (!LOG) ld<VEC>(y + base + (int64_t)i * VEC, pv);  // (the log form sums g alone)
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc += smx_term<LOG>(gv[e], pv[e]);
        }
        for (int o = W >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        for (int i = lane; i < nvec; i += W) {
          float gv[VEC], pv[VEC], d[VEC];
          ld<VEC>(gs + (int64_t)i * VEC, gv);
          ld<VEC>(y + base + (int64_t)i * VEC, pv);
#pragma unroll
          for (int e = 0; e < VEC; ++e) d[e] = smx_out<LOG>(gv[e], LOG ? expf(pv[e]) : pv[e], acc);
          st<VEC>(dx + s * seed_stride + base + (int64_t)i * VEC, d);
        }
      }
    }
  }
}

// ---- host: the contract and the path of a shape ----------------------------------------------------------------------------------
struct SoftmaxPlan {
  int vec;       // 16-byte accesses
  int W;         // lanes per row
  int resident;  // y and the seed's g of a row stay in registers
  int wide;      // an element offset of g does not fit 31 bits (the kernel indexes with 64 bits throughout)
  int64_t s_per; // seeds per grid.y slice
  int64_t blocks;
};

// the shape part of the contract (shared with lk_softmax_vjp_variant), with the messages under the caller's name
static int softmax_check_shape(const char* fn, int64_t S, int64_t R, int64_t L, int is_log, bool aligned, SoftmaxPlan* p) {
  LK_REQUIRE(is_log == 0 || is_log == 1, "%s: is_log must be 0 (y = softmax) or 1 (y = log_softmax)", fn);
  LK_REQUIRE(S >= 1 && R >= 0 && L >= 1 && L < (1ll << 30), "%s: extent out of range (1 <= S, 0 <= R, 1 <= L < 2^30)", fn);
  LK_REQUIRE((unsigned __int128)S * (unsigned __int128)R * (unsigned __int128)L < ((unsigned __int128)1 << 40),
             "%s: extent out of range (S * R * L < 2^40)", fn);
  p->vec = aligned && L % 4 == 0;
  p->wide = S * R * L >= (1ll << 31);
  const int64_t nvec = p->vec ? L / 4 : L;
  p->W = pow2_ceil(nvec, 64);
  p->resident = nvec <= (int64_t)p->W * SMX_NV;
  const int rpb = 256 / p->W;
  p->blocks = (R + rpb - 1) / rpb;
  if (p->blocks > STREAM_MAX_BLOCKS) p->blocks = STREAM_MAX_BLOCKS;
  p->s_per = seeds_per_slice(S, p->blocks * 4);
  return LK_OK;
}

static int softmax_check(const float* g, const float* y, int64_t S, int64_t R, int64_t L, int is_log, const float* dx,
                         SoftmaxPlan* p) {
  LK_REQUIRE(g && y && dx, "lk_softmax_vjp_f32: null pointer");
  const uintptr_t bits = (uintptr_t)g | (uintptr_t)y | (uintptr_t)dx;
  const int rc = softmax_check_shape("lk_softmax_vjp_f32", S, R, L, is_log, (bits & 15) == 0, p);
  if (rc != LK_OK) return rc;
  const unsigned __int128 rl = (unsigned __int128)R * L * 4, gb = rl * S;
  LK_REQUIRE(disjoint(dx, gb, g, gb) && disjoint(dx, gb, y, rl), "lk_softmax_vjp_f32: dx overlaps an input");
  return LK_OK;
}

}  // namespace lk

using namespace lk;

extern "C" int lk_softmax_vjp_f32(const float* g, const float* y, int64_t S, int64_t R, int64_t L, int is_log, float* dx,
                                  void* stream) {
  SoftmaxPlan p;
  const int rc = softmax_check(g, y, S, R, L, is_log, dx, &p);
  if (rc != LK_OK) return rc;
  if (R == 0) return LK_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)p.blocks, (unsigned)((S + p.s_per - 1) / p.s_per));
#define LK_SMX(V, LOG, RES) \
  hipLaunchKernelGGL((softmax_vjp_kernel<V, LOG, RES>), grid, dim3(256), 0, st, g, y, S, R, (int)L, p.W, p.s_per, dx)
#define LK_SMX_RES(V, LOG)     \
  do {                         \
    if (p.resident)            \
      LK_SMX(V, LOG, true);    \
    else                       \
      LK_SMX(V, LOG, false);   \
  } while (0)
  if (p.vec) {
    if (is_log) LK_SMX_RES(4, true);
    else LK_SMX_RES(4, false);
  } else {
    if (is_log) LK_SMX_RES(1, true);
    else LK_SMX_RES(1, false);
  }
#undef LK_SMX_RES
#undef LK_SMX
  return check_launch("softmax_vjp_kernel");
}

// vec | log2(lanes per row) << 1 | resident << 4 | seed-split << 5 | wide << 6 | is_log << 7 | workgroups << 8
extern "C" int lk_softmax_vjp_variant(int64_t S, int64_t R, int64_t L, int is_log, int aligned) {
  SoftmaxPlan p;
  if (softmax_check_shape("lk_softmax_vjp_variant", S, R, L, is_log, aligned != 0, &p) != LK_OK) return -1;
  int lg = 0;
  while ((1 << lg) < p.W) ++lg;
  return p.vec | lg << 1 | p.resident << 4 | (p.s_per < S ? 1 : 0) << 5 | p.wide << 6 | is_log << 7 | (int)p.blocks << 8;
}
