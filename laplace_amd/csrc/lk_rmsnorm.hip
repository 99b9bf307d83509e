// Forward and input VJP of nn.RMSNorm (the pre-norm of LLaMA / Mistral / Gemma / T5 blocks) for the seed-batched reverse sweep:
//   forward   r = 1 / sqrt(mean_row(x^2) + eps);  y = w * (x * r)
//   VJP       t = w * g;  xh = x * r;  m2 = mean_row(t * xh);  dx = r * (t - xh * m2)     for all S seeds
// Replaces the reverse passes through this layer of laplace/curvature/curvlinops.py:87-100 and curvature.py:88-129 (one stock
// autograd pass per seed).  Unlike LayerNorm (lk_normvjp.hip) nothing is subtracted: the mean of squares has non-negative terms
// only, there is no mean_row(t) term, and xhat is one multiply away from x, so the forward stores y and rstd [rows] alone and
// the VJP forms xh from x and rstd.
//
// A row kernel (lk_stream.h) on a plain [rows][D] matrix: a group of W lanes (a power of two <= 64) owns a row and
// reduces with a fixed xor-shuffle tree; xh and w of the row stay in registers across the seed loop while the row fits
// (RMS_NV vectors per lane) with two seeds' g in flight; longer rows read g twice.  16-byte loads where D % 4 == 0 and the
// pointers are 16-byte aligned, 4-byte loads otherwise.  Deterministic: every element has one owner, plain vector stores, no
// atomics on data; `amax` receives max|dx| as a bit pattern through atomicMax (order-independent).  Few rows: the seeds are split
// over grid.y.
#include "lk_stream.h"

namespace lk {

constexpr int RMS_SC = 2;  // seeds per pass of the on-chip path (their g tiles are in flight together)
constexpr int RMS_NV = 8;  // vectors of a row a lane keeps on chip

// w of vector i of a row (1 for a null pointer); a 16-byte load when VEC == 4 (the entry points count w into `aligned`)
template <int VEC>
__device__ __forceinline__ void rms_weight(const float* __restrict__ w, int i, float (&v)[VEC]) {
  if (w != nullptr) {
    ld<VEC>(w + (int64_t)i * VEC, v);
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = 1.f;
  }
}

// ---- forward: fp32 mean of squares, no subtraction anywhere ---------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(256) void rmsnorm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, int64_t R,
                                                          int D, int W, float eps, float* __restrict__ y,
                                                          float* __restrict__ rstd) {
  const int64_t row = (int64_t)blockIdx.x * (256 / W) + threadIdx.x / W;
  const int lane = threadIdx.x & (W - 1);
  const bool live = row < R;  // (dead groups stay in the shuffles and touch no memory)
  const int64_t base = live ? row * D : 0;
  const int nvec = live ? D / VEC : 0;
  float sq = 0.f;
  for (int i = lane; i < nvec; i += W) {  // (D < 2^30: i + W stays below 2^31)
    float v[VEC];
    ld<VEC>(x + base + (int64_t)i * VEC, v);
#pragma unroll
    for (int e = 0; e < VEC; ++e) sq += v[e] * v[e];
  }
  for (int off = W >> 1; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
  const float rs = 1.0f / sqrtf(sq / (float)D + eps);
  for (int i = lane; i < nvec; i += W) {
    float v[VEC], wv[VEC], yv[VEC];
    const int64_t o = base + (int64_t)i * VEC;
    ld<VEC>(x + o, v);
    rms_weight<VEC>(w, i, wv);
#pragma unroll
    for (int e = 0; e < VEC; ++e) yv[e] = wv[e] * (v[e] * rs);
    st<VEC>(y + o, yv);
  }
  if (live && lane == 0) rstd[row] = rs;
}

// ---- VJP ------------------------------------------------------------------------------------------------------------------------
template <int VEC, bool ONCHIP>
__global__ __launch_bounds__(256) void rmsnorm_vjp_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                          const float* __restrict__ rstd, const float* __restrict__ w, int S,
                                                          int64_t R, int D, int W, int s_per, int64_t seed_stride,
                                                          float* __restrict__ dx, unsigned* __restrict__ amax) {
  const int64_t row = (int64_t)blockIdx.x * (256 / W) + threadIdx.x / W;
  const int lane = threadIdx.x & (W - 1);
  const bool live = row < R;
  const int64_t base = live ? row * D : 0;
  const int nvec = live ? D / VEC : 0;
  const float rs = live ? rstd[row] : 0.f;
  const float fn = (float)D;
  const int s_begin = blockIdx.y * s_per;
  const int s_end = min(S, s_begin + s_per);
  float vmax = 0.f;
  if constexpr (ONCHIP) {
    float xh[RMS_NV][VEC], wv[RMS_NV][VEC];
    int64_t off[RMS_NV];
#pragma unroll
    for (int k = 0; k < RMS_NV; ++k) {
      const int i = k * W + lane;
      off[k] = -1;  // (no vector of the row here)
#pragma unroll
      for (int e = 0; e < VEC; ++e) xh[k][e] = wv[k][e] = 0.f;
      if (i < nvec) {
        off[k] = base + (int64_t)i * VEC;
        ld<VEC>(x + off[k], xh[k]);
        rms_weight<VEC>(w, i, wv[k]);
#pragma unroll
        for (int e = 0; e < VEC; ++e) xh[k][e] *= rs;
      }
    }
    for (int s0 = s_begin; s0 < s_end; s0 += RMS_SC) {
      float t[RMS_SC][RMS_NV][VEC], a2[RMS_SC];
#pragma unroll
      for (int j = 0; j < RMS_SC; ++j) {
        a2[j] = 0.f;
        const bool on = s0 + j < s_end;  // (uniform over the workgroup)
        const float* gs = g + (int64_t)(s0 + j) * seed_stride;
#pragma unroll
        for (int k = 0; k < RMS_NV; ++k) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) t[j][k][e] = 0.f;
          if (on && off[k] >= 0) {
            ld<VEC>(gs + off[k], t[j][k]);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              t[j][k][e] *= wv[k][e];
              a2[j] += t[j][k][e] * xh[k][e];
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < RMS_SC; ++j)
        for (int o = W >> 1; o > 0; o >>= 1) a2[j] += __shfl_xor(a2[j], o, 64);
#pragma unroll
      for (int j = 0; j < RMS_SC; ++j) {
        if (s0 + j >= s_end) continue;
        const float m2 = a2[j] / fn;
        float* ds = dx + (int64_t)(s0 + j) * seed_stride;
#pragma unroll
        for (int k = 0; k < RMS_NV; ++k) {
          if (off[k] >= 0) {
            float d[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              d[e] = rs * (t[j][k][e] - xh[k][e] * m2);
              vmax = fmaxf(vmax, fabsf(d[e]));
            }
            st<VEC>(ds + off[k], d);
          }
        }
      }
    }
  } else {
    for (int s = s_begin; s < s_end; ++s) {
      const float* gs = g + (int64_t)s * seed_stride;
      float* ds = dx + (int64_t)s * seed_stride;
      float a2 = 0.f;
#pragma unroll 4
      for (int i = lane; i < nvec; i += W) {
        float gv[VEC], xv[VEC], wv[VEC];
        const int64_t o = base + (int64_t)i * VEC;
        ld<VEC>(gs + o, gv);
        ld<VEC>(x + o, xv);
        rms_weight<VEC>(w, i, wv);
#pragma unroll
        for (int e = 0; e < VEC; ++e) a2 += (gv[e] * wv[e]) * (xv[e] * rs);
      }
      for (int o = W >> 1; o > 0; o >>= 1) a2 += __shfl_xor(a2, o, 64);
      const float m2 = a2 / fn;
#pragma unroll 4
      for (int i = lane; i < nvec; i += W) {
        float gv[VEC], xv[VEC], wv[VEC], d[VEC];
        const int64_t o = base + (int64_t)i * VEC;
        ld<VEC>(gs + o, gv);
        ld<VEC>(x + o, xv);
        rms_weight<VEC>(w, i, wv);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          d[e] = rs * (gv[e] * wv[e] - (xv[e] * rs) * m2);
          vmax = fmaxf(vmax, fabsf(d[e]));
        }
        st<VEC>(ds + o, d);
      }
    }
  }
  wave_amax(vmax, amax);
}

// ---- host: which path a shape takes ---------------------------------------------------------------------------------------------
struct RmsPlan {
  int vec;      // 16-byte loads
  int twopass;  // the row does not stay on chip
  int W;        // lanes per row
  int s_per;    // seeds per grid.y slice
  int64_t blocks;
};

// false: a shape outside the contract of the entry points (which refuse it with a message of their own)
static bool rmsnorm_plan(int64_t S, int64_t rows, int64_t D, bool aligned, RmsPlan* p) {
  if (S < 1 || S >= (1ll << 31) || rows < 0 || rows >= (1ll << 31) || D < 1 || D >= (1ll << 30)) return false;
  if ((unsigned __int128)S * (unsigned __int128)rows * (unsigned __int128)D >= ((unsigned __int128)1 << 40)) return false;
  p->vec = aligned && D % 4 == 0;
  const int64_t nvec = p->vec ? D / 4 : D;
  p->W = pow2_ceil(nvec, 64);
  p->twopass = nvec > (int64_t)p->W * RMS_NV;
  p->blocks = (rows + 256 / p->W - 1) / (256 / p->W);
  p->s_per = seeds_per_slice(S, p->blocks * 4);
  return true;
}

#define LK_RMSNORM_REQUIRE_SHAPE(FN, S, rows, D)                                                                          \
  LK_REQUIRE(S >= 1 && S < (1ll << 31) && rows >= 0 && rows < (1ll << 31) && D >= 1 && D < (1ll << 30),                    \
             FN ": extent out of range (1 <= S < 2^31, 0 <= rows < 2^31, 1 <= D < 2^30)");                                 \
  LK_REQUIRE((unsigned __int128)S * (unsigned __int128)rows * (unsigned __int128)D < ((unsigned __int128)1 << 40),        \
             FN ": too many elements (S * rows * D < 2^40)")

static int rmsnorm_check_fwd(const float* x, const float* w, int64_t rows, int64_t D, const float* y, const float* rstd,
                             RmsPlan* plan) {
  LK_REQUIRE(x && y && rstd, "lk_rmsnorm_fwd_f32: null pointer");
  LK_RMSNORM_REQUIRE_SHAPE("lk_rmsnorm_fwd_f32", 1, rows, D);
  const bool aligned = (((uintptr_t)x | (uintptr_t)y | (uintptr_t)w) & 15) == 0;
  rmsnorm_plan(1, rows, D, aligned, plan);
  return LK_OK;
}

static int rmsnorm_check_vjp(const float* g, const float* x, const float* rstd, const float* w, int64_t S, int64_t rows,
                             int64_t D, const float* dx, RmsPlan* plan) {
  LK_REQUIRE(g && x && rstd && dx, "lk_rmsnorm_vjp_f32: null pointer");
  LK_RMSNORM_REQUIRE_SHAPE("lk_rmsnorm_vjp_f32", S, rows, D);
  const unsigned __int128 bytes = (unsigned __int128)S * rows * D * 4;
  const unsigned __int128 g0 = (uintptr_t)g, d0 = (uintptr_t)dx;
  LK_REQUIRE(g0 + bytes <= d0 || d0 + bytes <= g0, "lk_rmsnorm_vjp_f32: dx overlaps g");
  const bool aligned = (((uintptr_t)g | (uintptr_t)x | (uintptr_t)dx | (uintptr_t)w) & 15) == 0;
  rmsnorm_plan(S, rows, D, aligned, plan);
  return LK_OK;
}

}  // namespace lk

using namespace lk;

extern "C" int lk_rmsnorm_fwd_f32(const float* x, const float* w, int64_t rows, int64_t D, float eps, float* y, float* rstd,
                                  void* stream) {
  RmsPlan p;
  const int rc = rmsnorm_check_fwd(x, w, rows, D, y, rstd, &p);
  if (rc != LK_OK) return rc;
  if (rows == 0) return LK_OK;
  hipStream_t st = (hipStream_t)stream;
  if (p.vec)
    hipLaunchKernelGGL(rmsnorm_fwd_kernel<4>, dim3((unsigned)p.blocks), dim3(256), 0, st, x, w, rows, (int)D, p.W, eps, y, rstd);
  else
    hipLaunchKernelGGL(rmsnorm_fwd_kernel<1>, dim3((unsigned)p.blocks), dim3(256), 0, st, x, w, rows, (int)D, p.W, eps, y, rstd);
  return check_launch("rmsnorm_fwd_kernel");
}

extern "C" int lk_rmsnorm_vjp_f32(const float* g, const float* x, const float* rstd, const float* w, int64_t S, int64_t rows,
                                  int64_t D, float* dx, unsigned* amax, void* stream) {
  RmsPlan p;
  const int rc = rmsnorm_check_vjp(g, x, rstd, w, S, rows, D, dx, &p);
  if (rc != LK_OK) return rc;
  if (rows == 0) return LK_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)p.blocks, (unsigned)((S + p.s_per - 1) / p.s_per));
  const int64_t seed_stride = rows * D;
#define LK_RMS_ROW(V, ON)                                                                                                   \
  hipLaunchKernelGGL((rmsnorm_vjp_kernel<V, ON>), grid, dim3(256), 0, st, g, x, rstd, w, (int)S, rows, (int)D, p.W, p.s_per, \
                     seed_stride, dx, amax)
  if (p.vec && !p.twopass) LK_RMS_ROW(4, true);
  else if (p.vec) LK_RMS_ROW(4, false);
  else if (!p.twopass) LK_RMS_ROW(1, true);
  else LK_RMS_ROW(1, false);
#undef LK_RMS_ROW
  return check_launch("rmsnorm_vjp_kernel");
}

// vec | two-pass << 1 | seed-split << 2 | log2(lanes) << 3 | min(seeds per slice, 2^24 - 1) << 6
extern "C" int lk_rmsnorm_variant(int64_t S, int64_t rows, int64_t D, int aligned) {
  RmsPlan p;
  if (!rmsnorm_plan(S, rows, D, aligned != 0, &p)) return -1;
  int lg = 0;
  while ((1 << lg) < p.W) ++lg;
  const int sp = p.s_per < (1 << 24) - 1 ? p.s_per : (1 << 24) - 1;
  return p.vec | p.twopass << 1 | (p.s_per < S ? 1 : 0) << 2 | lg << 3 | sp << 6;
}
