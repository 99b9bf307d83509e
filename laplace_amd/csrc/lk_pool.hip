// Max and average pooling on fp32 NHWC feature maps for the seed-batched reverse sweep (nn.MaxPool2d / nn.AvgPool2d,
// F.max_pool2d / F.avg_pool2d; ceil_mode false, no dilation):
//   forward   y[n, oh, ow, c] = max / mean over the in-image taps of the window at (oh * sh - ph, ow * sw - pw);
//             max also writes arg[n, oh, ow, c] = dy * kw + dx of the FIRST maximum in row-major scan order (strict >, the
//             tie rule of torch.max_pool2d), one byte per output element, shared by all seeds
//   VJP       dx[s, n, h, w, c] = sum over the windows that cover (h, w), in fixed (oh, ow) order, of
//             max: g[s, n, oh, ow, c] where the window's code names this pixel;  average: g[s, n, oh, ow, c] / div(window)
// Replaces, on the NHWC sweep, the stock pair of the NCHW sweep: max_pool2d(return_indices=True) and a scatter_add_ through
// int64 indices expanded over the seeds (8 index bytes per 4 data bytes, atomics).
//
// Both kernels are streaming: lanes along the channels, one lane per output element (forward) / per input pixel (VJP, the
// GATHER form: every dx element has one owner, plain stores, no atomics on data, repeated runs give the same bits).  16-byte
// loads of x / g and 4-byte loads of arg where C % 4 == 0 and the pointers are aligned, 4- and 1-byte loads otherwise.  The VJP
// lane reads the codes of its pixel's windows ONCE, keeps one match bit per window and channel (a pixel lies in at most
// ceil(kh / sh) * ceil(kw / sw) <= 64 windows) and then loops over the seeds, POOL_SC of them in flight per pass.  SELECTION
// (kh <= sh and kw <= sw: no two windows share a pixel) is a copy or a zero; SUMMING walks the covering windows and skips the
// loads of a window none of the lane's channels won.  Few pixels: the seeds are split over grid.y.  `amax` receives max|dx| as
// the bit pattern of a non-negative float through atomicMax, which is order-independent (wave_amax of lk_stream.h).
// Minimal traffic of the VJP: 4 S B C (OH OW + H W) + B C OH OW bytes.
#include "lk_stream.h"

namespace lk {

constexpr int POOL_SC = 4;  // seeds per pass of the VJP (their g loads are in flight together)

struct PoolGeom {
  int H, W, C, OH, OW, CV;  // CV: channel vectors per pixel
  int kh, kw, sh, sw, ph, pw;
  int cip, divisor;  // average: count_include_pad, divisor_override (<= 0: none)
  int big;           // the lane index does not fit 31 bits: 64-bit divisions
  FastDiv cv_div, w_div, h_div;  // by CV, by the width and the height of the map the lanes run over
};

// the codes of VEC adjacent channels, one per byte
template <int VEC>
__device__ __forceinline__ unsigned pool_ld_codes(const uint8_t* __restrict__ p) {
  if constexpr (VEC == 4) return *reinterpret_cast<const unsigned*>(p);
  else return *p;
}

// the divisor of the average over the window at (h0, w0)
__device__ __forceinline__ float pool_div(const PoolGeom& q, int h0, int w0) {
  if (q.divisor > 0) return (float)q.divisor;
  if (q.cip) return (float)(q.kh * q.kw);
  return (float)((min(h0 + q.kh, q.H) - max(h0, 0)) * (min(w0 + q.kw, q.W) - max(w0, 0)));
}

// ---- forward: a lane per output element (x VEC channels) ----------------------------------------------------------------------
template <int VEC, int KIND>
__global__ __launch_bounds__(256) void pool_fwd_kernel(const float* __restrict__ x, PoolGeom q, int64_t total,
                                                       float* __restrict__ y, uint8_t* __restrict__ arg) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    int cv, ow, oh;
    int64_t n;
    map_where(q, t, q.OH, q.OW, cv, ow, oh, n);
    const int h0 = oh * q.sh - q.ph, w0 = ow * q.sw - q.pw;
    const int dy_lo = max(0, -h0), dy_hi = min(q.kh, q.H - h0), dx_lo = max(0, -w0), dx_hi = min(q.kw, q.W - w0);
    const float* xn = x + n * q.H * q.W * q.C + cv * VEC;
    float acc[VEC];
    unsigned code[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      acc[e] = KIND == LK_POOL_MAX ? -INFINITY : 0.f;
      code[e] = (unsigned)(dy_lo * q.kw + dx_lo);  // (the first in-image tap: what a window of -inf reports)
    }
    for (int dy = dy_lo; dy < dy_hi; ++dy)
      for (int dx = dx_lo; dx < dx_hi; ++dx) {
        float v[VEC];
        ld<VEC>(xn + ((int64_t)(h0 + dy) * q.W + (w0 + dx)) * q.C, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          if constexpr (KIND == LK_POOL_MAX) {
            if (v[e] > acc[e] || v[e] != v[e]) {  // (strict >: the first maximum stays; a NaN wins, as in torch)
              acc[e] = v[e];
              code[e] = (unsigned)(dy * q.kw + dx);
            }
          } else {
            acc[e] += v[e];
          }
        }
      }
    const int64_t o = ((n * q.OH + oh) * q.OW + ow) * q.C + cv * VEC;
    if constexpr (KIND == LK_POOL_AVG) {
      const float d = pool_div(q, h0, w0);
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] = acc[e] / d;
    } else if constexpr (VEC == 4) {
      *reinterpret_cast<unsigned*>(arg + o) = code[0] | code[1] << 8 | code[2] << 16 | code[3] << 24;
    } else {
      arg[o] = (uint8_t)code[0];
    }
    st<VEC>(y + o, acc);
  }
}

// ---- VJP: a lane per input pixel (x VEC channels), all seeds of its grid.y slice ---------------------------------------------
template <int VEC, int KIND, bool SELECT>
__global__ __launch_bounds__(256) void pool_vjp_kernel(const float* __restrict__ g, const uint8_t* __restrict__ arg,
                                                       PoolGeom q, int S, int s_per, int64_t total, int64_t g_seed,
                                                       int64_t dx_seed, float* __restrict__ dx,
                                                       unsigned* __restrict__ amax) {
  const int s_begin = blockIdx.y * s_per;
  const int s_end = min(S, s_begin + s_per);
  float vmax = 0.f;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    int cv, w, h;
    int64_t n;
    map_where(q, t, q.H, q.W, cv, w, h, n);
    // the windows that cover (h, w): oh * sh - ph <= h < oh * sh - ph + kh
    const int nh = h + q.ph - q.kh + 1, nw = w + q.pw - q.kw + 1;
    // (SELECT: at most one per axis, so the loops below end after their first turn)
    const int oh_lo = nh <= 0 ? 0 : (nh + q.sh - 1) / q.sh, oh_hi = min(q.OH - 1, (h + q.ph) / q.sh);
    const int ow_lo = nw <= 0 ? 0 : (nw + q.sw - 1) / q.sw, ow_hi = min(q.OW - 1, (w + q.pw) / q.sw);
    const int64_t g0 = n * q.OH * q.OW * q.C + cv * VEC;  // this lane's channels at window (0, 0)
    float* dp = dx + ((n * q.H + h) * q.W + w) * q.C + cv * VEC;
    uint64_t won[VEC];  // bit j: window j (in the order of the loops below) names this pixel for channel e
#pragma unroll
    for (int e = 0; e < VEC; ++e) won[e] = 0;
    if constexpr (KIND == LK_POOL_MAX) {
      int j = 0;
      for (int oh = oh_lo; oh <= oh_hi; ++oh) {
        for (int ow = ow_lo; ow <= ow_hi; ++ow, ++j) {
          const unsigned want = (unsigned)((h - (oh * q.sh - q.ph)) * q.kw + (w - (ow * q.sw - q.pw)));
          const unsigned codes = pool_ld_codes<VEC>(arg + g0 + ((int64_t)oh * q.OW + ow) * q.C);
#pragma unroll
          for (int e = 0; e < VEC; ++e) won[e] |= (uint64_t)(((codes >> (8 * e)) & 255u) == want) << j;
          if constexpr (SELECT) break;
        }
        if constexpr (SELECT) break;
      }
    }
    uint64_t any = 0;
#pragma unroll
    for (int e = 0; e < VEC; ++e) any |= won[e];
    for (int s0 = s_begin; s0 < s_end; s0 += POOL_SC) {
      float acc[POOL_SC][VEC];
#pragma unroll
      for (int k = 0; k < POOL_SC; ++k)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[k][e] = 0.f;
      int j = 0;
      for (int oh = oh_lo; oh <= oh_hi; ++oh) {
        for (int ow = ow_lo; ow <= ow_hi; ++ow, ++j) {
          if (KIND == LK_POOL_AVG || ((any >> j) & 1)) {  // (max: skip a window none of this lane's channels won)
            const float* gp = g + g0 + ((int64_t)oh * q.OW + ow) * q.C;
            float d = 1.f;
            if constexpr (KIND == LK_POOL_AVG) d = pool_div(q, oh * q.sh - q.ph, ow * q.sw - q.pw);
            float gv[POOL_SC][VEC];
#pragma unroll
            for (int k = 0; k < POOL_SC; ++k)
              if (s0 + k < s_end) ld<VEC>(gp + (int64_t)(s0 + k) * g_seed, gv[k]);
#pragma unroll
            for (int k = 0; k < POOL_SC; ++k)
              if (s0 + k < s_end) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                  if constexpr (KIND == LK_POOL_MAX) acc[k][e] += ((won[e] >> j) & 1) ? gv[k][e] : 0.f;
                  else acc[k][e] += gv[k][e] / d;
                }
              }
          }
          if constexpr (SELECT) break;
        }
        if constexpr (SELECT) break;
      }
#pragma unroll
      for (int k = 0; k < POOL_SC; ++k)
        if (s0 + k < s_end) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) vmax = fmaxf(vmax, fabsf(acc[k][e]));
          st<VEC>(dp + (int64_t)(s0 + k) * dx_seed, acc[k]);
        }
    }
  }
  wave_amax(vmax, amax);
}

// ---- host: the contract and the path of a shape ----------------------------------------------------------------------------------
struct PoolPlan {
  int vec;      // 16-byte loads
  int summing;  // two windows may share a pixel
  int s_per;    // seeds per grid.y slice
  int64_t OH, OW, lanes, blocks;
};

// the part of the contract every entry point shares, with the messages under the caller's name; `lanes_over_input`: the launch
// runs a lane per input pixel (the VJP) or per output element (the forward)
static int pool_check_shape(const char* fn, int kind, int64_t S, int64_t B, int64_t H, int64_t W, int64_t C, int kh, int kw,
                            int sh, int sw, int ph, int pw, bool aligned, bool lanes_over_input, PoolPlan* p) {
  LK_REQUIRE(kind == LK_POOL_MAX || kind == LK_POOL_AVG, "%s: kind must be LK_POOL_MAX (0) or LK_POOL_AVG (1)", fn);
  LK_REQUIRE(kh >= 1 && kh <= 8 && kw >= 1 && kw <= 8, "%s: window out of range (1 <= kh, kw <= 8)", fn);
  LK_REQUIRE(sh >= 1 && sh < 32768 && sw >= 1 && sw < 32768, "%s: stride out of range (1 <= sh, sw < 32768)", fn);
  LK_REQUIRE(ph >= 0 && ph <= kh / 2 && pw >= 0 && pw <= kw / 2,
             "%s: padding out of range (0 <= ph <= kh / 2, 0 <= pw <= kw / 2)", fn);
  LK_REQUIRE(S >= 1 && S < (1ll << 31) && B >= 0 && B < (1ll << 31) && S * B < (1ll << 31) && H >= 1 && H < 32768 && W >= 1 &&
                 W < 32768 && C >= 1 && C < (1ll << 30),
             "%s: extent out of range (1 <= S, 0 <= B, S * B < 2^31, 1 <= H, W < 32768, 1 <= C < 2^30)", fn);
  LK_REQUIRE(H + 2 * ph >= kh && W + 2 * pw >= kw, "%s: empty output (OH, OW >= 1)", fn);
  p->OH = (H + 2 * ph - kh) / sh + 1;
  p->OW = (W + 2 * pw - kw) / sw + 1;
  const int64_t in_px = H * W, out_px = p->OH * p->OW;
  const unsigned __int128 count = (unsigned __int128)(S * B) * C * (in_px > out_px ? in_px : out_px);
  LK_REQUIRE(count < ((unsigned __int128)1 << 40), "%s: too many elements (S * B * C * max(H * W, OH * OW) < 2^40)", fn);
  p->vec = aligned && C % 4 == 0;
  p->summing = !(kh <= sh && kw <= sw);
  p->lanes = B * (lanes_over_input ? in_px : out_px) * (p->vec ? C / 4 : C);
  // (the kernels stride over the lanes; a launch takes fewer than 2^32 threads in x)
  const int64_t need = (p->lanes + 255) / 256, cap = ((1ll << 32) - 1) / 256;
  p->blocks = need < cap ? need : cap;
  p->s_per = seeds_per_slice(S, (p->lanes + 63) / 64);
  return LK_OK;
}

static PoolGeom pool_geometry(const PoolPlan& p, int64_t H, int64_t W, int64_t C, int kh, int kw, int sh, int sw, int ph,
                              int pw, int cip, int divisor, bool lanes_over_input) {
  PoolGeom q;
  q.H = (int)H, q.W = (int)W, q.C = (int)C, q.OH = (int)p.OH, q.OW = (int)p.OW, q.CV = (int)(p.vec ? C / 4 : C);
  q.kh = kh, q.kw = kw, q.sh = sh, q.sw = sw, q.ph = ph, q.pw = pw;
  q.cip = cip != 0, q.divisor = divisor;
  q.big = p.lanes >= (1ll << 31);
  q.cv_div = make_fastdiv(q.CV);
  q.w_div = make_fastdiv(lanes_over_input ? q.W : q.OW);
  q.h_div = make_fastdiv(lanes_over_input ? q.H : q.OH);
  return q;
}

static int pool_check_fwd(int kind, const float* x, int64_t B, int64_t H, int64_t W, int64_t C, int kh, int kw, int sh, int sw,
                          int ph, int pw, const float* y, const uint8_t* arg, PoolPlan* p) {
  LK_REQUIRE(x && y, "lk_pool_fwd_nhwc_f32: null pointer");
  const bool aligned = (((uintptr_t)x | (uintptr_t)y) & 15) == 0 && ((uintptr_t)arg & 3) == 0;
  const int rc = pool_check_shape("lk_pool_fwd_nhwc_f32", kind, 1, B, H, W, C, kh, kw, sh, sw, ph, pw, aligned, false, p);
  if (rc != LK_OK) return rc;
  LK_REQUIRE((arg != nullptr) == (kind == LK_POOL_MAX),
             "lk_pool_fwd_nhwc_f32: arg must be given for LK_POOL_MAX and null for LK_POOL_AVG");
  return LK_OK;
}

static int pool_check_vjp(int kind, const float* g, const uint8_t* arg, int64_t S, int64_t B, int64_t H, int64_t W, int64_t C,
                          int kh, int kw, int sh, int sw, int ph, int pw, const float* dx, PoolPlan* p) {
  LK_REQUIRE(g && dx, "lk_pool_vjp_nhwc_f32: null pointer");
  const bool aligned = (((uintptr_t)g | (uintptr_t)dx) & 15) == 0 && ((uintptr_t)arg & 3) == 0;
  const int rc = pool_check_shape("lk_pool_vjp_nhwc_f32", kind, S, B, H, W, C, kh, kw, sh, sw, ph, pw, aligned, true, p);
  if (rc != LK_OK) return rc;
  LK_REQUIRE((arg != nullptr) == (kind == LK_POOL_MAX),
             "lk_pool_vjp_nhwc_f32: arg must be given for LK_POOL_MAX and null for LK_POOL_AVG");
  const unsigned __int128 gb = (unsigned __int128)(S * B) * p->OH * p->OW * C * 4, db = (unsigned __int128)(S * B) * H * W * C * 4;
  const unsigned __int128 g0 = (uintptr_t)g, d0 = (uintptr_t)dx;
  LK_REQUIRE(g0 + gb <= d0 || d0 + db <= g0, "lk_pool_vjp_nhwc_f32: dx overlaps g");
  return LK_OK;
}

}  // namespace lk

using namespace lk;

extern "C" int lk_pool_fwd_nhwc_f32(int kind, const float* x, int64_t B, int64_t H, int64_t W, int64_t C, int kh, int kw,
                                    int sh, int sw, int ph, int pw, int count_include_pad, int divisor_override, float* y,
                                    uint8_t* arg, void* stream) {
  PoolPlan p;
  const int rc = pool_check_fwd(kind, x, B, H, W, C, kh, kw, sh, sw, ph, pw, y, arg, &p);
  if (rc != LK_OK) return rc;
  if (B == 0) return LK_OK;
  const PoolGeom q = pool_geometry(p, H, W, C, kh, kw, sh, sw, ph, pw, count_include_pad, divisor_override, false);
  hipStream_t st = (hipStream_t)stream;
#define LK_POOL_FWD(V, K) \
  hipLaunchKernelGGL((pool_fwd_kernel<V, K>), dim3((unsigned)p.blocks), dim3(256), 0, st, x, q, p.lanes, y, arg)
  if (kind == LK_POOL_MAX) {
    if (p.vec) LK_POOL_FWD(4, LK_POOL_MAX);
    else LK_POOL_FWD(1, LK_POOL_MAX);
  } else {
    if (p.vec) LK_POOL_FWD(4, LK_POOL_AVG);
    else LK_POOL_FWD(1, LK_POOL_AVG);
  }
#undef LK_POOL_FWD
  return check_launch("pool_fwd_kernel");
}

extern "C" int lk_pool_vjp_nhwc_f32(int kind, const float* g, const uint8_t* arg, int64_t S, int64_t B, int64_t H, int64_t W,
                                    int64_t C, int kh, int kw, int sh, int sw, int ph, int pw, int count_include_pad,
                                    int divisor_override, float* dx, unsigned* amax, void* stream) {
  PoolPlan p;
  const int rc = pool_check_vjp(kind, g, arg, S, B, H, W, C, kh, kw, sh, sw, ph, pw, dx, &p);
  if (rc != LK_OK) return rc;
  if (B == 0) return LK_OK;
  const PoolGeom q = pool_geometry(p, H, W, C, kh, kw, sh, sw, ph, pw, count_include_pad, divisor_override, true);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)p.blocks, (unsigned)((S + p.s_per - 1) / p.s_per));
  const int64_t g_seed = B * p.OH * p.OW * C, dx_seed = B * H * W * C;
#define LK_POOL_VJP(V, K, SEL)                                                                                              \
  hipLaunchKernelGGL((pool_vjp_kernel<V, K, SEL>), grid, dim3(256), 0, st, g, arg, q, (int)S, p.s_per, p.lanes, g_seed, dx_seed, \
                     dx, amax)
#define LK_POOL_VJP_K(K)                               \
  do {                                                 \
    if (p.vec && !p.summing) LK_POOL_VJP(4, K, true);  \
    else if (p.vec) LK_POOL_VJP(4, K, false);          \
    else if (!p.summing) LK_POOL_VJP(1, K, true);      \
    else LK_POOL_VJP(1, K, false);                     \
  } while (0)
  if (kind == LK_POOL_MAX) LK_POOL_VJP_K(LK_POOL_MAX);
  else LK_POOL_VJP_K(LK_POOL_AVG);
#undef LK_POOL_VJP_K
#undef LK_POOL_VJP
  return check_launch("pool_vjp_kernel");
}

// vec | summing << 1 | seed-split << 2 | seeds per pass << 4 | seeds per grid.y slice (capped at 65535) << 12
extern "C" int lk_pool_variant(int kind, int64_t S, int64_t B, int64_t H, int64_t W, int64_t C, int kh, int kw, int sh, int sw,
                               int ph, int pw, int aligned) {
  PoolPlan p;
  if (pool_check_shape("lk_pool_variant", kind, S, B, H, W, C, kh, kw, sh, sw, ph, pw, aligned != 0, true, &p) != LK_OK) return -1;
  const int slice = p.s_per > 65535 ? 65535 : p.s_per;
  return p.vec | p.summing << 1 | (p.s_per < S ? 1 : 0) << 2 | POOL_SC << 4 | slice << 12;
}
