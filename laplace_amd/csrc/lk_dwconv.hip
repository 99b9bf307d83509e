// Depthwise convolution (nn.Conv2d with groups == in_channels == out_channels, no dilation, zero padding) on NHWC feature maps
// for the seed-batched reverse sweep:
//   forward        y[n, oh, ow, c]     = bias[c] + sum over the in-image taps, in fixed (dy, dx) order, of
//                                        w_tap[dy kw + dx][c] * x[n, oh sh - ph + dy, ow sw - pw + dx, c]
//   backward-data  dx[s, n, h, w, c]   = sum over (dy, dx) in the same order with (h + ph - dy) % sh == 0, (w + pw - dx) % sw == 0
//                                        and oh = (h + ph - dy) / sh in [0, OH), ow likewise, of w_tap[dy kw + dx][c] * g[s, n, oh, ow, c]
// with g the cotangent as the two fp16 planes of a ONE-scale split tensor, g = (float(h) + float(l)) * 2^-sexp[0].
// Replaces, on the NHWC sweep, the library pair of the NCHW sweep - the module's own forward and convolution_backward with
// `groups` - which is the reverse pass through a depthwise layer of laplace/curvature/curvlinops.py:87-100 and
// curvature.py:88-129.
//
// A depthwise convolution has one input channel per output channel: no GEMM, a streaming kernel of the family of lk_pool.hip.
// Lanes run along the channels.  Forward: a lane per output element (x 4 channels), weights through L1.  Backward-data, the
// GATHER form: a lane owns a dx pixel (x 4 channels), loads its kh kw x 4 weights ONCE into registers and loops over the seeds of
// its grid.y slice, DW_SC of them in flight per pass; every dx element has one owner, stores are plain, repeated runs give the
// same bits; a pixel no window reaches stores 0.  The tap loops are unrolled over the tap-count class (<= 9, <= 25) so that the
// weights are indexed statically; the tap's (dy, dx), dy / sh and dy % sh are wave-uniform counters, and the lane's own
// (h + ph) / sh and % sh are taken once per pixel, so no tap costs a division.  8-byte loads of the planes and 16-byte loads /
// stores of w_tap and dx where C % 4 == 0 and the pointers are aligned, else one channel per lane.  `amax` receives max|dx| as
// the bit pattern of a non-negative float through atomicMax, one atomic per wave (wave_amax of lk_stream.h).
// Minimal traffic of the backward: 4 S B C (OH OW + H W) + 4 kh kw C bytes.
#include "lk_stream.h"

namespace lk {

constexpr int DW_SC = 4;  // seeds per pass of the backward (their plane loads are in flight together)

struct DwGeom {
  int H, W, C, OH, OW, CV;  // CV: channel vectors per pixel
  int kh, kw, sh, sw, ph, pw, T;  // T = kh * kw
  int big;  // the lane index does not fit 31 bits: 64-bit divisions
  FastDiv cv_div, w_div, h_div;  // by CV, by the width and the height of the map the lanes run over
  FastDiv sh_div, sw_div;
};

// ---- forward: a lane per output element (x VEC channels) ----------------------------------------------------------------------
template <int VEC, int TC>
__global__ __launch_bounds__(256) void dwconv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w_tap,
                                                         const float* __restrict__ bias, DwGeom q, int64_t total,
                                                         float* __restrict__ y) {
  constexpr int TMAX = TC ? 25 : 9;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    int cv, ow, oh;
    int64_t n;
    map_where(q, t, q.OH, q.OW, cv, ow, oh, n);
    const int h0 = oh * q.sh - q.ph, w0 = ow * q.sw - q.pw;
    const float* xn = x + n * q.H * q.W * q.C + cv * VEC;
    const float* wp = w_tap + cv * VEC;
    float acc[VEC];
    if (bias != nullptr) {
      ld<VEC>(bias + cv * VEC, acc);
    } else {
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    }
    int dy = 0, dx = 0;  // (wave-uniform: the tap of this turn)
#pragma unroll
    for (int tt = 0; tt < TMAX; ++tt) {
      if (tt < q.T) {
        const int ih = h0 + dy, iw = w0 + dx;
        if ((unsigned)ih < (unsigned)q.H && (unsigned)iw < (unsigned)q.W) {
          float xv[VEC], wv[VEC];
          ld<VEC>(xn + ((int64_t)ih * q.W + iw) * q.C, xv);
          ld<VEC>(wp + (int64_t)tt * q.C, wv);
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc[e] += wv[e] * xv[e];
        }
        if (++dx == q.kw) dx = 0, ++dy;
      }
    }
    st<VEC>(y + ((n * q.OH + oh) * q.OW + ow) * q.C + cv * VEC, acc);
  }
}

// ---- backward-data: a lane per input pixel (x VEC channels), all seeds of its grid.y slice ---------------------------------------
template <int VEC, int TC, bool STRIDED>
__global__ __launch_bounds__(256) void dwconv_bwd_kernel(const _Float16* __restrict__ gh, const _Float16* __restrict__ gl,
                                                         const int* __restrict__ sexp, const float* __restrict__ w_tap,
                                                         DwGeom q, int S, int s_per, int64_t total, int64_t g_seed,
                                                         int64_t dx_seed, float* __restrict__ dx,
                                                         unsigned* __restrict__ amax) {
  constexpr int TMAX = TC ? 25 : 9;
  const float scale = ldexpf(1.f, -sexp[0]);
  const int s_begin = blockIdx.y * s_per;
  const int s_end = min(S, s_begin + s_per);
  float vmax = 0.f;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    int cv, w, h;
    int64_t n;
    map_where(q, t, q.H, q.W, cv, w, h, n);
    // h + ph = qh sh + rh: tap row dy reaches this pixel from output row qh - dy / sh when dy % sh == rh (columns likewise)
    int qh = h + q.ph, rh = 0, qw = w + q.pw, rw = 0;
    if constexpr (STRIDED) {
      const int a = qh, b = qw;
      qh = fdiv(a, q.sh_div), rh = a - qh * q.sh;
      qw = fdiv(b, q.sw_div), rw = b - qw * q.sw;
    }
    float wr[TMAX][VEC];
#pragma unroll
    for (int tt = 0; tt < TMAX; ++tt) {
      if (tt < q.T) {
        ld<VEC>(w_tap + (int64_t)tt * q.C + cv * VEC, wr[tt]);
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) wr[tt][e] = 0.f;
      }
    }
    const int64_t g0 = n * q.OH * q.OW * q.C + cv * VEC;  // this lane's channels at output pixel (0, 0)
    float* dp = dx + ((n * q.H + h) * q.W + w) * q.C + cv * VEC;
    for (int s0 = s_begin; s0 < s_end; s0 += DW_SC) {
      float acc[DW_SC][VEC];
#pragma unroll
      for (int k = 0; k < DW_SC; ++k)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[k][e] = 0.f;
      // wave-uniform counters of the tap of this turn: column dxx, and dy / sh, dy % sh, dxx / sw, dxx % sw
      int dxx = 0, dyq = 0, dym = 0, dxq = 0, dxm = 0;
#pragma unroll
      for (int tt = 0; tt < TMAX; ++tt) {
        if (tt < q.T) {
          const int oh = qh - dyq, ow = qw - dxq;
          bool ok = (unsigned)oh < (unsigned)q.OH && (unsigned)ow < (unsigned)q.OW;
          if constexpr (STRIDED) ok = ok && rh == dym && rw == dxm;
          if (ok) {
            const int64_t o = g0 + ((int64_t)oh * q.OW + ow) * q.C;
            float gv[DW_SC][VEC];
#pragma unroll
            for (int k = 0; k < DW_SC; ++k)
              if (s0 + k < s_end) ld_split<VEC>(gh + o + (int64_t)(s0 + k) * g_seed, gl + o + (int64_t)(s0 + k) * g_seed, gv[k]);
#pragma unroll
            for (int k = 0; k < DW_SC; ++k)
              if (s0 + k < s_end) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[k][e] += wr[tt][e] * gv[k][e];
              }
          }
          if (++dxm == q.sw) dxm = 0, ++dxq;
          if (++dxx == q.kw) {
            dxx = dxq = dxm = 0;
            if (++dym == q.sh) dym = 0, ++dyq;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < DW_SC; ++k)
        if (s0 + k < s_end) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            acc[k][e] *= scale;
            vmax = fmaxf(vmax, fabsf(acc[k][e]));
          }
          st<VEC>(dp + (int64_t)(s0 + k) * dx_seed, acc[k]);
        }
    }
  }
  wave_amax(vmax, amax);
}

// ---- host: the contract and the path of a shape ----------------------------------------------------------------------------------
struct DwPlan {
  int vec;    // 16-byte loads of w_tap / x / dx, 8-byte loads of the planes
  int tc;     // tap class: 0 for <= 9 taps, 1 for <= 25
  int s_per;  // seeds per grid.y slice
  int64_t OH, OW, lanes, blocks;
};

// the part of the contract every entry point shares, with the messages under the caller's name; `lanes_over_input`: the launch
// runs a lane per input pixel (the backward) or per output element (the forward)
static int dwconv_check_shape(const char* fn, int64_t S, int64_t B, int64_t H, int64_t W, int64_t C, int kh, int kw, int sh,
                              int sw, int ph, int pw, bool aligned, bool lanes_over_input, DwPlan* p) {
  LK_REQUIRE(kh >= 1 && kw >= 1 && (int64_t)kh * kw <= 25, "%s: window out of range (1 <= kh, kw and kh * kw <= 25)", fn);
  LK_REQUIRE(sh >= 1 && sh <= 8 && sw >= 1 && sw <= 8, "%s: stride out of range (1 <= sh, sw <= 8)", fn);
  LK_REQUIRE(ph >= 0 && ph < kh && pw >= 0 && pw < kw, "%s: padding out of range (0 <= ph < kh, 0 <= pw < kw)", fn);
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
  p->tc = kh * kw > 9;
  p->lanes = B * (lanes_over_input ? in_px : out_px) * (p->vec ? C / 4 : C);
  // (the kernels stride over the lanes; a launch takes fewer than 2^32 threads in x)
  const int64_t need = (p->lanes + 255) / 256, cap = ((1ll << 32) - 1) / 256;
  p->blocks = need < cap ? need : cap;
  p->s_per = seeds_per_slice(S, (p->lanes + 63) / 64);
  return LK_OK;
}

static DwGeom dwconv_geometry(const DwPlan& p, int64_t H, int64_t W, int64_t C, int kh, int kw, int sh, int sw, int ph, int pw,
                              bool lanes_over_input) {
  DwGeom q;
  q.H = (int)H, q.W = (int)W, q.C = (int)C, q.OH = (int)p.OH, q.OW = (int)p.OW, q.CV = (int)(p.vec ? C / 4 : C);
  q.kh = kh, q.kw = kw, q.sh = sh, q.sw = sw, q.ph = ph, q.pw = pw, q.T = kh * kw;
  q.big = p.lanes >= (1ll << 31);
  q.cv_div = make_fastdiv(q.CV);
  q.w_div = make_fastdiv(lanes_over_input ? q.W : q.OW);
  q.h_div = make_fastdiv(lanes_over_input ? q.H : q.OH);
  q.sh_div = make_fastdiv(sh);
  q.sw_div = make_fastdiv(sw);
  return q;
}

static int dwconv_check_fwd(const float* x, const float* w_tap, const float* bias, int64_t B, int64_t H, int64_t W, int64_t C,
                            int kh, int kw, int sh, int sw, int ph, int pw, const float* y, DwPlan* p) {
  LK_REQUIRE(x && w_tap && y, "lk_dwconv_fwd_nhwc_f32: null pointer");
  const bool aligned = (((uintptr_t)x | (uintptr_t)w_tap | (uintptr_t)bias | (uintptr_t)y) & 15) == 0;
  return dwconv_check_shape("lk_dwconv_fwd_nhwc_f32", 1, B, H, W, C, kh, kw, sh, sw, ph, pw, aligned, false, p);
}

static int dwconv_check_bwd(const void* g_h, const void* g_l, const int* sexp, const float* w_tap, int64_t S, int64_t B,
                            int64_t H, int64_t W, int64_t C, int kh, int kw, int sh, int sw, int ph, int pw, const float* dx,
                            DwPlan* p) {
  LK_REQUIRE(g_h && g_l && sexp && w_tap && dx, "lk_dwconv_bwd_nhwc_f16x2: null pointer");
  const bool aligned = (((uintptr_t)g_h | (uintptr_t)g_l) & 7) == 0 && (((uintptr_t)w_tap | (uintptr_t)dx) & 15) == 0;
  const int rc = dwconv_check_shape("lk_dwconv_bwd_nhwc_f16x2", S, B, H, W, C, kh, kw, sh, sw, ph, pw, aligned, true, p);
  if (rc != LK_OK) return rc;
  const unsigned __int128 gb = (unsigned __int128)(S * B) * p->OH * p->OW * C * 2, db = (unsigned __int128)(S * B) * H * W * C * 4;
  const unsigned __int128 d0 = (uintptr_t)dx;
  for (const void* plane : {g_h, g_l}) {
    const unsigned __int128 g0 = (uintptr_t)plane;
    LK_REQUIRE(g0 + gb <= d0 || d0 + db <= g0, "lk_dwconv_bwd_nhwc_f16x2: dx overlaps g");
  }
  return LK_OK;
}

}  // namespace lk

using namespace lk;

extern "C" int lk_dwconv_fwd_nhwc_f32(const float* x, const float* w_tap, const float* bias, int64_t B, int64_t H, int64_t W,
                                      int64_t C, int kh, int kw, int sh, int sw, int ph, int pw, float* y, void* stream) {
  DwPlan p;
  const int rc = dwconv_check_fwd(x, w_tap, bias, B, H, W, C, kh, kw, sh, sw, ph, pw, y, &p);
  if (rc != LK_OK) return rc;
  if (B == 0) return LK_OK;
  const DwGeom q = dwconv_geometry(p, H, W, C, kh, kw, sh, sw, ph, pw, false);
  hipStream_t st = (hipStream_t)stream;
#define LK_DW_FWD(V, TC) \
  hipLaunchKernelGGL((dwconv_fwd_kernel<V, TC>), dim3((unsigned)p.blocks), dim3(256), 0, st, x, w_tap, bias, q, p.lanes, y)
  if (p.vec && p.tc) LK_DW_FWD(4, 1);
  else if (p.vec) LK_DW_FWD(4, 0);
  else if (p.tc) LK_DW_FWD(1, 1);
  else LK_DW_FWD(1, 0);
#undef LK_DW_FWD
  return check_launch("dwconv_fwd_kernel");
}

extern "C" int lk_dwconv_bwd_nhwc_f16x2(const void* g_h, const void* g_l, const int* sexp, const float* w_tap, int64_t S,
                                        int64_t B, int64_t H, int64_t W, int64_t C, int kh, int kw, int sh, int sw, int ph,
                                        int pw, float* dx, unsigned* amax, void* stream) {
  DwPlan p;
  const int rc = dwconv_check_bwd(g_h, g_l, sexp, w_tap, S, B, H, W, C, kh, kw, sh, sw, ph, pw, dx, &p);
  if (rc != LK_OK) return rc;
  if (B == 0) return LK_OK;
  const DwGeom q = dwconv_geometry(p, H, W, C, kh, kw, sh, sw, ph, pw, true);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)p.blocks, (unsigned)((S + p.s_per - 1) / p.s_per));
  const int64_t g_seed = B * p.OH * p.OW * C, dx_seed = B * H * W * C;
  const _Float16 *gh = (const _Float16*)g_h, *gl = (const _Float16*)g_l;
  const bool strided = sh > 1 || sw > 1;
#define LK_DW_BWD(V, TC, STR)                                                                                                   \
  hipLaunchKernelGGL((dwconv_bwd_kernel<V, TC, STR>), grid, dim3(256), 0, st, gh, gl, sexp, w_tap, q, (int)S, p.s_per, p.lanes, \
                     g_seed, dx_seed, dx, amax)
#define LK_DW_BWD_T(V, TC)           \
  do {                               \
    if (strided) LK_DW_BWD(V, TC, true); \
    else LK_DW_BWD(V, TC, false);    \
  } while (0)
  if (p.vec && p.tc) LK_DW_BWD_T(4, 1);
  else if (p.vec) LK_DW_BWD_T(4, 0);
  else if (p.tc) LK_DW_BWD_T(1, 1);
  else LK_DW_BWD_T(1, 0);
#undef LK_DW_BWD_T
#undef LK_DW_BWD
  return check_launch("dwconv_bwd_kernel");
}

// vec | strided << 1 | seed-split << 2 | tap class << 3 | seeds per pass << 4 | seeds per grid.y slice (capped at 65535) << 12
extern "C" int lk_dwconv_variant(int64_t S, int64_t B, int64_t H, int64_t W, int64_t C, int kh, int kw, int sh, int sw, int ph,
                                 int pw, int aligned) {
  DwPlan p;
  if (dwconv_check_shape("lk_dwconv_variant", S, B, H, W, C, kh, kw, sh, sw, ph, pw, aligned != 0, true, &p) != LK_OK) return -1;
  const int slice = p.s_per > 65535 ? 65535 : p.s_per;
  return p.vec | (sh > 1 || sw > 1 ? 1 : 0) << 1 | (p.s_per < S ? 1 : 0) << 2 | p.tc << 3 | DW_SC << 4 | slice << 12;
}
