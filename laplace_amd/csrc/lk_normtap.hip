// Per-sample Jacobian of an affine normalisation layer y = w * xhat + b with respect to w and b for all seeds of the NHWC
// split-fp16 reverse sweep, read where the sweep leaves the cotangent of the layer's output:
//   Js[n][s][wcol0 + ch] = sum_l g[s][n][l][ch] * xhat[n][l][ch]        Js[n][s][bcol0 + ch] = sum_l g[s][n][l][ch]
// with g [S][B][L][Ch] the two fp16 planes of a ONE-scale split tensor, g = (float(h) + float(l)) * 2^-sexp[0], x [B][L][Ch] fp32
// and xhat = (x - mu[ch]) * rstd[ch] formed in registers (x itself when mu and rstd are null): a tapped eval-mode BatchNorm2d
// needs neither an fp32 NCHW copy of its cotangent nor an activation-sized xhat tensor.  The NHWC counterpart of layout 1 of
// lk_jac_norm_affine_f32 (lk_norm.hip); replaces the same norm-parameter columns of CurvatureInterface.jacobians
// (laplace/curvature/curvature.py:88-129) and of GGNInterface.diag / EFInterface.diag (curvature.py:413-433, 494-505).
//
// A streaming reduction over L.  Lanes run along the channels: a workgroup of 256 lanes owns CXW channel vectors (a power of
// two) of one sample, its 256 / CXW lane rows stride over the positions.  A lane keeps its xhat values in registers across the
// seeds of a pass, whose plane loads are in flight together, so x is read once per pass and not once per seed; fp32
// accumulators, the exact power-of-two scale once at the store.  ALL seeds of a pass are reduced together: the lane rows of a
// wave meet in an xor-shuffle tree, the four waves in a fixed tree through LDS - two barriers per pass, not per seed.  Every Js
// element has one owner and a plain store, no atomics: repeated runs give the same bits.  Few (sample, channel tile) pairs:
// the SEEDS are split over grid.y (every slice re-reads x); L is never split.
// Minimal traffic: 4 S B L Ch (planes) + 4 B L Ch (x) + 8 B S Ch (out) bytes.
#include "lk_stream.h"

namespace lk {

// seeds per pass: 2 * VEC * NT_SC accumulators per lane (64 for the wide forms)
template <int VEC>
struct NtSc {
  static constexpr int value = VEC == 8 ? 4 : 8;
};
// widest channel tile of a workgroup, in channel vectors (the LDS tree holds 3 waves x CXW x 2 VEC NT_SC floats: 24 KiB)
template <int VEC>
struct NtCap {
  static constexpr int value = VEC == 1 ? 64 : 32;
};

template <int VEC>
struct NtPlanes;  // the raw halves of VEC adjacent channels of both planes (one load each)
template <>
struct NtPlanes<8> {
  f16x8 h, l;
};
template <>
struct NtPlanes<4> {
  f16x4 h, l;
};
template <>
struct NtPlanes<1> {
  _Float16 h, l;
};

template <int VEC>
__device__ __forceinline__ void nt_ld_planes(const _Float16* __restrict__ h, const _Float16* __restrict__ l, NtPlanes<VEC>& r) {
  if constexpr (VEC == 8) {
    r.h = *reinterpret_cast<const f16x8*>(h), r.l = *reinterpret_cast<const f16x8*>(l);
  } else if constexpr (VEC == 4) {
    r.h = *reinterpret_cast<const f16x4*>(h), r.l = *reinterpret_cast<const f16x4*>(l);
  } else {
    r.h = *h, r.l = *l;
  }
}

template <int VEC>
__device__ __forceinline__ float nt_value(const NtPlanes<VEC>& r, int e) {
  if constexpr (VEC == 1) return (float)r.h + (float)r.l;
  else return (float)r.h[e] + (float)r.l[e];
}

// g planes [S][B][L][Ch], x [B][L][Ch]; blockIdx.x = (sample, channel tile), blockIdx.y = seed slice
template <int VEC>
__global__ __launch_bounds__(256) void jac_normtap_kernel(const _Float16* __restrict__ gh, const _Float16* __restrict__ gl,
                                                          const int* __restrict__ sexp, const float* __restrict__ x,
                                                          const float* __restrict__ mu, const float* __restrict__ rstd, int S,
                                                          int B, int L, int Ch, int CXW, int tiles, int s_per,
                                                          float* __restrict__ Js, int64_t P, int64_t wcol0, int64_t bcol0) {
  constexpr int SC = NtSc<VEC>::value, NA = 2 * VEC * SC, CAP = NtCap<VEC>::value;
  __shared__ float red[3 * NA * CAP];  // [wave - 1][accumulator][channel lane]
  const int CV = Ch / VEC;
  const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
  const int tx = threadIdx.x & (CXW - 1), ty = threadIdx.x / CXW, TL = 256 / CXW;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cv = tile * CXW + tx;
  const bool live = cv < CV;  // (dead lanes stay in the shuffles and the barriers and touch no global memory)
  const int s_begin = blockIdx.y * s_per;
  const int s_end = min(S, s_begin + s_per);
  const float scale = ldexpf(1.f, -sexp[0]);
  const int64_t c0 = (int64_t)cv * VEC;
  float m[VEC], r[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) m[e] = 0.f, r[e] = 1.f;  // (x - 0) * 1 is x, bit for bit
  if (live && mu != nullptr) ld<VEC>(mu + c0, m), ld<VEC>(rstd + c0, r);
  const float* xn = x + (int64_t)n * L * Ch + c0;
  const int64_t seed_stride = (int64_t)B * L * Ch;
  const int64_t gn = (int64_t)n * L * Ch + c0;
  for (int s0 = s_begin; s0 < s_end; s0 += SC) {
    float aw[SC][VEC], ab[SC][VEC];
#pragma unroll
    for (int k = 0; k < SC; ++k)
#pragma unroll
      for (int e = 0; e < VEC; ++e) aw[k][e] = ab[k][e] = 0.f;
    if (live) {
      for (int l = ty; l < L; l += TL) {
        const int64_t o = gn + (int64_t)l * Ch;
        NtPlanes<VEC> pv[SC];
#pragma unroll
        for (int k = 0; k < SC; ++k)
          if (s0 + k < s_end) nt_ld_planes<VEC>(gh + o + (s0 + k) * seed_stride, gl + o + (s0 + k) * seed_stride, pv[k]);  // (uniform)
        float xh[VEC];
        ld<VEC>(xn + (int64_t)l * Ch, xh);
#pragma unroll
        for (int e = 0; e < VEC; ++e) xh[e] = (xh[e] - m[e]) * r[e];
#pragma unroll
        for (int k = 0; k < SC; ++k)
          if (s0 + k < s_end) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              const float v = nt_value<VEC>(pv[k], e);
              aw[k][e] += v * xh[e];
              ab[k][e] += v;
            }
          }
      }
    }
    // the lane rows of a wave: xor-shuffle tree over the lane bits above the channel lanes (fixed order)
    for (int off = 32; off >= CXW; off >>= 1) {
#pragma unroll
      for (int k = 0; k < SC; ++k)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          aw[k][e] += __shfl_xor(aw[k][e], off, 64);
          ab[k][e] += __shfl_xor(ab[k][e], off, 64);
        }
    }
    // the four waves: (w0 + w2) + (w1 + w3) through LDS; with CXW == 64 a wave is one lane row
    const bool head = lane < CXW;  // (the lanes that hold their wave's sums for channel lane `lane` == tx)
    if (wave > 0 && head) {
      float* mine = red + (size_t)(wave - 1) * NA * CAP + lane;
#pragma unroll
      for (int k = 0; k < SC; ++k)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          mine[(size_t)((k * VEC + e) * 2) * CAP] = aw[k][e];
          mine[(size_t)((k * VEC + e) * 2 + 1) * CAP] = ab[k][e];
        }
    }
    __syncthreads();
    if (wave == 0 && head && live) {
      const float *w1 = red + lane, *w2 = w1 + (size_t)NA * CAP, *w3 = w2 + (size_t)NA * CAP;
#pragma unroll
      for (int k = 0; k < SC; ++k)
        if (s0 + k < s_end) {
          float* out = Js + ((int64_t)n * S + (s0 + k)) * P;
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            const size_t j = (size_t)((k * VEC + e) * 2) * CAP;
            const float sw = (aw[k][e] + w2[j]) + (w1[j] + w3[j]);
            const float sb = (ab[k][e] + w2[j + CAP]) + (w1[j + CAP] + w3[j + CAP]);
            if (wcol0 >= 0) out[wcol0 + c0 + e] = sw * scale;
            if (bcol0 >= 0) out[bcol0 + c0 + e] = sb * scale;
          }
        }
    }
    __syncthreads();  // (the next pass writes `red` again)
  }
}

// ---- host: the contract and the path of a shape ----------------------------------------------------------------------------------
struct NtPlan {
  int vec;    // channels per lane: 8 (16-byte plane loads), 4 (8-byte) or 1
  int sc;     // seeds per pass
  int cxw;    // channel vectors per workgroup (a power of two)
  int s_per;  // seeds per grid.y slice
  int64_t tiles, blocks;
};

// the part of the contract the entry point and the variant query share, with the messages under the caller's name
static int normtap_check_shape(const char* fn, int64_t S, int64_t B, int64_t L, int64_t Ch, bool aligned, NtPlan* p) {
  LK_REQUIRE(S >= 1 && S < (1ll << 31) && B >= 0 && B < (1ll << 31) && S * B < (1ll << 31) && L >= 1 && L < (1ll << 30) &&
                 Ch >= 1 && Ch < (1ll << 30),
             "%s: extent out of range (1 <= S, 0 <= B, S * B < 2^31, 1 <= L < 2^30, 1 <= Ch < 2^30)", fn);
  const unsigned __int128 count = (unsigned __int128)(S * B) * L * Ch;
  LK_REQUIRE(count < ((unsigned __int128)1 << 40), "%s: too many elements (S * B * L * Ch < 2^40)", fn);
  p->vec = aligned && Ch % 8 == 0 ? 8 : (aligned && Ch % 4 == 0 ? 4 : 1);
  p->sc = p->vec == 8 ? NtSc<8>::value : (p->vec == 4 ? NtSc<4>::value : NtSc<1>::value);
  const int64_t CV = Ch / p->vec;
  p->cxw = pow2_ceil(CV, p->vec == 1 ? NtCap<1>::value : NtCap<8>::value);
  p->tiles = (CV + p->cxw - 1) / p->cxw;
  p->blocks = B * p->tiles;
  LK_REQUIRE(p->blocks < (1ll << 31), "%s: too many channel tiles for one launch (B * tiles < 2^31)", fn);
  p->s_per = seeds_per_slice(S, p->blocks * 4);
  return LK_OK;
}

static int normtap_check(const void* g_h, const void* g_l, const int* sexp, const float* x, const float* mu, const float* rstd,
                         int64_t S, int64_t B, int64_t L, int64_t Ch, const float* Js, int64_t P, int64_t wcol0, int64_t bcol0,
                         NtPlan* p) {
  const char* fn = "lk_jac_norm_affine_nhwc_f16x2";
  LK_REQUIRE(g_h && g_l && sexp && x && Js, "%s: null pointer", fn);
  LK_REQUIRE((mu == nullptr) == (rstd == nullptr), "%s: mu and rstd are given together or not at all", fn);
  // vector class 8: 16-byte loads of the planes, of x and of mu / rstd; class 4: 8-byte plane loads, 16-byte fp32 loads
  const bool aligned = (((uintptr_t)g_h | (uintptr_t)g_l | (uintptr_t)x | (uintptr_t)mu | (uintptr_t)rstd) & 15) == 0;
  const int rc = normtap_check_shape(fn, S, B, L, Ch, aligned, p);
  if (rc != LK_OK) return rc;
  LK_REQUIRE((wcol0 < 0 || wcol0 + Ch <= P) && (bcol0 < 0 || bcol0 + Ch <= P), "%s: column range outside Js", fn);
  LK_REQUIRE(wcol0 < 0 || bcol0 < 0 || wcol0 + Ch <= bcol0 || bcol0 + Ch <= wcol0, "%s: weight and bias columns overlap", fn);
  return LK_OK;
}

}  // namespace lk

using namespace lk;

extern "C" int lk_jac_norm_affine_nhwc_f16x2(const void* g_h, const void* g_l, const int* sexp, const float* x, const float* mu,
                                             const float* rstd, int64_t S, int64_t B, int64_t L, int64_t Ch, float* Js, int64_t P,
                                             int64_t wcol0, int64_t bcol0, void* stream) {
  NtPlan p;
  const int rc = normtap_check(g_h, g_l, sexp, x, mu, rstd, S, B, L, Ch, Js, P, wcol0, bcol0, &p);
  if (rc != LK_OK) return rc;
  if (B == 0 || (wcol0 < 0 && bcol0 < 0)) return LK_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)p.blocks, (unsigned)((S + p.s_per - 1) / p.s_per));
  const _Float16 *gh = (const _Float16*)g_h, *gl = (const _Float16*)g_l;
#define LK_NT(V)                                                                                                               \
  hipLaunchKernelGGL((jac_normtap_kernel<V>), grid, dim3(256), 0, st, gh, gl, sexp, x, mu, rstd, (int)S, (int)B, (int)L, (int)Ch, \
                     p.cxw, (int)p.tiles, p.s_per, Js, P, wcol0, bcol0)
  if (p.vec == 8) LK_NT(8);
  else if (p.vec == 4) LK_NT(4);
  else LK_NT(1);
#undef LK_NT
  return check_launch("jac_normtap_kernel");
}

// vector class (0: 1 channel per lane, 1: 4, 2: 8) | seed-split << 2 | affine << 3 | seeds per pass << 4 | log2(lane rows per
// workgroup) << 8 | seeds per grid.y slice (capped at 255) << 12 | channel tiles per sample (capped at 2047) << 20
extern "C" int lk_normtap_variant(int64_t S, int64_t B, int64_t L, int64_t Ch, int affine, int aligned) {
  NtPlan p;
  if (normtap_check_shape("lk_normtap_variant", S, B, L, Ch, aligned != 0, &p) != LK_OK) return -1;
  int rows_log2 = 0;
  while ((p.cxw << rows_log2) < 256) ++rows_log2;
  const int slice = p.s_per > 255 ? 255 : p.s_per;
  const int tiles = p.tiles > 2047 ? 2047 : (int)p.tiles;
  return (p.vec == 8 ? 2 : (p.vec == 4 ? 1 : 0)) | (p.s_per < S ? 1 : 0) << 2 | (affine ? 1 : 0) << 3 | p.sc << 4 | rows_log2 << 8 |
         slice << 12 | tiles << 20;
}
