// Forward and input VJP of the per-sample normalisation layers (GroupNorm, LayerNorm) for the seed-batched reverse sweep:
//   forward   mu, var over a statistics row;  rstd = 1 / sqrt(var + eps);  xhat = (x - mu) * rstd;  y = w * xhat + b
//   VJP       t = w * g;  m1 = mean_row(t);  m2 = mean_row(t * xhat);  dx = rstd * (t - m1 - xhat * m2)     for all S seeds
// Replaces the reverse passes through these layers of laplace/curvature/curvlinops.py:87-100 and curvature.py:88-129 (one stock
// autograd pass per seed).  Unlike an eval-mode BatchNorm (a per-channel scale, lk_vjp.hip) the VJP is a reduction per statistics
// row (n, group) of N = (Ch / G) * L elements; xhat and rstd are shared by all seeds.
//
// Geometry as lk_norm.hip: layout 0 is [B][Ch][L], layout 1 is [B][L][Ch].  Two kernels:
//   * ROW: a group of W lanes (a power of two <= 64) owns one statistics row; fixed xor-shuffle tree.  Serves layout 0 (the row is
//     N contiguous floats), layout 1 with L == 1 (LayerNorm: the row is Ch / G contiguous floats) and layout 1 with at least
//     NVJP_WIDE channels per group (runs of Ch / G floats, one per position).
//   * TILE: layout 1 with narrow groups (GroupNorm(32, 64) on NHWC: two channels per group).  A workgroup owns GT adjacent groups
//     of one sample so that its lanes still read whole channel vectors; lane columns are the channel vectors, lane rows stride
//     over the positions; per-channel sums meet in LDS (fixed halving tree), then one lane per group adds its channels in order.
// Both keep xhat and w of the row on chip across the seed loop and a seed's g between the reduction and the write while the row
// fits (NVJP_NV vectors per lane); longer rows read g twice.  16-byte loads where the contiguous extent is a multiple of 4
// floats and the pointers are 16-byte aligned, 4-byte loads otherwise.  Deterministic: every dx element has one owner, plain
// vector stores, no atomics on data; `amax` receives max|dx| as the bit pattern of a non-negative float through atomicMax, which
// is order-independent (wave_amax of lk_stream.h).  Few rows: the seeds are split over grid.y.
#include "lk_stream.h"

namespace lk {

constexpr int NVJP_SC = 2;     // seeds per pass of the on-chip paths (their g tiles are in flight together)
constexpr int NVJP_NV = 8;     // vectors of a row (ROW) / positions (TILE) a lane keeps on chip
constexpr int NVJP_WIDE = 16;  // layout 1, L > 1: channels per group from which a lane group owns a whole row
constexpr int NVJP_TILE_LANES = 16;  // TILE: channel vectors a workgroup aims to read per position
constexpr int NVJP_MAX_GT = 64;      // TILE: most groups per workgroup (one channel per group, 16-byte loads)

// Where the elements of a statistics row are: vector i of the row (VEC floats) is run i / cvt, vector i % cvt of that run
struct RowGeom {
  int64_t sample_stride;  // L * Ch
  int64_t row_stride;     // between the rows of adjacent groups of a sample: N (layout 0) or Ch / G (layout 1)
  int64_t pitch;          // between the runs of a row: Ch (layout 1; layout 0 has one run)
  int cvt;                // vectors per run
  int cpg;                // Ch / G
  int channel_major;      // layout 0: the channel of element e is e / L; layout 1: e % (Ch / G)
  FastDiv cvt_div, l_div;
};

template <int VEC>
__device__ __forceinline__ int64_t row_off(const RowGeom& q, int i, int& cv) {
  const int run = fdiv(i, q.cvt_div);
  cv = i - run * q.cvt;
  return (int64_t)run * q.pitch + (int64_t)cv * VEC;
}

// affine values of vector i of group grp (1 / 0 for a null pointer)
template <int VEC>
__device__ __forceinline__ void row_affine(const RowGeom& q, const float* __restrict__ p, float dflt, int grp, int i, int cv,
                                           float (&v)[VEC]) {
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    const int c = q.channel_major ? fdiv(i * VEC + e, q.l_div) : cv * VEC + e;
    v[e] = p != nullptr ? p[(int64_t)grp * q.cpg + c] : dflt;
  }
}

// ---- forward: a lane group per statistics row, mean-shifted two-pass variance ------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(256) void norm_fwd_row_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ b, int64_t R, int G, int N, RowGeom q,
                                                           int W, float eps, float* __restrict__ y,
                                                           float* __restrict__ xhat, float* __restrict__ rstd) {
  const int64_t row = (int64_t)blockIdx.x * (256 / W) + threadIdx.x / W;
  const int lane = threadIdx.x & (W - 1);
  const bool live = row < R;  // (dead groups stay in the shuffles and touch no memory)
  const int64_t n = live ? row / G : 0;
  const int grp = live ? (int)(row - n * G) : 0;
  const int64_t base = n * q.sample_stride + (int64_t)grp * q.row_stride;
  const int nvec = live ? N / VEC : 0;
  float sum = 0.f;
  for (int64_t iw = lane; iw < nvec; iw += W) {  // (64-bit: iw + W may pass 2^31 on the longest rows)
    const int i = (int)iw;
    int cv;
    float v[VEC];
    ld<VEC>(x + base + row_off<VEC>(q, i, cv), v);
#pragma unroll
    for (int e = 0; e < VEC; ++e) sum += v[e];
  }
  for (int off = W >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
  const float mu = sum / (float)N;
  float sq = 0.f;
  for (int64_t iw = lane; iw < nvec; iw += W) {
    const int i = (int)iw;
    int cv;
    float v[VEC];
    ld<VEC>(x + base + row_off<VEC>(q, i, cv), v);
#pragma unroll
    for (int e = 0; e < VEC; ++e) sq += (v[e] - mu) * (v[e] - mu);
  }
  for (int off = W >> 1; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
  const float rs = 1.0f / sqrtf(sq / (float)N + eps);
  for (int64_t iw = lane; iw < nvec; iw += W) {
    const int i = (int)iw;
    int cv;
    float v[VEC], wv[VEC], bv[VEC], xh[VEC], yv[VEC];
    const int64_t o = base + row_off<VEC>(q, i, cv);
    ld<VEC>(x + o, v);
    row_affine<VEC>(q, w, 1.f, grp, i, cv, wv);
    row_affine<VEC>(q, b, 0.f, grp, i, cv, bv);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      xh[e] = (v[e] - mu) * rs;
      yv[e] = wv[e] * xh[e] + bv[e];
    }
    st<VEC>(xhat + o, xh);
    st<VEC>(y + o, yv);
  }
  if (live && lane == 0) rstd[row] = rs;
}

// ---- VJP, ROW kernel ----------------------------------------------------------------------------------------------------------
template <int VEC, bool ONCHIP>
__global__ __launch_bounds__(256) void norm_vjp_row_kernel(const float* __restrict__ g, const float* __restrict__ xhat,
                                                           const float* __restrict__ rstd, const float* __restrict__ w,
                                                           int S, int64_t R, int G, int N, RowGeom q, int W, int s_per,
                                                           int64_t seed_stride, float* __restrict__ dx,
                                                           unsigned* __restrict__ amax) {
  const int64_t row = (int64_t)blockIdx.x * (256 / W) + threadIdx.x / W;
  const int lane = threadIdx.x & (W - 1);
  const bool live = row < R;
  const int64_t n = live ? row / G : 0;
  const int grp = live ? (int)(row - n * G) : 0;
  const int64_t base = n * q.sample_stride + (int64_t)grp * q.row_stride;
  const int nvec = live ? N / VEC : 0;
  const float rs = live ? rstd[row] : 0.f;
  const float fn = (float)N;
  const int s_begin = blockIdx.y * s_per;
  const int s_end = min(S, s_begin + s_per);
  float vmax = 0.f;
  if constexpr (ONCHIP) {
    float xv[NVJP_NV][VEC], wv[NVJP_NV][VEC];
    int64_t off[NVJP_NV];
#pragma unroll
    for (int k = 0; k < NVJP_NV; ++k) {
      const int i = k * W + lane;
      off[k] = -1;  // (no vector of the row here)
#pragma unroll
      for (int e = 0; e < VEC; ++e) xv[k][e] = wv[k][e] = 0.f;
      if (i < nvec) {
        int cv;
        off[k] = base + row_off<VEC>(q, i, cv);
        ld<VEC>(xhat + off[k], xv[k]);
        row_affine<VEC>(q, w, 1.f, grp, i, cv, wv[k]);
      }
    }
    for (int s0 = s_begin; s0 < s_end; s0 += NVJP_SC) {
      float t[NVJP_SC][NVJP_NV][VEC], a1[NVJP_SC], a2[NVJP_SC];
#pragma unroll
      for (int j = 0; j < NVJP_SC; ++j) {
        a1[j] = a2[j] = 0.f;
        const bool on = s0 + j < s_end;  // (uniform over the workgroup)
        const float* gs = g + (int64_t)(s0 + j) * seed_stride;
#pragma unroll
        for (int k = 0; k < NVJP_NV; ++k) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) t[j][k][e] = 0.f;
          if (on && off[k] >= 0) {
            ld<VEC>(gs + off[k], t[j][k]);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              t[j][k][e] *= wv[k][e];
              a1[j] += t[j][k][e];
              a2[j] += t[j][k][e] * xv[k][e];
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < NVJP_SC; ++j)
        for (int o = W >> 1; o > 0; o >>= 1) {
          a1[j] += __shfl_xor(a1[j], o, 64);
          a2[j] += __shfl_xor(a2[j], o, 64);
        }
#pragma unroll
      for (int j = 0; j < NVJP_SC; ++j) {
        if (s0 + j >= s_end) continue;
        const float m1 = a1[j] / fn, m2 = a2[j] / fn;
        float* ds = dx + (int64_t)(s0 + j) * seed_stride;
#pragma unroll
        for (int k = 0; k < NVJP_NV; ++k) {
          if (off[k] >= 0) {
            float d[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              d[e] = rs * (t[j][k][e] - m1 - xv[k][e] * m2);
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
      float a1 = 0.f, a2 = 0.f;
#pragma unroll 4
      for (int64_t iw = lane; iw < nvec; iw += W) {
        const int i = (int)iw;
        int cv;
        float gv[VEC], xv[VEC], wv[VEC];
        const int64_t o = base + row_off<VEC>(q, i, cv);
        ld<VEC>(gs + o, gv);
        ld<VEC>(xhat + o, xv);
        row_affine<VEC>(q, w, 1.f, grp, i, cv, wv);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const float t = gv[e] * wv[e];
          a1 += t;
          a2 += t * xv[e];
        }
      }
      for (int o = W >> 1; o > 0; o >>= 1) {
        a1 += __shfl_xor(a1, o, 64);
        a2 += __shfl_xor(a2, o, 64);
      }
      const float m1 = a1 / fn, m2 = a2 / fn;
#pragma unroll 4
      for (int64_t iw = lane; iw < nvec; iw += W) {
        const int i = (int)iw;
        int cv;
        float gv[VEC], xv[VEC], wv[VEC], d[VEC];
        const int64_t o = base + row_off<VEC>(q, i, cv);
        ld<VEC>(gs + o, gv);
        ld<VEC>(xhat + o, xv);
        row_affine<VEC>(q, w, 1.f, grp, i, cv, wv);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          d[e] = rs * (gv[e] * wv[e] - m1 - xv[e] * m2);
          vmax = fmaxf(vmax, fabsf(d[e]));
        }
        st<VEC>(ds + o, d);
      }
    }
  }
  wave_amax(vmax, amax);
}

// ---- VJP, TILE kernel: g [S][B][L][Ch], fewer than NVJP_WIDE channels per group ---------------------------------------------------
template <int VEC, bool ONCHIP>
__global__ __launch_bounds__(256) void norm_vjp_tile_kernel(const float* __restrict__ g, const float* __restrict__ xhat,
                                                            const float* __restrict__ rstd, const float* __restrict__ w,
                                                            int S, int L, int Ch, int G, int cpg, int GT, int CXW,
                                                            int s_per, int64_t seed_stride, float* __restrict__ dx,
                                                            unsigned* __restrict__ amax) {
  constexpr int SC = ONCHIP ? NVJP_SC : 1;  // (the two-pass path takes one seed at a time)
  constexpr int NV = ONCHIP ? NVJP_NV : 1;
  __shared__ float red[SC * 2 * 256 * VEC];        // [seed][t | t * xhat][lane row][channel of the tile]
  __shared__ float stat[SC * 2 * NVJP_MAX_GT];     // [seed][m1 | m2][group of the tile]
  const int tiles = (G + GT - 1) / GT;
  const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
  const int g_lo = tile * GT, g_live = min(GT, G - g_lo);
  const int c_lo = g_lo * cpg, cvt = g_live * cpg / VEC;
  const int tx = threadIdx.x & (CXW - 1), ty = threadIdx.x / CXW, TL = 256 / CXW;
  const bool live = tx < cvt;
  const int64_t mine = (int64_t)n * L * Ch + c_lo + tx * VEC;  // this lane's channel vector at position 0
  const int plane = TL * CXW * VEC;
  const float fn = (float)cpg * (float)L;
  const int s_begin = blockIdx.y * s_per;
  const int s_end = min(S, s_begin + s_per);
  float wv[VEC], rsv[VEC];
  int gl[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    const int c = tx * VEC + e;
    gl[e] = live ? c / cpg : 0;
    wv[e] = live ? (w != nullptr ? w[c_lo + c] : 1.f) : 0.f;
    rsv[e] = live ? rstd[(int64_t)n * G + g_lo + gl[e]] : 0.f;
  }
  float xv[NV][VEC];
  if constexpr (ONCHIP) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int l = ty + k * TL;
#pragma unroll
      for (int e = 0; e < VEC; ++e) xv[k][e] = 0.f;
      if (live && l < L) ld<VEC>(xhat + mine + (int64_t)l * Ch, xv[k]);
    }
  }
  float vmax = 0.f;
  for (int s0 = s_begin; s0 < s_end; s0 += SC) {
    float t[SC][NV][VEC], a1[SC][VEC], a2[SC][VEC];
#pragma unroll
    for (int j = 0; j < SC; ++j) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) a1[j][e] = a2[j][e] = 0.f;
      const bool on = s0 + j < s_end;  // (uniform over the workgroup)
      const float* gs = g + (int64_t)(s0 + j) * seed_stride + mine;
      if constexpr (ONCHIP) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
          const int l = ty + k * TL;
#pragma unroll
          for (int e = 0; e < VEC; ++e) t[j][k][e] = 0.f;
          if (on && live && l < L) {
            ld<VEC>(gs + (int64_t)l * Ch, t[j][k]);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              t[j][k][e] *= wv[e];
              a1[j][e] += t[j][k][e];
              a2[j][e] += t[j][k][e] * xv[k][e];
            }
          }
        }
      } else if (live) {
#pragma unroll 4
        for (int l = ty; l < L; l += TL) {
          float gv[VEC], xl[VEC];
          ld<VEC>(gs + (int64_t)l * Ch, gv);
          ld<VEC>(xhat + mine + (int64_t)l * Ch, xl);
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            const float tt = gv[e] * wv[e];
            a1[j][e] += tt;
            a2[j][e] += tt * xl[e];
          }
        }
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        red[(j * 2 + 0) * plane + (ty * CXW + tx) * VEC + e] = a1[j][e];
        red[(j * 2 + 1) * plane + (ty * CXW + tx) * VEC + e] = a2[j][e];
      }
    }
    __syncthreads();
    for (int st = TL >> 1; st > 0; st >>= 1) {  // the lane rows, halving
      if (ty < st) {
#pragma unroll
        for (int jq = 0; jq < SC * 2; ++jq)
#pragma unroll
          for (int e = 0; e < VEC; ++e)
            red[jq * plane + (ty * CXW + tx) * VEC + e] += red[jq * plane + ((ty + st) * CXW + tx) * VEC + e];
      }
      __syncthreads();
    }
    for (int idx = threadIdx.x; idx < SC * 2 * g_live; idx += 256) {  // the channels of a group, in order
      const int jq = idx / g_live, gi = idx - jq * g_live;
      float sum = 0.f;
      for (int c = 0; c < cpg; ++c) sum += red[jq * plane + gi * cpg + c];
      stat[jq * NVJP_MAX_GT + gi] = sum / fn;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SC; ++j) {
      if (s0 + j >= s_end || !live) continue;
      float m1[VEC], m2[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        m1[e] = stat[(j * 2 + 0) * NVJP_MAX_GT + gl[e]];
        m2[e] = stat[(j * 2 + 1) * NVJP_MAX_GT + gl[e]];
      }
      const float* gs = g + (int64_t)(s0 + j) * seed_stride + mine;
      float* ds = dx + (int64_t)(s0 + j) * seed_stride + mine;
      if constexpr (ONCHIP) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
          const int l = ty + k * TL;
          if (l < L) {
            float d[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              d[e] = rsv[e] * (t[j][k][e] - m1[e] - xv[k][e] * m2[e]);
              vmax = fmaxf(vmax, fabsf(d[e]));
            }
            st<VEC>(ds + (int64_t)l * Ch, d);
          }
        }
      } else {
#pragma unroll 4
        for (int l = ty; l < L; l += TL) {
          float gv[VEC], xl[VEC], d[VEC];
          ld<VEC>(gs + (int64_t)l * Ch, gv);
          ld<VEC>(xhat + mine + (int64_t)l * Ch, xl);
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            d[e] = rsv[e] * (gv[e] * wv[e] - m1[e] - xl[e] * m2[e]);
            vmax = fmaxf(vmax, fabsf(d[e]));
          }
          st<VEC>(ds + (int64_t)l * Ch, d);
        }
      }
    }
    // (the next pass writes `red` only after every lane has left the group sums above, and `stat` only after its own barriers)
  }
  wave_amax(vmax, amax);
}

// ---- host: which kernel a shape takes -------------------------------------------------------------------------------------------
struct NormPlan {
  int tile;     // 0: ROW kernel, 1: TILE kernel
  int vec;      // 16-byte loads
  int twopass;  // the row does not stay on chip
  int W;        // ROW: lanes per row; TILE: lanes across the channel vectors (CXW)
  int GT;       // TILE: groups per workgroup
  int s_per;    // seeds per grid.y slice
  int64_t blocks;
  int64_t N, cpg;
};

static inline int64_t gcd64(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// false: a shape outside the contract of the entry points (which refuse it with a message of their own)
static bool normvjp_plan(int64_t S, int64_t B, int64_t L, int64_t Ch, int64_t G, int layout, bool aligned, bool forward,
                         NormPlan* p) {
  if (S < 1 || B < 0 || L < 1 || Ch < 1 || G < 1 || (layout != 0 && layout != 1) || Ch % G != 0 || S >= (1ll << 31) ||
      B >= (1ll << 31) || L >= (1ll << 30) || Ch >= (1ll << 30) || (Ch / G) * L >= (1ll << 31))
    return false;
  p->cpg = Ch / G;
  p->N = p->cpg * L;
  p->GT = 1;
  if (layout == 0 || L == 1 || p->cpg >= NVJP_WIDE || forward) {
    p->tile = 0;
    p->vec = aligned && (layout == 0 ? p->N : p->cpg) % 4 == 0;
    const int64_t nvec = p->vec ? p->N / 4 : p->N;
    p->W = pow2_ceil(nvec, 64);
    p->twopass = nvec > (int64_t)p->W * NVJP_NV;
    p->blocks = (B * G + 256 / p->W - 1) / (256 / p->W);
  } else {
    p->tile = 1;
    p->vec = aligned && Ch % 4 == 0;
    const int64_t V = p->vec ? 4 : 1, g0 = V / gcd64(p->cpg, V), want = NVJP_TILE_LANES * V;
    int64_t GT = g0 * ((want + g0 * p->cpg - 1) / (g0 * p->cpg));  // (a multiple of g0: every tile starts on a vector)
    if (GT > G) GT = G;
    p->GT = (int)GT;
    p->W = pow2_ceil(GT * p->cpg / V, 256);
    p->twopass = L > (int64_t)(256 / p->W) * NVJP_NV;
    p->blocks = B * ((G + GT - 1) / GT);
  }
  p->s_per = seeds_per_slice(S, p->blocks * 4);
  return true;
}

static RowGeom row_geometry(const NormPlan& p, int64_t L, int64_t Ch, int layout) {
  const int V = p.vec ? 4 : 1;
  RowGeom q;
  q.sample_stride = L * Ch;
  q.row_stride = layout == 0 ? p.N : p.cpg;
  q.pitch = layout == 0 ? 0 : Ch;
  q.cvt = (int)((layout == 0 ? p.N : p.cpg) / V);
  q.cpg = (int)p.cpg;
  q.channel_major = layout == 0;
  q.cvt_div = make_fastdiv(q.cvt);
  q.l_div = make_fastdiv((int)L);
  return q;
}

// the part of the contract both entry points share, with the messages under the caller's name (used inside a checker function)
#define LK_NORMVJP_REQUIRE_SHAPE(FN, S, B, L, Ch, G, layout)                                                                  \
  LK_REQUIRE(layout == 0 || layout == 1, FN ": layout must be 0 ([B][Ch][L]) or 1 ([B][L][Ch])");                               \
  LK_REQUIRE(G >= 1 && Ch >= 1 && Ch % G == 0, FN ": G must be >= 1 and divide Ch");                                           \
  LK_REQUIRE(S >= 1 && S < (1ll << 31) && B >= 0 && B < (1ll << 31) && L >= 1 && L < (1ll << 30) && Ch < (1ll << 30),          \
             FN ": extent out of range (1 <= S < 2^31, 0 <= B < 2^31, 1 <= L, Ch < 2^30)");                                     \
  LK_REQUIRE((Ch / G) * L < (1ll << 31), FN ": statistics row too long ((Ch / G) * L < 2^31)")

static int normvjp_check_fwd(const float* x, int64_t B, int64_t L, int64_t Ch, int64_t G, int layout, const float* y,
                             const float* xhat, const float* rstd, NormPlan* plan) {
  LK_REQUIRE(x && y && xhat && rstd, "lk_norm_fwd_f32: null pointer");
  LK_NORMVJP_REQUIRE_SHAPE("lk_norm_fwd_f32", 1, B, L, Ch, G, layout);
  const bool aligned = (((uintptr_t)x | (uintptr_t)y | (uintptr_t)xhat) & 15) == 0;
  normvjp_plan(1, B, L, Ch, G, layout, aligned, true, plan);
  LK_REQUIRE(plan->blocks < (1ll << 31), "lk_norm_fwd_f32: too many rows for one launch");
  return LK_OK;
}

static int normvjp_check_vjp(const float* g, const float* xhat, const float* rstd, int64_t S, int64_t B, int64_t L,
                             int64_t Ch, int64_t G, int layout, const float* dx, NormPlan* plan) {
  LK_REQUIRE(g && xhat && rstd && dx, "lk_norm_vjp_f32: null pointer");
  LK_NORMVJP_REQUIRE_SHAPE("lk_norm_vjp_f32", S, B, L, Ch, G, layout);
  const unsigned __int128 bytes = (unsigned __int128)S * B * L * Ch * 4;
  const unsigned __int128 g0 = (uintptr_t)g, d0 = (uintptr_t)dx;
  LK_REQUIRE(g0 + bytes <= d0 || d0 + bytes <= g0, "lk_norm_vjp_f32: dx overlaps g");
  const bool aligned = (((uintptr_t)g | (uintptr_t)xhat | (uintptr_t)dx) & 15) == 0;
  normvjp_plan(S, B, L, Ch, G, layout, aligned, false, plan);
  LK_REQUIRE(plan->blocks < (1ll << 31), "lk_norm_vjp_f32: too many rows for one launch");
  return LK_OK;
}

}  // namespace lk

using namespace lk;

extern "C" int lk_norm_fwd_f32(const float* x, const float* w, const float* b, int64_t B, int64_t L, int64_t Ch, int64_t G,
                               int layout, float eps, float* y, float* xhat, float* rstd, void* stream) {
  NormPlan p;
  const int rc = normvjp_check_fwd(x, B, L, Ch, G, layout, y, xhat, rstd, &p);
  if (rc != LK_OK) return rc;
  if (B == 0) return LK_OK;
  const RowGeom q = row_geometry(p, L, Ch, layout);
  hipStream_t st = (hipStream_t)stream;
  if (p.vec)
    hipLaunchKernelGGL(norm_fwd_row_kernel<4>, dim3((unsigned)p.blocks), dim3(256), 0, st, x, w, b, B * G, (int)G, (int)p.N, q,
                       p.W, eps, y, xhat, rstd);
  else
    hipLaunchKernelGGL(norm_fwd_row_kernel<1>, dim3((unsigned)p.blocks), dim3(256), 0, st, x, w, b, B * G, (int)G, (int)p.N, q,
                       p.W, eps, y, xhat, rstd);
  return check_launch("norm_fwd_row_kernel");
}

extern "C" int lk_norm_vjp_f32(const float* g, const float* xhat, const float* rstd, const float* w, int64_t S, int64_t B,
                               int64_t L, int64_t Ch, int64_t G, int layout, float* dx, unsigned* amax, void* stream) {
  NormPlan p;
  const int rc = normvjp_check_vjp(g, xhat, rstd, S, B, L, Ch, G, layout, dx, &p);
  if (rc != LK_OK) return rc;
  if (B == 0) return LK_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)p.blocks, (unsigned)((S + p.s_per - 1) / p.s_per));
  const int64_t seed_stride = B * L * Ch;
  if (!p.tile) {
    const RowGeom q = row_geometry(p, L, Ch, layout);
#define LK_NORM_ROW(V, ON)                                                                                                  \
  hipLaunchKernelGGL((norm_vjp_row_kernel<V, ON>), grid, dim3(256), 0, st, g, xhat, rstd, w, (int)S, B * G, (int)G, (int)p.N, q, \
                     p.W, p.s_per, seed_stride, dx, amax)
    if (p.vec && !p.twopass) LK_NORM_ROW(4, true);
    else if (p.vec) LK_NORM_ROW(4, false);
    else if (!p.twopass) LK_NORM_ROW(1, true);
    else LK_NORM_ROW(1, false);
#undef LK_NORM_ROW
    return check_launch("norm_vjp_row_kernel");
  }
#define LK_NORM_TILE(V, ON)                                                                                                  \
  hipLaunchKernelGGL((norm_vjp_tile_kernel<V, ON>), grid, dim3(256), 0, st, g, xhat, rstd, w, (int)S, (int)L, (int)Ch, (int)G,   \
                     (int)p.cpg, p.GT, p.W, p.s_per, seed_stride, dx, amax)
  if (p.vec && !p.twopass) LK_NORM_TILE(4, true);
  else if (p.vec) LK_NORM_TILE(4, false);
  else if (!p.twopass) LK_NORM_TILE(1, true);
  else LK_NORM_TILE(1, false);
#undef LK_NORM_TILE
  return check_launch("norm_vjp_tile_kernel");
}

// kernel | vec << 1 | two-pass << 2 | seed-split << 3 | lanes << 4 | groups per workgroup << 16 (LK_NORMVJP_* of laplace_hip.h)
extern "C" int lk_norm_sweep_variant(int64_t S, int64_t B, int64_t L, int64_t Ch, int64_t G, int layout, int aligned) {
  NormPlan p;
  if (!normvjp_plan(S, B, L, Ch, G, layout, aligned != 0, false, &p) || p.blocks >= (1ll << 31)) return -1;
  return p.tile | p.vec << 1 | p.twopass << 2 | (p.s_per < S ? 1 : 0) << 3 | p.W << 4 | p.GT << 16;
}
