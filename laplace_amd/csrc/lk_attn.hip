// Scaled dot-product self-attention for the seed-batched reverse sweep: forward and the VJP of ALL seeds in one call,
//   P = softmax(scale * Q K^T (+ causal mask: key j <= query i)),  O = P V,
//   dV = P^T gO,  dP = gO V^T,  delta = rowsum(gO o O),  dS = P o (dP - delta),  dQ = scale dS K,  dK = scale dS^T Q,
// on fp32 operands [B][H][T][D] (layout 0) or [B][T][H][D] (layout 1, what Linear -> view -> transpose leaves); gO, dQ, dK, dV
// carry a leading [S] in the same layout.  The probabilities belong to the sample, not to the seed: they are rebuilt on chip
// from q, k and lse [B][H][T] (row maximum + log of the row sum of the scaled, masked scores) and never reach HBM.  Replaces,
// for an attention node, the reverse passes of laplace/curvature/curvlinops.py:87-100 (the KFAC backward) and of the jacrev
// materialisation of CurvatureInterface.jacobians, laplace/curvature/curvature.py:88-129 (one stock autograd pass per seed).
//
// All products run on the exact fp32 matrix instruction v_mfma_f32_16x16x4_f32 (bit for bit a k-ordered fmaf chain), in two
// forms whose results share one register map - column = lane & 15, row = 4 (lane >> 4) + register:
//   DOT   C[r][c]  = sum_d X[r][d] Y[c][d]     X: 16 rows of an LDS tile, Y: 16 rows held in registers (the OWNER's rows)
//   ACC   W[m][c] += sum_r X[r][m] Z[r][c]     X: the same LDS tile, Z: a DOT result used as the B operand as it lies
// so the owner's row is always the COLUMN: softmax statistics, delta and lse of a row are lane-local scalars, a DOT result
// feeds an ACC with no transposition, and the accumulators hold [d][owner row], stored as 16-byte vectors along d.
// A workgroup of 4 waves owns ATTN_BM = 64 rows (16 per wave) of one (b, h) and streams the other side through LDS in stages
// of ATTN_BN = 32 rows; D is padded to DP = 16, 32, 64 or 128 with zeros (fma(0, 0, c) == c).
//   forward   owner = query rows; streams K, V with the running-maximum softmax (the maximum is always subtracted)
//   VJP pass 1 owner = query rows; writes dq and delta [S][B][H][T] (workspace); streams K, V
//   VJP pass 2 owner = key rows;   writes dk, dv; streams Q, gO, lse, delta
// Every output element has one owner, a fixed reduction order and a plain store: two equal calls are bit-equal.
// RESIDENT (T <= ATTN_RESIDENT_MAX_T): the owner's P block [64][T] is built ONCE into LDS (each lane keeps its own registers'
// worth: no transposition, no barrier) and the seeds loop over it; beyond that it is rebuilt per seed.  Few (b, h, block)
// triples: the seeds are split over grid.y (each slice rebuilds P once).
// delta is accumulated in the order of the DOT chain (d = 16 c + 4 g + e over c, e, g), so that with T == 1, where O == V and
// P == 1, dP - delta is exactly 0.
// Minimal traffic of a VJP call: 4 S B H T D (2 reads of gO + 3 writes) + 8 S B H T (delta) + the per-sample operands.
#include "lk_attn_strided.h"
#include "lk_stream.h"

#include <math.h>

namespace lk {

constexpr int ATTN_BM = 64;               // owner rows per workgroup (16 per wave)
constexpr int ATTN_BN = 32;               // streamed rows per LDS stage
constexpr int ATTN_TILE = 16;             // rows and columns of one matrix-instruction tile (the softmax rescales per tile)
constexpr int ATTN_RESIDENT_MAX_T = 256;  // largest T whose [64][T] probability block stays in LDS (64 KiB)
constexpr int ATTN_MAX_D = 128;

struct AttnGeo {
  int64_t row, head, batch, seed;  // strides in floats (of o and go)
  int B, H, T, D;
};
// the strides of another group of tensors of the same [S][B][H][T][D] extents: GI the operands q, k, v (no seed), GD the cotangents
// dq, dk, dv.  Both equal the AttnGeo's own in layouts 0 and 1; the strided entry points set the row and batch strides
struct AttnStride {
  int64_t row, head, batch, seed;
};

template <int NC>
struct AttnTile {
  static constexpr int DP = 16 * NC, LD = DP + 4;  // (row stride of an LDS tile: 16-byte aligned, off the bank period)
};

// 16 floats per 16 of DP of one row: this lane's 4 adjacent d of every 16-wide chunk (zeros past D or for a dead row)
template <int NC>
__device__ __forceinline__ void attn_load_frag(const float* __restrict__ row, int D, int g, f32x4 (&f)[NC]) {
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int d = 16 * c + 4 * g;
    f[c] = (row != nullptr && d < D) ? *reinterpret_cast<const f32x4*>(row + d) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// ATTN_BN rows [row0, row0 + ATTN_BN) of one (b, h) -> LDS tile [ATTN_BN][LD]; rows >= T and d >= D are zeros
template <int NC>
__device__ __forceinline__ void attn_stage(float* __restrict__ dst, const float* __restrict__ base, int64_t row_stride, int row0,
                                           int T, int D) {
  constexpr int V = AttnTile<NC>::DP / 4, LD = AttnTile<NC>::LD;
  for (int i = threadIdx.x; i < ATTN_BN * V; i += 256) {
    const int r = i / V, c4 = i - r * V, row = row0 + r;
    f32x4 val = {0.f, 0.f, 0.f, 0.f};
    if (row < T && 4 * c4 < D) val = *reinterpret_cast<const f32x4*>(base + (int64_t)row * row_stride + 4 * c4);
    *reinterpret_cast<f32x4*>(dst + r * LD + 4 * c4) = val;
  }
}

// DOT: C[r][c] = sum_d X[r][d] Y[c][d]; xs: 16 rows of an LDS tile, yf: the fragment of row c = n of Y
template <int NC>
__device__ __forceinline__ f32x4 attn_dot(const float* __restrict__ xs, const f32x4 (&yf)[NC], int n, int g) {
  constexpr int LD = AttnTile<NC>::LD;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(xs + n * LD + 16 * c + 4 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], yf[c][e], acc, 0, 0, 0);
  }
  return acc;
}

// ACC: W[16 c + m][col] += sum_r X[r][16 c + m] Z[r][col]; z: a DOT result (row r = 4 g + register)
template <int NC>
__device__ __forceinline__ void attn_acc(const float* __restrict__ xs, const f32x4 z, f32x4 (&acc)[NC], int n, int g) {
  constexpr int LD = AttnTile<NC>::LD;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
      acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(xs[(4 * g + s) * LD + 16 * c + n], z[s], acc[c], 0, 0, 0);
  }
}

// sum_d a[d] b[d] of this lane's row in the order of the DOT chain (c, e, then the lane group g that holds d = 16 c + 4 g + e)
template <int NC>
__device__ __forceinline__ float attn_rowdot(const f32x4 (&a)[NC], const f32x4 (&b)[NC], int n) {
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int gg = 0; gg < 4; ++gg) acc = fmaf(__shfl(a[c][e], n + 16 * gg, 64), __shfl(b[c][e], n + 16 * gg, 64), acc);
  return acc;
}

template <int NC>
__device__ __forceinline__ void attn_store_frag(float* __restrict__ row, int D, int g, const f32x4 (&acc)[NC], float mul) {
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int d = 16 * c + 4 * g;
    if (d < D) *reinterpret_cast<f32x4*>(row + d) = f32x4{acc[c][0] * mul, acc[c][1] * mul, acc[c][2] * mul, acc[c][3] * mul};
  }
}

__device__ __forceinline__ float attn_colmax(float v) {  // over the 4 lane groups that share a column
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float attn_colsum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// blockIdx.x = ((b * H + h) * nblk + block of 64 query rows)
template <int NC>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                       const float* __restrict__ v, AttnGeo G, AttnStride GI, int nblk, float scale,
                                                       int causal, float* __restrict__ o, float* __restrict__ lse) {
  constexpr int LD = AttnTile<NC>::LD;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *xk = smem, *xv = smem + ATTN_BN * LD;
  const int bh = blockIdx.x / nblk, blk = blockIdx.x - bh * nblk, b = bh / G.H, h = bh - b * G.H;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
  const int T = G.T, D = G.D, q0 = blk * ATTN_BM, myrow = q0 + 16 * wave + n;
  const int64_t base = (int64_t)b * G.batch + (int64_t)h * G.head, ibase = (int64_t)b * GI.batch + (int64_t)h * GI.head;
  f32x4 qf[NC], acc[NC];
  attn_load_frag<NC>(myrow < T ? q + ibase + (int64_t)myrow * GI.row : nullptr, D, g, qf);
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;
  const int kend = causal ? min(T, q0 + ATTN_BM) : T;
  for (int k0 = 0; k0 < kend; k0 += ATTN_BN) {
    __syncthreads();
    attn_stage<NC>(xk, k + ibase, GI.row, k0, T, D);
    attn_stage<NC>(xv, v + ibase, GI.row, k0, T, D);
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < ATTN_BN / ATTN_TILE; ++sub) {
      const int kk = k0 + 16 * sub;
      if (kk >= kend || (causal && kk > q0 + 16 * wave + 15)) continue;  // (wave-uniform; key block 0 is never skipped)
      const f32x4 s = attn_dot<NC>(xk + sub * 16 * LD, qf, n, g);
      float sv[4], bm = -INFINITY;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int key = kk + 4 * g + t;
        sv[t] = (key < T && (!causal || key <= myrow)) ? s[t] * scale : -INFINITY;
        bm = fmaxf(bm, sv[t]);
      }
      const float mn = fmaxf(m, attn_colmax(bm));  // (finite: key 0 is valid for every row)
      const float alpha = expf(m - mn);
      f32x4 p;
      float rs = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        p[t] = sv[t] == -INFINITY ? 0.f : expf(sv[t] - mn);
        rs += p[t];
      }
      l = l * alpha + attn_colsum(rs);
      m = mn;
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c] *= alpha;
      attn_acc<NC>(xv + sub * 16 * LD, p, acc, n, g);
    }
  }
  if (myrow < T) {
    float* orow = o + base + (int64_t)myrow * G.row;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int d = 16 * c + 4 * g;
      if (d < D) *reinterpret_cast<f32x4*>(orow + d) = f32x4{acc[c][0] / l, acc[c][1] / l, acc[c][2] / l, acc[c][3] / l};
    }
    if (g == 0) lse[(int64_t)bh * T + myrow] = m + logf(l);
  }
}

// VJP pass 1: owner = 64 query rows; dq and delta.  blockIdx.x as the forward, blockIdx.y = seed slice
template <int NC, bool RESIDENT>
__global__ __launch_bounds__(256) void attn_vjp_q_kernel(const float* __restrict__ go, const float* __restrict__ q,
                                                         const float* __restrict__ k, const float* __restrict__ v,
                                                         const float* __restrict__ o, const float* __restrict__ lse, AttnGeo G,
                                                         AttnStride GI, AttnStride GD, int S, int nblk, int s_per, float scale,
                                                         int causal, float* __restrict__ dq, float* __restrict__ delta) {
  constexpr int LD = AttnTile<NC>::LD;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *xk = smem, *xv = smem + ATTN_BN * LD, *pres = smem + 2 * ATTN_BN * LD + threadIdx.x;  // pres[(tile * 4 + t) * 256]
  const int bh = blockIdx.x / nblk, blk = blockIdx.x - bh * nblk, b = bh / G.H, h = bh - b * G.H;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
  const int T = G.T, D = G.D, q0 = blk * ATTN_BM, myrow = q0 + 16 * wave + n;
  const int64_t base = (int64_t)b * G.batch + (int64_t)h * G.head, ibase = (int64_t)b * GI.batch + (int64_t)h * GI.head;
  const int64_t dbase = (int64_t)b * GD.batch + (int64_t)h * GD.head + (int64_t)myrow * GD.row;
  const bool live = myrow < T;
  f32x4 qf[NC];
  attn_load_frag<NC>(live ? q + ibase + (int64_t)myrow * GI.row : nullptr, D, g, qf);
  const float lse_i = live ? lse[(int64_t)bh * T + myrow] : 0.f;
  const int kend = causal ? min(T, q0 + ATTN_BM) : T;
  const int last_key = q0 + 16 * wave + 15;  // (causal: no key above it is visible to this wave)

  auto prob = [&](const float* xs, int kk) {
    const f32x4 s = attn_dot<NC>(xs, qf, n, g);
    f32x4 p;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int key = kk + 4 * g + t;
      p[t] = (live && key < T && (!causal || key <= myrow)) ? expf(s[t] * scale - lse_i) : 0.f;
    }
    return p;
  };

  if constexpr (RESIDENT) {
    for (int k0 = 0; k0 < kend; k0 += ATTN_BN) {
      __syncthreads();
      attn_stage<NC>(xk, k + ibase, GI.row, k0, T, D);
      __syncthreads();
#pragma unroll
      for (int sub = 0; sub < ATTN_BN / ATTN_TILE; ++sub) {
        const int kk = k0 + 16 * sub;
        if (kk >= kend || (causal && kk > last_key)) continue;
        const f32x4 p = prob(xk + sub * 16 * LD, kk);
#pragma unroll
        for (int t = 0; t < 4; ++t) pres[((kk >> 4) * 4 + t) * 256] = p[t];
      }
    }
  }
  const int s_end = min(S, ((int)blockIdx.y + 1) * s_per);
  for (int s = blockIdx.y * s_per; s < s_end; ++s) {
    const int64_t sbase = (int64_t)s * G.seed + base + (int64_t)myrow * G.row;
    f32x4 gof[NC], of[NC], acc[NC];
    attn_load_frag<NC>(live ? go + sbase : nullptr, D, g, gof);
    attn_load_frag<NC>(live ? o + base + (int64_t)myrow * G.row : nullptr, D, g, of);
    const float dl = attn_rowdot<NC>(gof, of, n);
    if (live && g == 0) delta[((int64_t)s * G.B * G.H + bh) * T + myrow] = dl;
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < kend; k0 += ATTN_BN) {
      __syncthreads();
      attn_stage<NC>(xk, k + ibase, GI.row, k0, T, D);
      attn_stage<NC>(xv, v + ibase, GI.row, k0, T, D);
      __syncthreads();
#pragma unroll
      for (int sub = 0; sub < ATTN_BN / ATTN_TILE; ++sub) {
        const int kk = k0 + 16 * sub;
        if (kk >= kend || (causal && kk > last_key)) continue;
        f32x4 p;
        if constexpr (RESIDENT) {
#pragma unroll
          for (int t = 0; t < 4; ++t) p[t] = pres[((kk >> 4) * 4 + t) * 256];
        } else {
          p = prob(xk + sub * 16 * LD, kk);
        }
        const f32x4 dp = attn_dot<NC>(xv + sub * 16 * LD, gof, n, g);
        f32x4 ds;
#pragma unroll
        for (int t = 0; t < 4; ++t) ds[t] = p[t] * (dp[t] - dl);
        attn_acc<NC>(xk + sub * 16 * LD, ds, acc, n, g);
      }
    }
    if (live) attn_store_frag<NC>(dq + (int64_t)s * GD.seed + dbase, D, g, acc, scale);
  }
}

// VJP pass 2: owner = 64 key rows; dk and dv.  Streams q, go (per seed), lse and delta
template <int NC, bool RESIDENT>
__global__ __launch_bounds__(256) void attn_vjp_kv_kernel(const float* __restrict__ go, const float* __restrict__ q,
                                                          const float* __restrict__ k, const float* __restrict__ v,
                                                          const float* __restrict__ lse, const float* __restrict__ delta,
                                                          AttnGeo G, AttnStride GI, AttnStride GD, int S, int nblk, int s_per,
                                                          float scale, int causal, float* __restrict__ dk,
                                                          float* __restrict__ dv) {
  constexpr int LD = AttnTile<NC>::LD;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *xq = smem, *xg = smem + ATTN_BN * LD, *pres = smem + 2 * ATTN_BN * LD + threadIdx.x;
  const int bh = blockIdx.x / nblk, blk = blockIdx.x - bh * nblk, b = bh / G.H, h = bh - b * G.H;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
  const int T = G.T, D = G.D, k0blk = blk * ATTN_BM, myrow = k0blk + 16 * wave + n;
  const int64_t base = (int64_t)b * G.batch + (int64_t)h * G.head, ibase = (int64_t)b * GI.batch + (int64_t)h * GI.head;
  const int64_t dbase = (int64_t)b * GD.batch + (int64_t)h * GD.head + (int64_t)myrow * GD.row;
  const bool live = myrow < T;
  f32x4 kf[NC], vf[NC];
  attn_load_frag<NC>(live ? k + ibase + (int64_t)myrow * GI.row : nullptr, D, g, kf);
  attn_load_frag<NC>(live ? v + ibase + (int64_t)myrow * GI.row : nullptr, D, g, vf);
  const int qstart = causal ? (k0blk / ATTN_BN) * ATTN_BN : 0;  // (causal: no query below the block's first key sees it)
  const int first_key = k0blk + 16 * wave;
  const float* lse_bh = lse + (int64_t)bh * T;

  auto prob = [&](const float* xs, int qq) {
    const f32x4 s = attn_dot<NC>(xs, kf, n, g);
    f32x4 p;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int qi = qq + 4 * g + t;
      p[t] = (live && qi < T && (!causal || myrow <= qi)) ? expf(s[t] * scale - lse_bh[qi]) : 0.f;
    }
    return p;
  };

  if constexpr (RESIDENT) {
    for (int i0 = qstart; i0 < T; i0 += ATTN_BN) {
      __syncthreads();
      attn_stage<NC>(xq, q + ibase, GI.row, i0, T, D);
      __syncthreads();
#pragma unroll
      for (int sub = 0; sub < ATTN_BN / ATTN_TILE; ++sub) {
        const int qq = i0 + 16 * sub;
        if (qq >= T || (causal && qq + 15 < first_key)) continue;
        const f32x4 p = prob(xq + sub * 16 * LD, qq);
#pragma unroll
        for (int t = 0; t < 4; ++t) pres[((qq >> 4) * 4 + t) * 256] = p[t];
      }
    }
  }
  const int s_end = min(S, ((int)blockIdx.y + 1) * s_per);
  for (int s = blockIdx.y * s_per; s < s_end; ++s) {
    const int64_t sbase = (int64_t)s * G.seed + base;
    const float* dl_bh = delta + ((int64_t)s * G.B * G.H + bh) * T;
    f32x4 acck[NC], accv[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acck[c] = accv[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int i0 = qstart; i0 < T; i0 += ATTN_BN) {
      __syncthreads();
      attn_stage<NC>(xq, q + ibase, GI.row, i0, T, D);
      attn_stage<NC>(xg, go + sbase, G.row, i0, T, D);
      __syncthreads();
#pragma unroll
      for (int sub = 0; sub < ATTN_BN / ATTN_TILE; ++sub) {
        const int qq = i0 + 16 * sub;
        if (qq >= T || (causal && qq + 15 < first_key)) continue;
        f32x4 p;
        if constexpr (RESIDENT) {
#pragma unroll
          for (int t = 0; t < 4; ++t) p[t] = pres[((qq >> 4) * 4 + t) * 256];
        } else {
          p = prob(xq + sub * 16 * LD, qq);
        }
        const f32x4 dp = attn_dot<NC>(xg + sub * 16 * LD, vf, n, g);
        f32x4 ds;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int qi = qq + 4 * g + t;
          ds[t] = p[t] * (dp[t] - (qi < T ? dl_bh[qi] : 0.f));
        }
        attn_acc<NC>(xg + sub * 16 * LD, p, accv, n, g);
        attn_acc<NC>(xq + sub * 16 * LD, ds, acck, n, g);
      }
    }
    if (live) {
      attn_store_frag<NC>(dk + (int64_t)s * GD.seed + dbase, D, g, acck, scale);
      attn_store_frag<NC>(dv + (int64_t)s * GD.seed + dbase, D, g, accv, 1.f);
    }
  }
}

// ---- host: the contract and the path of a shape ----------------------------------------------------------------------------------
struct AttnPlan {
  int nc;         // DP / 16: 1, 2, 4 or 8
  int resident;   // the owner's probability block stays in LDS over the seeds
  int s_per;      // seeds per grid.y slice
  int64_t nblk;   // owner blocks (of ATTN_BM rows) per (b, h)
  int64_t blocks;  // grid.x
  size_t lds_fwd, lds_vjp;
  AttnGeo geo;
  AttnStride in, out;  // (the strides of q, k, v and of dq, dk, dv: the geo's own unless a strided entry point sets them)
};

// the part of the contract the entry points and the variant query share, with the messages under the caller's name
static int attn_check_shape(const char* fn, int64_t S, int64_t B, int64_t H, int64_t T, int64_t D, int layout, AttnPlan* p) {
  LK_REQUIRE(layout == 0 || layout == 1, "%s: layout is 0 ([B][H][T][D]) or 1 ([B][T][H][D])", fn);
  LK_REQUIRE(D >= 4 && D <= ATTN_MAX_D && D % 4 == 0, "%s: head dim out of range (D %% 4 == 0, 4 <= D <= 128)", fn);
  LK_REQUIRE(S >= 1 && S < (1ll << 31) && B >= 0 && B < (1ll << 31) && S * B < (1ll << 31) && H >= 1 && H < (1ll << 16) &&
                 T >= 1 && T < (1ll << 15),
             "%s: extent out of range (1 <= S, 0 <= B, S * B < 2^31, 1 <= H < 2^16, 1 <= T < 2^15)", fn);
  const unsigned __int128 count = (unsigned __int128)(S * B) * H * T * D;
  LK_REQUIRE(count < ((unsigned __int128)1 << 40), "%s: too many elements (S * B * H * T * D < 2^40)", fn);
  p->nc = D <= 16 ? 1 : (D <= 32 ? 2 : (D <= 64 ? 4 : 8));
  p->nblk = (T + ATTN_BM - 1) / ATTN_BM;
  p->blocks = B * H * p->nblk;
  LK_REQUIRE(p->blocks < (1ll << 31), "%s: too many row blocks for one launch (B * H * ceil(T / 64) < 2^31)", fn);
  p->resident = T <= ATTN_RESIDENT_MAX_T;
  p->s_per = seeds_per_slice(S, p->blocks * 4);
  const size_t stage = (size_t)2 * ATTN_BN * (16 * p->nc + 4) * sizeof(float);
  p->lds_fwd = stage;
  p->lds_vjp = stage + (p->resident ? (size_t)((T + 15) / 16) * 4 * 256 * sizeof(float) : 0);
  AttnGeo& g = p->geo;
  g.B = (int)B, g.H = (int)H, g.T = (int)T, g.D = (int)D;
  g.row = layout == 0 ? D : H * D;
  g.head = layout == 0 ? T * D : D;
  g.batch = H * T * D;
  g.seed = B * H * T * D;
  p->in = p->out = AttnStride{g.row, g.head, g.batch, g.seed};
  return LK_OK;
}

static int attn_check(const char* fn, const void* const* in, const size_t* in_bytes, int n_in, const void* const* out,
                      const size_t* out_bytes, int n_out, float scale) {
  uintptr_t bits = 0;
  for (int i = 0; i < n_in; ++i) {
    LK_REQUIRE(in[i] != nullptr, "%s: null pointer", fn);
    bits |= (uintptr_t)in[i];
  }
  for (int i = 0; i < n_out; ++i) {
    LK_REQUIRE(out[i] != nullptr, "%s: null pointer", fn);
    bits |= (uintptr_t)out[i];
  }
  LK_REQUIRE((bits & 15) == 0, "%s: pointers must be 16-byte aligned", fn);
  LK_REQUIRE(isfinite(scale), "%s: scale must be finite", fn);
  for (int i = 0; i < n_out; ++i)
    for (int j = 0; j < n_in; ++j)
      LK_REQUIRE(disjoint(out[i], out_bytes[i], in[j], in_bytes[j]), "%s: an output overlaps an input", fn);
  return LK_OK;
}

static int attn_check_workspace(const char* fn, size_t need, size_t ws_bytes) {
  LK_REQUIRE(ws_bytes >= need, "%s: workspace too small (lk_attn_vjp_workspace_bytes)", fn);
  return LK_OK;
}

static size_t attn_delta_bytes(int64_t S, int64_t B, int64_t H, int64_t T) {
  return align_up((size_t)S * B * H * T * sizeof(float), 16);
}

template <typename Kern>
static void attn_allow_lds(Kern kern, size_t bytes) {  // (every launch: the attribute belongs to the current device)
  if (bytes > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

template <int NC>
static void attn_launch_fwd(const AttnPlan& p, const float* q, const float* k, const float* v, float scale, int causal, float* o,
                            float* lse, hipStream_t st) {
  hipLaunchKernelGGL((attn_fwd_kernel<NC>), dim3((unsigned)p.blocks), dim3(256), p.lds_fwd, st, q, k, v, p.geo, p.in, (int)p.nblk,
                     scale, causal, o, lse);
}

template <int NC, bool RES>
static void attn_launch_vjp(const AttnPlan& p, const float* go, const float* q, const float* k, const float* v, const float* o,
                            const float* lse, int S, float scale, int causal, float* dq, float* dk, float* dv, float* delta,
                            hipStream_t st) {
  const dim3 grid((unsigned)p.blocks, (unsigned)((S + p.s_per - 1) / p.s_per));
  attn_allow_lds(attn_vjp_q_kernel<NC, RES>, p.lds_vjp);
  hipLaunchKernelGGL((attn_vjp_q_kernel<NC, RES>), grid, dim3(256), p.lds_vjp, st, go, q, k, v, o, lse, p.geo, p.in, p.out, S,
                     (int)p.nblk, p.s_per, scale, causal, dq, delta);
  attn_allow_lds(attn_vjp_kv_kernel<NC, RES>, p.lds_vjp);
  hipLaunchKernelGGL((attn_vjp_kv_kernel<NC, RES>), grid, dim3(256), p.lds_vjp, st, go, q, k, v, lse, delta, p.geo, p.in, p.out, S,
                     (int)p.nblk, p.s_per, scale, causal, dk, dv);
}

}  // namespace lk

using namespace lk;

#define LK_ATTN_BY_NC(CALL) \
  switch (p.nc) {           \
    case 1: CALL(1); break; \
    case 2: CALL(2); break; \
    case 4: CALL(4); break; \
    default: CALL(8); break; \
  }

extern "C" int lk_attn_fwd_f32(const float* q, const float* k, const float* v, int64_t B, int64_t H, int64_t T, int64_t D, int layout,
                               float scale, int causal, float* o, float* lse, void* stream) {
  const char* fn = "lk_attn_fwd_f32";
  AttnPlan p;
  int rc = attn_check_shape(fn, 1, B, H, T, D, layout, &p);
  if (rc != LK_OK) return rc;
  const size_t n1 = (size_t)B * H * T * D * sizeof(float), nl = (size_t)B * H * T * sizeof(float);
  const void* in[3] = {q, k, v};
  const size_t in_bytes[3] = {n1, n1, n1};
  const void* out[2] = {o, lse};
  const size_t out_bytes[2] = {n1, nl};
  rc = attn_check(fn, in, in_bytes, 3, out, out_bytes, 2, scale);
  if (rc != LK_OK) return rc;
  if (B == 0) return LK_OK;
  hipStream_t st = (hipStream_t)stream;
#define LK_ATTN_FWD(N) attn_launch_fwd<N>(p, q, k, v, scale, causal != 0, o, lse, st)
  LK_ATTN_BY_NC(LK_ATTN_FWD)
#undef LK_ATTN_FWD
  return check_launch("attn_fwd_kernel");
}

extern "C" size_t lk_attn_vjp_workspace_bytes(int64_t S, int64_t B, int64_t H, int64_t T, int64_t D) {
  AttnPlan p;
  if (attn_check_shape("lk_attn_vjp_workspace_bytes", S, B, H, T, D, 0, &p) != LK_OK) return 0;
  return attn_delta_bytes(S, B, H, T);
}

extern "C" int lk_attn_vjp_f32(const float* go, const float* q, const float* k, const float* v, const float* o, const float* lse,
                               int64_t S, int64_t B, int64_t H, int64_t T, int64_t D, int layout, float scale, int causal, float* dq,
                               float* dk, float* dv, void* ws, size_t ws_bytes, void* stream) {
  const char* fn = "lk_attn_vjp_f32";
  AttnPlan p;
  int rc = attn_check_shape(fn, S, B, H, T, D, layout, &p);
  if (rc != LK_OK) return rc;
  const size_t n1 = (size_t)B * H * T * D * sizeof(float), nS = (size_t)S * n1, nl = (size_t)B * H * T * sizeof(float);
  const size_t need = attn_delta_bytes(S, B, H, T);
  const void* in[6] = {go, q, k, v, o, lse};
  const size_t in_bytes[6] = {nS, n1, n1, n1, n1, nl};
  const void* out[4] = {dq, dk, dv, ws};
  const size_t out_bytes[4] = {nS, nS, nS, need};
  rc = attn_check(fn, in, in_bytes, 6, out, out_bytes, 4, scale);
  if (rc != LK_OK) return rc;
  rc = attn_check_workspace(fn, need, ws_bytes);
  if (rc != LK_OK) return rc;
  if (B == 0) return LK_OK;
  hipStream_t st = (hipStream_t)stream;
#define LK_ATTN_VJP(N)                                                                                                    \
  if (p.resident) attn_launch_vjp<N, true>(p, go, q, k, v, o, lse, (int)S, scale, causal != 0, dq, dk, dv, (float*)ws, st); \
  else attn_launch_vjp<N, false>(p, go, q, k, v, o, lse, (int)S, scale, causal != 0, dq, dk, dv, (float*)ws, st)
  LK_ATTN_BY_NC(LK_ATTN_VJP)
#undef LK_ATTN_VJP
  return check_launch("attn_vjp_kernel");
}

// The strided entry points: layout 1 with a row stride of ldq floats for q, k, v (the slices of a packed projection where it left
// them) and of ldd floats for dq, dk, dv (one buffer that the projection's VJP reads); o, go and lse as in layout 1.  The same
// kernels on the same plan: with ldq = ldd = H D bit-equal to the layout-1 entry points (csrc/lk_attn_strided.h: their contract)
extern "C" int lk_attn_fwd_strided_f32(const float* q, const float* k, const float* v, int64_t ldq, int64_t B, int64_t H, int64_t T,
                                       int64_t D, float scale, int causal, float* o, float* lse, void* stream) {
  const char* fn = "lk_attn_fwd_strided_f32";
  AttnPlan p;
  int rc = attn_check_shape(fn, 1, B, H, T, D, 1, &p);
  if (rc != LK_OK) return rc;
  rc = attn_check_strides(fn, 1, B, H, T, D, ldq, ldq);
  if (rc != LK_OK) return rc;
  const size_t n1 = (size_t)B * H * T * D * sizeof(float), nl = (size_t)B * H * T * sizeof(float);
  const size_t ni = attn_strided_bytes(B * T, ldq, H * D);
  const void* in[3] = {q, k, v};
  const size_t in_bytes[3] = {ni, ni, ni};
  const void* out[2] = {o, lse};
  const size_t out_bytes[2] = {n1, nl};
  rc = attn_check(fn, in, in_bytes, 3, out, out_bytes, 2, scale);
  if (rc != LK_OK) return rc;
  if (B == 0) return LK_OK;
  p.in.row = ldq, p.in.batch = T * ldq;
  hipStream_t st = (hipStream_t)stream;
#define LK_ATTN_FWD(N) attn_launch_fwd<N>(p, q, k, v, scale, causal != 0, o, lse, st)
  LK_ATTN_BY_NC(LK_ATTN_FWD)
#undef LK_ATTN_FWD
  return check_launch("attn_fwd_kernel");
}

extern "C" int lk_attn_vjp_strided_f32(const float* go, const float* q, const float* k, const float* v, int64_t ldq, const float* o,
                                       const float* lse, int64_t S, int64_t B, int64_t H, int64_t T, int64_t D, float scale,
                                       int causal, float* dq, float* dk, float* dv, int64_t ldd, void* ws, size_t ws_bytes,
                                       void* stream) {
  const char* fn = "lk_attn_vjp_strided_f32";
  AttnPlan p;
  int rc = attn_check_shape(fn, S, B, H, T, D, 1, &p);
  if (rc != LK_OK) return rc;
  rc = attn_check_strides(fn, S, B, H, T, D, ldq, ldd);
  if (rc != LK_OK) return rc;
  const size_t n1 = (size_t)B * H * T * D * sizeof(float), nS = (size_t)S * n1, nl = (size_t)B * H * T * sizeof(float);
  const size_t ni = attn_strided_bytes(B * T, ldq, H * D), nd = attn_strided_bytes(S * B * T, ldd, H * D);
  const size_t need = attn_delta_bytes(S, B, H, T);
  const void* in[6] = {go, q, k, v, o, lse};
  const size_t in_bytes[6] = {nS, ni, ni, ni, n1, nl};
  const void* out[4] = {dq, dk, dv, ws};
  const size_t out_bytes[4] = {nd, nd, nd, need};
  rc = attn_check(fn, in, in_bytes, 6, out, out_bytes, 4, scale);
  if (rc != LK_OK) return rc;
  rc = attn_check_workspace(fn, need, ws_bytes);
  if (rc != LK_OK) return rc;
  const float* const outs[3] = {dq, dk, dv};
  rc = attn_check_interleave(fn, outs, 3, S * B * T, ldd, H * D);
  if (rc != LK_OK) return rc;
  if (B == 0) return LK_OK;
  p.in.row = ldq, p.in.batch = T * ldq;
  p.out.row = ldd, p.out.batch = T * ldd, p.out.seed = B * T * ldd;
  hipStream_t st = (hipStream_t)stream;
#define LK_ATTN_VJP(N)                                                                                                    \
  if (p.resident) attn_launch_vjp<N, true>(p, go, q, k, v, o, lse, (int)S, scale, causal != 0, dq, dk, dv, (float*)ws, st); \
  else attn_launch_vjp<N, false>(p, go, q, k, v, o, lse, (int)S, scale, causal != 0, dq, dk, dv, (float*)ws, st)
  LK_ATTN_BY_NC(LK_ATTN_VJP)
#undef LK_ATTN_VJP
  return check_launch("attn_vjp_kernel");
}

// resident | seed-split << 1 | log2(DP / 16) << 2 | causal << 4 | layout << 5 | seeds per grid.y slice (capped at 255) << 8 |
// owner blocks per (b, h) (capped at 4095) << 16
extern "C" int lk_attn_variant(int64_t S, int64_t B, int64_t H, int64_t T, int64_t D, int layout, int causal) {
  AttnPlan p;
  if (attn_check_shape("lk_attn_variant", S, B, H, T, D, layout, &p) != LK_OK) return -1;
  const int nc_log2 = p.nc == 1 ? 0 : (p.nc == 2 ? 1 : (p.nc == 4 ? 2 : 3));
  const int slice = p.s_per > 255 ? 255 : p.s_per;
  const int nblk = p.nblk > 4095 ? 4095 : (int)p.nblk;
  return p.resident | (p.s_per < S ? 1 : 0) << 1 | nc_log2 << 2 | (causal ? 1 : 0) << 4 | layout << 5 | slice << 8 | nblk << 16;
}
