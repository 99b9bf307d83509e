// Samples of the GLM predictive, written out: (f_mu [B][C], f_var [B][C][C] or [B][C], z [C][n]) -> out [n][B][C], draw-major,
//   out[s][b][c] = f_mu[b][c] + sum_{j <= c} L_b[c][j] z[j][s],   L_b = chol(f_var_b)         (diag: sqrt(f_var[b][c]) z[c][s])
// or the row softmax of each draw.  Replaces the torch sequence of laplace/utils/utils.py:337-378 (normal_samples) behind
// laplace/baselaplace.py _glm_functional_samples / _glm_predictive_samples: a batched vendor Cholesky, a batched matmul with the
// shared draw, a broadcast add into [B][C][n] read back through permute(2, 0, 1), and for classification a softmax tensor of the
// same size.  One launch; z is given (the caller's draw), so the values are draw for draw those of the reference.
//
// The mc link (lk_link.hip) reduces over the draws and writes B C floats; this kernel writes n B C of them and is bound by that
// stream, so the work is split over (sample, DRAW CHUNK), grid.y running over the chunks.
//   The chunk rule (gs_split; a pure function of B, C, n, so two equal calls split alike).  Draws are dealt in stages of 16.
//   W = the workgroups one chunk needs (ceil(B / 4) in regime 0, B otherwise), stages = ceil(n / 16),
//   want = min(stages, ceil(512 / W))      (512 = two workgroups for each of the 256 CUs),
//   per = 16 ceil(stages / want) draws a chunk, chunks = ceil(n / per); chunk y owns draws [y per, min(n, (y + 1) per)).
//   Every chunk factorises its sample again: the same instructions on the same values, hence the same bits.  Chunk 0 alone
//   writes info[b].
// Three regimes (lk_glm_samples_variant names the one a shape takes, and the chunk count):
//   0  full covariance, C <= 64: a WAVE per (sample, chunk), four samples a workgroup.  The lower triangle is staged through a
//      wave-private LDS tile of odd row stride C | 1, the factor lives in registers a lane per row (chol_rows), L z is a
//      j-ascending fmaf chain per lane against wave-uniform loads of z, a draw's row is one coalesced store along c; the softmax
//      statistics are xor-shuffle trees.
//   1  full covariance, C <= 192: a WORKGROUP per (sample, chunk).  L is resident in LDS, CP = 16 ceil(C / 16) rows of CP + 1
//      floats with an identity tail.  Right-looking blocked Cholesky with 16-wide panels: wave 0 factors the diagonal block in
//      registers, the rows below are solved a thread per row, the trailing update runs tile by tile on v_mfma_f32_16x16x4_f32
//      (the exact fp32 instruction) round-robin over the four waves.  L z runs on the same instruction with z staged through LDS
//      16 draws at a time ([CP][16]); register r of lane (g, c16) of tile I is class 16 I + 4 g + r of draw s0 + c16, so a lane's
//      accumulator IS a 16-byte piece of an output row and goes out as one vector store (C % 4 == 0; four 4-byte stores
//      otherwise), or first through the softmax: maximum and sum over the lane groups by shuffles, over the waves through LDS.
//   2  marginal variances, C <= 4096: a workgroup per (sample, chunk), streaming.  Thread t owns the four adjacent classes
//      4 t + 1024 q .. + 3 for q < 4 (16 classes), f_mu and sqrt(f_var) in registers.  z is [C][n], a draw's column is strided:
//      a stage of ND = 16 | 8 | 4 draws (C <= 1024 | 2048 | 4096: about 64 KiB) is read along n and transposed into LDS as
//      [ND][CS], CS = 64 ceil(C / 64) + 64 / ND (the transposing writes and the 16-byte reads both fall on distinct banks).  The
//      softmax takes the maximum, the sum and the values in three passes over the staged tile (an fmaf each: nothing is kept
//      but the statistics), shuffle trees within a wave and one LDS exchange across the waves for all ND draws at once.  Every
//      store is a 16-byte vector where C % 4 == 0.
// A pivot that is not positive (or not finite) at column j: info[b] = j + 1 and all n rows of sample b are NaN; the other
// samples are unaffected.  One owner per output element, plain stores, fixed reduction orders, no atomics: bit-reproducible.
#include "lk_linkdev.h"  // wave_max, lane_bcast, chol_rows
#include "lk_stream.h"

#include <float.h>
#include <math.h>

namespace lk {

constexpr int GS_WAVE_C = 64;                    // largest C of the wave regime
constexpr int GS_MAX_C = LK_LINK_MAX_C;          // full covariance
constexpr int GS_MAX_C_DIAG = LK_LINK_WIDE_MAX_C;
constexpr int GS_NS = 16;                        // draws of a stage = columns of one matrix-instruction tile
constexpr int GS_MAXT = 3;                       // row tiles per wave: ceil(GS_MAX_C / 16 / 4)
constexpr int64_t GS_TARGET_WG = 512;            // two workgroups per CU

__device__ __forceinline__ float gs_nan() { return __int_as_float(0x7fc00000); }

// ---- 0: full covariance, C <= 64: a wave per (sample, chunk) ---------------------------------------------------------------------
template <int NC>
__global__ __launch_bounds__(256) void gs_wave_kernel(const float* __restrict__ f_mu, const float* __restrict__ f_var,
                                                      const float* __restrict__ z, int64_t B, int C, int n, int per, int softmax,
                                                      float* __restrict__ out, int* __restrict__ info) {
  extern __shared__ float lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + wave;
  const bool live = b < B, own = live && lane < C;
  const int ld = C | 1;
  float* tile = lds + wave * (C * ld);
  if (live) {
    const float* fv = f_var + b * C * C;
#pragma unroll 4
    for (int idx = lane; idx < C * C; idx += 64) {
      const int i = idx / C, j = idx - i * C;
      if (j <= i) tile[i * ld + j] = fv[idx];
    }
  }
  __syncthreads();
  if (!live) return;  // (no barrier below)
  float a[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) a[k] = (own && k <= lane) ? tile[lane * ld + k] : (k == lane ? 1.f : 0.f);
  const int bad = chol_rows<NC>(a, lane, C);
  if (blockIdx.y == 0 && lane == 0) info[b] = bad;
  const int sbeg = blockIdx.y * per, send = min(n, sbeg + per);
  const int64_t step = B * C;
  float* op = out + ((int64_t)sbeg * B + b) * C + lane;
  if (bad) {
    for (int s = sbeg; s < send; ++s, op += step)
      if (own) *op = gs_nan();
    return;
  }
  const float mu = own ? f_mu[b * C + lane] : 0.f;
  for (int s = sbeg; s < send; ++s, op += step) {
    float f = mu;
#pragma unroll
    for (int j = 0; j < NC; ++j)
      if (j < C) f = fmaf(a[j], z[(int64_t)j * n + s], f);  // (wave-uniform address; a[j] == 0 for j > lane)
    if (softmax) {
      const float m = wave_max(lane < C ? f : -INFINITY);
      const float e = lane < C ? expf(f - m) : 0.f;
      f = e / wave_sum(e);
    }
    if (own) *op = f;
  }
}

// ---- 1: full covariance, 64 < C <= 192: a workgroup per (sample, chunk), L resident in LDS ---------------------------------------
// row tile q of wave w: tiles are dealt 0 1 2 3 | 3 2 1 0 | 0 1 2 3 (tile I costs I + 1 products)
__device__ __forceinline__ int gs_row_tile(int q, int wave) { return 4 * q + ((q & 1) ? 3 - wave : wave); }

static inline size_t gs_block_lds(int64_t C) {
  const size_t CP = (size_t)((C + 15) / 16 * 16);
  return (CP * (CP + 1) + CP * GS_NS + 128 + 4) * sizeof(float);
}

template <bool VEC>
__global__ __launch_bounds__(256) void gs_block_kernel(const float* __restrict__ f_mu, const float* __restrict__ f_var,
                                                       const float* __restrict__ z, int64_t B, int C, int n, int per, int softmax,
                                                       float* __restrict__ out, int* __restrict__ info) {
  extern __shared__ float lds[];
  const int CP = (C + 15) & ~15, ld = CP + 1, T = CP >> 4;
  float* Lm = lds;                    // [CP][ld]
  float* zs = Lm + CP * ld;           // [CP][16]
  float* red = zs + CP * GS_NS;       // [2][4 waves][16 columns]
  int* flag = (int*)(red + 128);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c16 = lane & 15;
  const int64_t b = blockIdx.x;
  const float* fv = f_var + b * C * C;
  for (int i = wave; i < CP; i += 4)
    for (int j = lane; j < CP; j += 64) Lm[i * ld + j] = (i < C && j <= i) ? fv[i * C + j] : (i == j ? 1.f : 0.f);
  if (tid == 0) *flag = 0;
  __syncthreads();
  for (int p = 0; p < T; ++p) {
    const int j0 = 16 * p;
    if (wave == 0) {  // the diagonal block: rows in the registers of lanes 0..15
      float a[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) a[k] = (lane < 16 && k <= lane) ? Lm[(j0 + lane) * ld + j0 + k] : (k == lane ? 1.f : 0.f);
      const int bad = chol_rows<16>(a, lane, 16);
      if (bad) {
        if (lane == 0) *flag = j0 + bad;
      } else if (lane < 16) {
#pragma unroll
        for (int k = 0; k < 16; ++k) Lm[(j0 + lane) * ld + j0 + k] = a[k];  // (zeros above the diagonal: L z reads whole tiles)
      }
    }
    __syncthreads();
    if (*flag) break;  // (uniform)
    const int i = j0 + 16 + tid;  // the rows below: L21 = A21 L11^-T, a thread per row
    if (i < CP) {
      float r[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) r[k] = Lm[i * ld + j0 + k];
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        float v = r[c];
#pragma unroll
        for (int k = 0; k < c; ++k) v = fmaf(-r[k], Lm[(j0 + c) * ld + j0 + k], v);
        r[c] = v / Lm[(j0 + c) * ld + j0 + c];
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) Lm[i * ld + j0 + k] = r[k];
    }
    __syncthreads();
    int t = 0;  // trailing update of the lower tiles (I, J), p < J <= I: a tile per wave in turn
    for (int I = p + 1; I < T; ++I)
      for (int J = p + 1; J <= I; ++J, ++t) {
        if ((t & 3) != wave) continue;
        float* ct = Lm + (16 * I + 4 * g) * ld + 16 * J + c16;
        f32x4 acc = {ct[0], ct[ld], ct[2 * ld], ct[3 * ld]};
        const float* ar = Lm + (16 * I + c16) * ld + j0 + g;
        const float* br = Lm + (16 * J + c16) * ld + j0 + g;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(-ar[4 * kk], br[4 * kk], acc, 0, 0, 0);
        ct[0] = acc[0], ct[ld] = acc[1], ct[2 * ld] = acc[2], ct[3 * ld] = acc[3];
      }
    __syncthreads();
  }
  const int bad = *flag;
  if (blockIdx.y == 0 && tid == 0) info[b] = bad;
  const int sbeg = blockIdx.y * per, send = min(n, sbeg + per);
  if (bad) {
    for (int s = sbeg; s < send; ++s)
      for (int c = tid; c < C; c += 256) out[((int64_t)s * B + b) * C + c] = gs_nan();
    return;
  }
  f32x4 muv[GS_MAXT];
#pragma unroll
  for (int q = 0; q < GS_MAXT; ++q) {
    const int I = gs_row_tile(q, wave);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cls = 16 * I + 4 * g + r;
      muv[q][r] = cls < C ? f_mu[b * C + cls] : 0.f;
    }
  }
  for (int s0 = sbeg; s0 < send; s0 += GS_NS) {
    __syncthreads();  // (the previous stage and its statistics are read)
    for (int idx = tid; idx < CP * GS_NS; idx += 256) {
      const int k = idx >> 4, c = idx & 15;
      zs[idx] = (k < C && s0 + c < send) ? z[(int64_t)k * n + s0 + c] : 0.f;
    }
    __syncthreads();
    f32x4 f[GS_MAXT];
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < GS_MAXT; ++q) {
      const int I = gs_row_tile(q, wave);
      f[q] = muv[q];
      if (I < T) {
        const float* ar = Lm + (16 * I + c16) * ld + g;
        for (int J = 0; J <= I; ++J) {
          const float* br = zs + (16 * J + g) * GS_NS + c16;
#pragma unroll
          for (int kk = 0; kk < 4; ++kk)
            f[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[16 * J + 4 * kk], br[4 * kk * GS_NS], f[q], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (16 * I + 4 * g + r < C) m = fmaxf(m, f[q][r]);
      }
    }
    if (softmax) {  // (uniform) the statistics of draw s0 + c16: over the lane groups by shuffles, over the waves through LDS
      m = fmaxf(m, __shfl_xor(m, 16, 64));
      m = fmaxf(m, __shfl_xor(m, 32, 64));
      if (g == 0) red[wave * 16 + c16] = m;
      __syncthreads();
      m = fmaxf(fmaxf(red[c16], red[16 + c16]), fmaxf(red[32 + c16], red[48 + c16]));
      float sum = 0.f;
#pragma unroll
      for (int q = 0; q < GS_MAXT; ++q) {
        const int I = gs_row_tile(q, wave);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          f[q][r] = (I < T && 16 * I + 4 * g + r < C) ? expf(f[q][r] - m) : 0.f;
          sum += f[q][r];
        }
      }
      sum += __shfl_xor(sum, 16, 64);
      sum += __shfl_xor(sum, 32, 64);
      if (g == 0) red[64 + wave * 16 + c16] = sum;
      __syncthreads();
      sum = ((red[64 + c16] + red[80 + c16]) + red[96 + c16]) + red[112 + c16];
#pragma unroll
      for (int q = 0; q < GS_MAXT; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) f[q][r] /= sum;
    }
    if (s0 + c16 < send) {  // the tile goes out from the accumulators: a lane holds four adjacent classes of one draw
      float* op = out + ((int64_t)(s0 + c16) * B + b) * C;
#pragma unroll
      for (int q = 0; q < GS_MAXT; ++q) {
        const int cls = 16 * gs_row_tile(q, wave) + 4 * g;
        if (VEC) {
          if (cls < C) *reinterpret_cast<f32x4*>(op + cls) = f[q];
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (cls + r < C) op[cls + r] = f[q][r];
        }
      }
    }
  }
}

// ---- 2: marginal variances, C <= 4096: streaming, a workgroup per (sample, chunk) --------------------------------------------------
static inline int gs_diag_nd(int64_t C) { return C <= 1024 ? 16 : (C <= 2048 ? 8 : 4); }
static inline int64_t gs_diag_cs(int64_t C, int nd) { return (C + 63) / 64 * 64 + 64 / nd; }

template <int ND, bool VEC>
__global__ __launch_bounds__(256) void gs_diag_kernel(const float* __restrict__ f_mu, const float* __restrict__ f_var,
                                                      const float* __restrict__ z, int64_t B, int C, int n, int per, int softmax,
                                                      float* __restrict__ out, int* __restrict__ info) {
  extern __shared__ float lds[];
  const int C4 = (C + 3) & ~3, CS = ((C + 63) & ~63) + 64 / ND;
  float* zs = lds;            // [ND][CS]: draw d of the stage, class c
  float* red = zs + ND * CS;  // [2][4 waves][ND]
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int64_t b = blockIdx.x;
  float mu[4][4], sd[4][4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int cls = 1024 * q + 4 * t + e;
      mu[q][e] = cls < C ? f_mu[b * C + cls] : 0.f;
      sd[q][e] = cls < C ? sqrtf(f_var[b * C + cls]) : 0.f;
    }
  if (blockIdx.y == 0 && t == 0) info[b] = 0;
  const int sbeg = blockIdx.y * per, send = min(n, sbeg + per);
  for (int s0 = sbeg; s0 < send; s0 += ND) {
    __syncthreads();  // (the previous stage and its statistics are read)
    for (int idx = t; idx < C4 * ND; idx += 256) {  // global reads run along n, the LDS tile is draw-major
      const int c = idx / ND, d = idx % ND;
      zs[d * CS + c] = (c < C && s0 + d < send) ? z[(int64_t)c * n + s0 + d] : 0.f;
    }
    __syncthreads();
    float m[ND], sum[ND];
    if (softmax) {  // (uniform)
#pragma unroll
      for (int d = 0; d < ND; ++d) m[d] = -INFINITY, sum[d] = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c0 = 1024 * q + 4 * t;
        if (c0 < C4) {
#pragma unroll
          for (int d = 0; d < ND; ++d) {
            const f32x4 zz = *reinterpret_cast<const f32x4*>(zs + d * CS + c0);
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (c0 + e < C) m[d] = fmaxf(m[d], fmaf(sd[q][e], zz[e], mu[q][e]));
          }
        }
      }
#pragma unroll
      for (int d = 0; d < ND; ++d) m[d] = wave_max(m[d]);
      if (lane == 0) {
#pragma unroll
        for (int d = 0; d < ND; ++d) red[wave * ND + d] = m[d];
      }
      __syncthreads();
#pragma unroll
      for (int d = 0; d < ND; ++d) m[d] = fmaxf(fmaxf(red[d], red[ND + d]), fmaxf(red[2 * ND + d], red[3 * ND + d]));
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c0 = 1024 * q + 4 * t;
        if (c0 < C4) {
#pragma unroll
          for (int d = 0; d < ND; ++d) {
            const f32x4 zz = *reinterpret_cast<const f32x4*>(zs + d * CS + c0);
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (c0 + e < C) sum[d] += expf(fmaf(sd[q][e], zz[e], mu[q][e]) - m[d]);
          }
        }
      }
#pragma unroll
      for (int d = 0; d < ND; ++d) sum[d] = wave_sum(sum[d]);
      if (lane == 0) {
#pragma unroll
        for (int d = 0; d < ND; ++d) red[(4 + wave) * ND + d] = sum[d];
      }
      __syncthreads();
#pragma unroll
      for (int d = 0; d < ND; ++d) sum[d] = ((red[4 * ND + d] + red[5 * ND + d]) + red[6 * ND + d]) + red[7 * ND + d];
    }
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      if (s0 + d >= send) break;  // (uniform)
      float* op = out + ((int64_t)(s0 + d) * B + b) * C;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c0 = 1024 * q + 4 * t;
        if (c0 < C4) {
          const f32x4 zz = *reinterpret_cast<const f32x4*>(zs + d * CS + c0);
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[e] = fmaf(sd[q][e], zz[e], mu[q][e]);
            if (softmax) v[e] = expf(v[e] - m[d]) / sum[d];
          }
          if (VEC) {
            st<4>(op + c0, v);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (c0 + e < C) op[c0 + e] = v[e];
          }
        }
      }
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// the regime of a shape: 0 a wave per (sample, chunk), 1 a workgroup with L in LDS, 2 streaming over marginal variances; negative:
// outside the contract
static int gs_regime(int64_t B, int64_t C, int64_t n, int diag) {
  if (C < 1 || C > (diag ? GS_MAX_C_DIAG : GS_MAX_C) || B < 0 || B >= (1ll << 31) || n < 1 || n >= (1ll << 20)) return -1;
  if ((unsigned __int128)n * B * C >= ((unsigned __int128)1 << 40)) return -1;
  return diag ? 2 : (C <= GS_WAVE_C ? 0 : 1);
}

struct GsSplit {
  int chunks, per;  // chunk y owns draws [y per, min(n, (y + 1) per))
};
static GsSplit gs_split(int64_t B, int64_t n, int regime) {
  const int64_t W = regime == 0 ? (B + 3) / 4 : B, stages = (n + GS_NS - 1) / GS_NS;
  int64_t want = W > 0 ? (GS_TARGET_WG + W - 1) / W : 1;
  if (want > stages) want = stages;
  if (want < 1) want = 1;
  const int64_t per = (stages + want - 1) / want * GS_NS;
  return {(int)((n + per - 1) / per), (int)per};
}

static int gs_check(const float* f_mu, const float* f_var, const float* z, int64_t B, int64_t C, int64_t n, int diag,
                    const float* out, const int32_t* info) {
  LK_REQUIRE(f_mu && f_var && z && out && info, "lk_glm_samples_f32: null pointer");
  if (diag)
    LK_REQUIRE(C >= 1 && C <= GS_MAX_C_DIAG, "lk_glm_samples_f32: C = %lld outside 1 <= C <= LK_LINK_WIDE_MAX_C = %d (marginal variances)",
               (long long)C, GS_MAX_C_DIAG);
  else
    LK_REQUIRE(C >= 1 && C <= GS_MAX_C,
               "lk_glm_samples_f32: C = %lld outside 1 <= C <= LK_LINK_MAX_C = %d (the factor of a sample must fit the LDS)",
               (long long)C, GS_MAX_C);
  LK_REQUIRE(B >= 0 && B < (1ll << 31), "lk_glm_samples_f32: B out of range (0 <= B < 2^31)");
  LK_REQUIRE(n >= 1 && n < (1ll << 20), "lk_glm_samples_f32: n_samples out of range (1 <= n_samples < 2^20)");
  LK_REQUIRE((unsigned __int128)n * B * C < ((unsigned __int128)1 << 40),
             "lk_glm_samples_f32: n_samples * B * C out of range (< 2^40 output elements)");
  LK_REQUIRE((((uintptr_t)f_mu | (uintptr_t)f_var | (uintptr_t)z | (uintptr_t)out | (uintptr_t)info) & 15) == 0,
             "lk_glm_samples_f32: pointers must be 16-byte aligned");
  const unsigned __int128 bc = (unsigned __int128)B * C * 4, ob = bc * n, ib = (unsigned __int128)B * 4;
  const unsigned __int128 in_bytes[3] = {bc, diag ? bc : bc * C, (unsigned __int128)C * n * 4};
  const void* in[3] = {f_mu, f_var, z};
  for (int k = 0; k < 3; ++k)
    LK_REQUIRE(disjoint(out, ob, in[k], in_bytes[k]) && disjoint(info, ib, in[k], in_bytes[k]),
               "lk_glm_samples_f32: an output overlaps an input");
  LK_REQUIRE(disjoint(out, ob, info, ib), "lk_glm_samples_f32: out overlaps info");
  return LK_OK;
}

template <typename Kern>
static void gs_allow_lds(Kern kern, size_t bytes) {  // (every launch: the attribute belongs to the current device)
  if (bytes > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

#define GS_LAUNCH(KERN, GX)                                                                                                      \
  do {                                                                                                                           \
    gs_allow_lds(KERN, lds);                                                                                                     \
    hipLaunchKernelGGL(KERN, dim3((unsigned)(GX), (unsigned)sp.chunks), dim3(256), lds, st, f_mu, f_var, z, B, (int)C, (int)n,   \
                       sp.per, sm, out, info);                                                                                   \
  } while (0)

}  // namespace lk

using namespace lk;

extern "C" int lk_glm_samples_f32(const float* f_mu, const float* f_var, const float* z, int64_t B, int64_t C, int64_t n_samples,
                                  int diag, int softmax, float* out, int32_t* info, void* stream) {
  const int rc = gs_check(f_mu, f_var, z, B, C, n_samples, diag, out, info);
  if (rc != LK_OK) return rc;
  if (B == 0) return LK_OK;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = n_samples;
  const int regime = gs_regime(B, C, n, diag), sm = softmax != 0;
  const GsSplit sp = gs_split(B, n, regime);
  const bool vec = C % 4 == 0;
  if (regime == 0) {
    const size_t lds = (size_t)4 * C * (C | 1) * sizeof(float);
    const int64_t quads = (B + 3) / 4;
    if (C <= 16) GS_LAUNCH(gs_wave_kernel<16>, quads);
    else if (C <= 32) GS_LAUNCH(gs_wave_kernel<32>, quads);
    else GS_LAUNCH(gs_wave_kernel<64>, quads);
    return check_launch("gs_wave_kernel");
  }
  if (regime == 1) {
    const size_t lds = gs_block_lds(C);
    if (vec) GS_LAUNCH(gs_block_kernel<true>, B);
    else GS_LAUNCH(gs_block_kernel<false>, B);
    return check_launch("gs_block_kernel");
  }
  const int nd = gs_diag_nd(C);
  const size_t lds = (size_t)(nd * gs_diag_cs(C, nd) + 8 * nd) * sizeof(float);
  if (nd == 16) {
    if (vec) GS_LAUNCH((gs_diag_kernel<16, true>), B);
    else GS_LAUNCH((gs_diag_kernel<16, false>), B);
  } else if (nd == 8) {
    if (vec) GS_LAUNCH((gs_diag_kernel<8, true>), B);
    else GS_LAUNCH((gs_diag_kernel<8, false>), B);
  } else {
    if (vec) GS_LAUNCH((gs_diag_kernel<4, true>), B);
    else GS_LAUNCH((gs_diag_kernel<4, false>), B);
  }
  return check_launch("gs_diag_kernel");
}

// regime | chunks << 8 (softmax changes neither), or a negative value for a shape lk_glm_samples_f32 refuses
extern "C" int lk_glm_samples_variant(int64_t B, int64_t C, int64_t n_samples, int diag, int softmax) {
  (void)softmax;
  const int regime = gs_regime(B, C, n_samples, diag);
  if (regime < 0) return regime;
  return regime | gs_split(B, n_samples, regime).chunks << 8;
}
