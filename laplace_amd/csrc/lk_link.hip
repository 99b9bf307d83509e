// The link approximations of the GLM predictive for classification, fused: (f_mu [B][C], f_var [B][C][C] or [B][C]) -> probs [B][C]
//   probit        softmax(f_mu / sqrt(1 + pi/8 var_diag))
//   mc            L = chol(f_var_b);  f_s = f_mu + L z[:, s];  probs = (1 / n) sum_s softmax(f_s)      (z [C][n] is given)
//   bridge(_norm) the Dirichlet mean of the Laplace bridge from the row sums, column sums, total and diagonal of f_var_b
// Replaces the torch sequences of laplace/baselaplace.py:598-695 (the three links of _glm_predictive) and
// laplace/utils/utils.py:337-378 (normal_samples: a batched vendor Cholesky, a batched matmul with the shared draw, a
// [n][B][C] logits tensor, a softmax tensor of that size and a mean) by one launch that writes B C floats.
//
// Three regimes by C (lk_glm_link_variant names the one a shape takes):
//   C <= 64   one WAVE per sample, four samples per workgroup.  The sample's block is staged through a wave-private LDS tile whose
//             row stride C | 1 is odd (a lane per row reads its row with no bank conflict); the factorisation is right-looking,
//             column by column, a lane per row with the row in registers: the pivot and the column entries l_kj reach the other
//             lanes as v_readlane scalars.  L z is a j-ascending fmaf chain per lane against wave-uniform loads of z, the softmax
//             statistics of a sample column are xor-shuffle trees, sum_s p_s stays in one register per lane (= class).
//   C <= 192  one WORKGROUP per sample.  L is resident in LDS, padded to CP = 16 ceil(C / 16) rows of CP + 1 floats with an
//             identity tail (192 * 193 * 4 B = 148 KiB of the 160 KiB).  Right-looking blocked Cholesky with 16-wide panels: wave
//             0 factors the diagonal block with the register scheme above, the rows below it are solved a thread per row, and the
//             trailing update A22 -= L21 L21^T runs tile by tile on v_mfma_f32_16x16x4_f32 (the exact fp32 instruction: a
//             k-ordered fmaf chain) round-robin over the four waves.  L z runs on the same instruction, z staged through LDS 16
//             draws at a time ([CP][16]: the B operand is read conflict-free); the row tiles are dealt to the waves
//             boustrophedon (their cost grows with the row); maximum and sum of a sample column are reduced over the lane groups by
//             shuffles and over the waves through LDS; sum_s p_s is kept per class in registers and the 16 columns of a stage are
//             added in ascending s.
//   C > 192   refused (the factor does not fit the LDS); lk_linkwide.hip serves 193 to 4096 classes through an entry point of its own.
// Probit and bridge have no factorisation and keep no matrix: ONE streaming pass over the block (lanes along the columns keep the
// column sums, a shuffle tree per row gives the row sum, the diagonal is picked up on the way), with the geometry of the regime.
// Every output element has one owner, every reduction a fixed order, stores are plain: two equal calls are bit-equal.
#include "lk_linkdev.h"  // wave_max, lane_bcast, chol_rows
#include "lk_stream.h"

#include <float.h>
#include <math.h>

namespace lk {

constexpr int LINK_WAVE_C = 64;          // largest C of the wave-per-sample regime
constexpr int LINK_MAX_C = LK_LINK_MAX_C;
constexpr int LINK_NS = 16;              // draws per z stage = columns of one matrix-instruction tile
constexpr int LINK_MAXT = 3;             // row tiles per wave: ceil(LINK_MAX_C / 16 / 4)

// ---- mc, C <= 64: a wave per sample ---------------------------------------------------------------------------------------------
template <int NC>
__global__ __launch_bounds__(256) void link_mc_wave_kernel(const float* __restrict__ f_mu, const float* __restrict__ f_var,
                                                           const float* __restrict__ z, int64_t B, int C, int n, int diag,
                                                           float* __restrict__ probs, int* __restrict__ info) {
  extern __shared__ float lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + wave;
  const bool live = b < B, own = live && lane < C;
  const int ld = C | 1;
  float* tile = lds + wave * (C * ld);
  float a[NC];
  float sd = 0.f;
  int bad = 0;
  if (!diag) {
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
#pragma unroll
    for (int k = 0; k < NC; ++k) a[k] = (own && k <= lane) ? tile[lane * ld + k] : (k == lane ? 1.f : 0.f);
    bad = chol_rows<NC>(a, lane, C);
  } else {
    if (!live) return;
    if (own) sd = sqrtf(f_var[b * C + lane]);
  }
  if (bad) {
    if (own) probs[b * C + lane] = __int_as_float(0x7fc00000);
    if (lane == 0) info[b] = bad;
    return;
  }
  const float mu = own ? f_mu[b * C + lane] : 0.f;
  const float* zl = z + (own ? lane : 0) * n;
  float psum = 0.f;
  for (int s = 0; s < n; ++s) {
    float f = mu;
    if (diag) {
      f = fmaf(sd, zl[s], mu);
    } else {
#pragma unroll
      for (int j = 0; j < NC; ++j)
        if (j < C) f = fmaf(a[j], z[j * n + s], f);  // (wave-uniform address; a[j] == 0 for j > lane)
    }
    const float m = wave_max(lane < C ? f : -INFINITY);
    const float e = lane < C ? expf(f - m) : 0.f;
    psum += e / wave_sum(e);
  }
  if (own) probs[b * C + lane] = psum / (float)n;
  if (live && lane == 0) info[b] = 0;
}

// ---- mc, 64 < C <= 192: a workgroup per sample, L resident in LDS ---------------------------------------------------------------
// row tile q of wave w: tiles are dealt 0 1 2 3 | 3 2 1 0 | 0 1 2 3 (tile I costs I + 1 products)
__device__ __forceinline__ int link_row_tile(int q, int wave) { return 4 * q + ((q & 1) ? 3 - wave : wave); }

static inline size_t link_block_lds(int64_t C) {
  const size_t CP = (size_t)((C + 15) / 16 * 16);
  return (CP * (CP + 1) + CP * LINK_NS + 128 + 4) * sizeof(float);
}

__global__ __launch_bounds__(256) void link_mc_block_kernel(const float* __restrict__ f_mu, const float* __restrict__ f_var,
                                                            const float* __restrict__ z, int C, int n, int diag,
                                                            float* __restrict__ probs, int* __restrict__ info) {
  extern __shared__ float lds[];
  const int CP = (C + 15) & ~15, ld = CP + 1, T = CP >> 4;
  float* Lm = lds;                      // [CP][ld]
  float* zs = Lm + CP * ld;             // [CP][16]
  float* red = zs + CP * LINK_NS;       // [2][4 waves][16 columns]
  int* flag = (int*)(red + 128);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c16 = lane & 15;
  const int64_t b = blockIdx.x;
  const float* fv = f_var + (diag ? b * C : b * C * C);
  for (int i = wave; i < CP; i += 4)
    for (int j = lane; j < CP; j += 64) {
      float v = i == j ? 1.f : 0.f;
      if (i < C && j <= i) v = diag ? (i == j ? sqrtf(fv[i]) : 0.f) : fv[i * C + j];
      Lm[i * ld + j] = v;
    }
  if (tid == 0) *flag = 0;
  __syncthreads();
  if (!diag) {
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
  }
  const int bad = *flag;
  if (bad) {
    if (tid < C) probs[b * C + tid] = __int_as_float(0x7fc00000);
    if (tid == 0) info[b] = bad;
    return;
  }
  // f = f_mu + L z on row tiles of 16 classes x 16 draws: register r of lane (g, c16) is class 16 I + 4 g + r, draw s0 + c16
  float run[LINK_MAXT][4];
  f32x4 muv[LINK_MAXT];
#pragma unroll
  for (int q = 0; q < LINK_MAXT; ++q) {
    const int I = link_row_tile(q, wave);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cls = 16 * I + 4 * g + r;
      muv[q][r] = cls < C ? f_mu[b * C + cls] : 0.f;
      run[q][r] = 0.f;
    }
  }
  for (int s0 = 0; s0 < n; s0 += LINK_NS) {
    __syncthreads();  // (the previous stage and its statistics are read)
    for (int idx = tid; idx < CP * LINK_NS; idx += 256) {
      const int k = idx >> 4, c = idx & 15;
      zs[idx] = (k < C && s0 + c < n) ? z[k * n + s0 + c] : 0.f;
    }
    __syncthreads();
    f32x4 f[LINK_MAXT];
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < LINK_MAXT; ++q) {
      const int I = link_row_tile(q, wave);
      f[q] = muv[q];
      if (I < T) {
        const float* ar = Lm + (16 * I + c16) * ld + g;
        for (int J = diag ? I : 0; J <= I; ++J) {
          const float* br = zs + (16 * J + g) * LINK_NS + c16;
#pragma unroll
          for (int kk = 0; kk < 4; ++kk)
            f[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[16 * J + 4 * kk], br[4 * kk * LINK_NS], f[q], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (16 * I + 4 * g + r < C) m = fmaxf(m, f[q][r]);
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    if (g == 0) red[wave * 16 + c16] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[c16], red[16 + c16]), fmaxf(red[32 + c16], red[48 + c16]));
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < LINK_MAXT; ++q) {
      const int I = link_row_tile(q, wave);
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
    for (int q = 0; q < LINK_MAXT; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) f[q][r] /= sum;
    const int cnt = min(LINK_NS, n - s0);
    for (int nn = 0; nn < cnt; ++nn) {  // the stage's columns in ascending s (every lane of a group ends with the same sums)
#pragma unroll
      for (int q = 0; q < LINK_MAXT; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) run[q][r] += __shfl(f[q][r], (lane & 48) + nn, 64);
    }
  }
  if (c16 == 0) {
#pragma unroll
    for (int q = 0; q < LINK_MAXT; ++q) {
      const int I = link_row_tile(q, wave);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int cls = 16 * I + 4 * g + r;
        if (cls < C) probs[b * C + cls] = run[q][r] / (float)n;
      }
    }
  }
  if (tid == 0) info[b] = 0;
}

// ---- probit and the Laplace bridge: one streaming pass, NW waves per sample (1: four samples per workgroup, 4: one) -------------
template <int NW, bool MAX>
__device__ __forceinline__ float link_group_reduce(float v, float* red) {
  v = MAX ? wave_max(v) : wave_sum(v);
  if constexpr (NW == 1) {
    return v;
  } else {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return MAX ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : ((red[0] + red[1]) + red[2]) + red[3];
  }
}

template <int NW>
__global__ __launch_bounds__(256) void link_stream_kernel(const float* __restrict__ f_mu, const float* __restrict__ f_var, int64_t B,
                                                          int C, int link, int diag, float c1, float rk, float* __restrict__ probs,
                                                          int* __restrict__ info) {
  constexpr int CW = NW == 1 ? LINK_WAVE_C : LINK_MAX_C, NCOL = CW / 64, GROUPS = 4 / NW;
  __shared__ float sh[GROUPS][(2 + NW) * CW];
  __shared__ float red[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int grp = NW == 1 ? wave : 0, wsub = NW == 1 ? 0 : wave;
  const int t = NW == 1 ? lane : (int)threadIdx.x;  // the class this thread owns
  const int64_t b = (int64_t)blockIdx.x * GROUPS + grp;
  const bool live = b < B, own = live && t < C;
  float* rowS = sh[grp];
  float* dgS = rowS + CW;
  float* colP = dgS + CW;  // [NW][CW]
  const float mu = own ? f_mu[b * C + t] : 0.f;
  float row = 0.f, col = 0.f, dg = 0.f;
  if (diag) {
    dg = own ? f_var[b * C + t] : 0.f;
    row = col = dg;
  } else if (link == LK_LINK_PROBIT) {
    dg = own ? f_var[b * C * C + (int64_t)t * (C + 1)] : 0.f;
  } else {
    float cs[NCOL];
#pragma unroll
    for (int q = 0; q < NCOL; ++q) cs[q] = 0.f;
    if (live) {
      const float* fv = f_var + b * C * C;
      for (int i = wsub; i < C; i += NW) {
        float rs = 0.f;
#pragma unroll
        for (int q = 0; q < NCOL; ++q) {
          const int j = lane + 64 * q;
          const float v = j < C ? fv[i * C + j] : 0.f;
          cs[q] += v;
          rs += v;
          if (j == i) dgS[i] = v;
        }
        rs = wave_sum(rs);
        if (lane == 0) rowS[i] = rs;
      }
    }
#pragma unroll
    for (int q = 0; q < NCOL; ++q) colP[wsub * CW + lane + 64 * q] = cs[q];
    __syncthreads();
    if (own) {
      row = rowS[t];
      dg = dgS[t];
#pragma unroll
      for (int w = 0; w < NW; ++w) col += colP[w * CW + t];
    }
  }
  float out;
  if (link == LK_LINK_PROBIT) {
    const float x = (1.f / sqrtf(1.f + 0.39269908169872414f * dg)) * mu;  // pi / 8
    const float m = link_group_reduce<NW, true>(own ? x : -INFINITY, red);
    const float e = own ? expf(x - m) : 0.f;
    out = e / link_group_reduce<NW, false>(e, red);
  } else {
    const float K = (float)C;
    const float smu = link_group_reduce<NW, false>(mu, red);
    const float tot = link_group_reduce<NW, false>(row, red);
    float bm = mu - row * (smu / tot);
    float var = dg - row * col / tot;
    if (link == LK_LINK_BRIDGE_NORM) {
      const float scale = (link_group_reduce<NW, false>(own ? var : 0.f, red) / K) / rk;
      bm = bm / sqrtf(scale);
      var = var / scale;
    }
    const float sneg = link_group_reduce<NW, false>(own ? expf(-bm) : 0.f, red);
    const float alpha = (c1 + expf(bm) / (K * K) * sneg) / var;
    out = alpha / link_group_reduce<NW, false>(own ? alpha : 0.f, red);
    if (out != out) out = 1.f;  // torch.nan_to_num(nan=1.0): NaN -> 1, +-inf -> the largest finite values
    else if (out > FLT_MAX) out = FLT_MAX;
    else if (out < -FLT_MAX) out = -FLT_MAX;
  }
  if (own) probs[b * C + t] = out;
  if (live && t == 0) info[b] = 0;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
// the regime of a shape: 0 a wave per sample, 1 a workgroup per sample; negative: outside the contract
static int link_regime(int64_t B, int64_t C, int64_t n, int link, int diag) {
  (void)diag;
  if (link < 0 || link > 3 || C < 1 || C > LINK_MAX_C || B < 0 || B >= (1ll << 31)) return -1;
  if (link == LK_LINK_MC && (n < 1 || n >= (1ll << 20))) return -1;
  return C <= LINK_WAVE_C ? 0 : 1;
}

static int link_check(const float* f_mu, const float* f_var, const float* z, int64_t B, int64_t C, int64_t n, int link, int diag,
                      const float* probs, const int32_t* info) {
  LK_REQUIRE(link >= 0 && link <= 3, "lk_glm_link_f32: link must be 0 (probit), 1 (mc), 2 (bridge) or 3 (bridge_norm), got %d", link);
  LK_REQUIRE(f_mu && f_var && probs && info && (z || link != LK_LINK_MC), "lk_glm_link_f32: null pointer");
  LK_REQUIRE(C >= 1 && C <= LINK_MAX_C,
             "lk_glm_link_f32: C = %lld outside 1 <= C <= LK_LINK_MAX_C = %d (the factor of a sample must fit the LDS)", (long long)C,
             LINK_MAX_C);
  LK_REQUIRE(B >= 0 && B < (1ll << 31), "lk_glm_link_f32: B out of range (0 <= B < 2^31)");
  LK_REQUIRE(link != LK_LINK_MC || (n >= 1 && n < (1ll << 20)), "lk_glm_link_f32: n_samples out of range (1 <= n_samples < 2^20)");
  const float* zz = link == LK_LINK_MC ? z : nullptr;
  LK_REQUIRE((((uintptr_t)f_mu | (uintptr_t)f_var | (uintptr_t)zz | (uintptr_t)probs | (uintptr_t)info) & 15) == 0,
             "lk_glm_link_f32: pointers must be 16-byte aligned");
  const unsigned __int128 bc = (unsigned __int128)B * C * 4;
  const unsigned __int128 in_bytes[3] = {bc, diag ? bc : bc * C, zz ? (unsigned __int128)C * n * 4 : 0};
  const void* in[3] = {f_mu, f_var, zz};
  for (int k = 0; k < 3; ++k)
    LK_REQUIRE(disjoint(probs, bc, in[k], in_bytes[k]) && disjoint(info, (unsigned __int128)B * 4, in[k], in_bytes[k]),
               "lk_glm_link_f32: an output overlaps an input");
  LK_REQUIRE(disjoint(probs, bc, info, (unsigned __int128)B * 4), "lk_glm_link_f32: probs overlaps info");
  return LK_OK;
}

template <typename Kern>
static void link_allow_lds(Kern kern, size_t bytes) {  // (every launch: the attribute belongs to the current device)
  if (bytes > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace lk

using namespace lk;

extern "C" int lk_glm_link_f32(const float* f_mu, const float* f_var, const float* z, int64_t B, int64_t C, int64_t n_samples,
                               int link, int diag, float* probs, int32_t* info, void* stream) {
  const int rc = link_check(f_mu, f_var, z, B, C, n_samples, link, diag, probs, info);
  if (rc != LK_OK) return rc;
  if (B == 0) return LK_OK;
  hipStream_t st = (hipStream_t)stream;
  const int regime = link_regime(B, C, n_samples, link, diag), dg = diag != 0;
  const unsigned quads = (unsigned)((B + 3) / 4);
  if (link != LK_LINK_MC) {
    const float c1 = (float)(1.0 - 2.0 / (double)C), rk = (float)sqrt((double)C / 2.0);
    if (regime == 0)
      hipLaunchKernelGGL(link_stream_kernel<1>, dim3(quads), dim3(256), 0, st, f_mu, f_var, B, (int)C, link, dg, c1, rk, probs, info);
    else
      hipLaunchKernelGGL(link_stream_kernel<4>, dim3((unsigned)B), dim3(256), 0, st, f_mu, f_var, B, (int)C, link, dg, c1, rk, probs,
                         info);
    return check_launch("link_stream_kernel");
  }
  if (regime == 0) {
    const size_t lds = dg ? 0 : (size_t)4 * C * (C | 1) * sizeof(float);
#define LK_LINK_WAVE(NC)                                                                                                      \
  do {                                                                                                                        \
    link_allow_lds(link_mc_wave_kernel<NC>, lds);                                                                             \
    hipLaunchKernelGGL(link_mc_wave_kernel<NC>, dim3(quads), dim3(256), lds, st, f_mu, f_var, z, B, (int)C, (int)n_samples, dg, \
                       probs, info);                                                                                          \
  } while (0)
    if (C <= 16) LK_LINK_WAVE(16);
    else if (C <= 32) LK_LINK_WAVE(32);
    else LK_LINK_WAVE(64);
#undef LK_LINK_WAVE
    return check_launch("link_mc_wave_kernel");
  }
  const size_t lds = link_block_lds(C);
  link_allow_lds(link_mc_block_kernel, lds);
  hipLaunchKernelGGL(link_mc_block_kernel, dim3((unsigned)B), dim3(256), lds, st, f_mu, f_var, z, (int)C, (int)n_samples, dg, probs,
                     info);
  return check_launch("link_mc_block_kernel");
}

extern "C" int lk_glm_link_variant(int64_t B, int64_t C, int64_t n_samples, int link, int diag) {
  return link_regime(B, C, n_samples, link, diag);
}
