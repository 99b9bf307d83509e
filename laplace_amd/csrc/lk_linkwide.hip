// The link approximations of the GLM predictive for LK_LINK_MAX_C < C <= LK_LINK_WIDE_MAX_C classes, where the Cholesky factor of a
// sample no longer fits the LDS (lk_link.hip serves C <= 192): (f_mu [B][C], f_var [B][C][C] or [B][C]) -> probs [B][C].
// Replaces the torch sequences of laplace/baselaplace.py:598-695 and laplace/utils/utils.py:337-378, which at this width also form
// diag_embed(f_var) [B][C][C] for mc with the marginal variances, and for probit a [B][C][C] covariance only to read its diagonal.
// One launch, a workgroup of 256 threads (four waves) per sample, three kernels (lk_glm_link_wide_variant names the one a call takes):
//
//   2  mc, full covariance, C <= 224: an out-of-LDS blocked Cholesky, then L z, softmax and the mean in the same launch.  The
//      workgroups are persistent over b = blockIdx.x, blockIdx.x + slots, ..., each with its own slab [CP][CP] of the workspace
//      (CP = 32 ceil(C / 32)); L is written to the slab, f_var is read once and never written.  The factorisation is LEFT-looking
//      with 32-wide column panels: a right-looking update would re-write the trailing matrix for every panel (about C^3 / 48 * 8
//      bytes), the left-looking form only re-reads finished columns (C^3 / 48 floats).  The design is that of a 1024-class kernel
//      (the panel then takes 144 KiB of LDS); LK_LINK_WIDE_MAX_C_FULL stands at 224 because that is as far as the kernel has been
//      checked on a device, and the register tiers of L z (LW_MAXT) are sized for it.  For panel k:
//        1. the (CP - 32 k) x 32 panel of f_var goes to LDS with a row stride of 36 floats: the accumulator tiles of the matrix
//           instruction (bank 16 g + c16) and the 16-byte row reads of the solve (36 i mod 64 visits every fourth bank once in 16
//           rows) are both conflict-free;
//        2. panel -= L[32k:, :32k] L[32k:32k+32, :32k]^T on v_mfma_f32_16x16x4_f32 (the exact fp32 instruction) in k-slices of 64
//           columns, ascending.  The 32 pivot rows of a slice are staged in LDS once ([32][68]) and held in registers by every wave
//           for all its row tiles; the rows of L stream from the slab as 16-byte loads, one tile ahead of the products.  A lane's
//           16-byte load holds k = 4 g .. 4 g + 3, so instruction m of a 16-column group takes k = 4 g + m for both operands: a
//           fixed order, the same for every element.  A tile's accumulators live in the LDS panel between slices (every element
//           has one owning wave); the row tiles are dealt to the four waves boustrophedon;
//        3. wave 0 factors the 32 x 32 diagonal block in registers, a lane per row (chol_rows<32>); the rows below are solved a
//           thread per row against the block in LDS;
//        4. the panel is stored to the slab with zeros above the diagonal and an identity tail for rows and columns in [C, CP).
//      A pivot <= 0 or not finite sets info[b] = j + 1, makes row b of probs NaN and the workgroup goes on to its next sample.
//      __syncthreads() orders the slab writes before the same workgroup's reads; no workgroup reads another's slab.
//      f_s = f_mu + L z[:, s] runs on the same instruction with z staged 16 draws at a time through the LDS the panel has left
//      ([CP][20]: the operand reads fall on bank 16 g + c16), L read from the slab once per stage four tiles ahead; maximum and sum
//      of a draw over the classes by shuffles within a wave and through LDS across the waves; sum_s p_s per class in registers, the
//      16 columns of a stage added in ascending s; the division by n as in link_mc_block_kernel.
//   1  mc, marginal variances, C <= 4096: a thread owns classes t, t + 256, ... (at most 16) with f_mu and sqrt(f_var) in registers
//      for the whole draw loop; z [C][n] is read four draws at a time (16-byte loads where n % 4 == 0, scalar loads otherwise);
//      maximum and sum of the four draws in one pass of shuffles and one LDS exchange each; sum_s softmax stays in registers.
//   0  probit and bridge(_norm), C <= 4096: the streaming pass of link_stream_kernel for rows longer than the workgroup, up to 16
//      classes a thread.  The bridge over the full covariance reads the C x C block once: the rows are split over the four waves,
//      a wave's lanes run along the columns and keep its column sums in registers (16 per lane up to C = 1024, 64 beyond: a wave
//      owns whole rows, so the row sum is one shuffle tree), the diagonal is picked up on the way, the four partial column sums are
//      added in wave order.
// Every output element has one owner, every reduction a fixed order, stores are plain, no atomics: two equal calls are bit-equal.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; no kernel uses scratch): linkwide_mc_full_kernel 192 VGPRs,
// linkwide_mc_diag_kernel 187, linkwide_stream_kernel 219 (its 64-sums bridge tier included): two waves per SIMD each.
#include "lk_linkdev.h"  // wave_max, lane_bcast, chol_rows
#include "lk_stream.h"

#include <float.h>
#include <math.h>

namespace lk {

constexpr int LW_MIN_C = LK_LINK_MAX_C + 1;
constexpr int LW_MAX_C = LK_LINK_WIDE_MAX_C;
constexpr int LW_MAX_C_FULL = LK_LINK_WIDE_MAX_C_FULL;
constexpr int LW_NCL = LW_MAX_C / 256;       // classes a thread owns at most
constexpr int LW_PW = 32;                    // panel width
constexpr int LW_PS = 36;                    // row stride of the LDS panel
constexpr int LW_KS = 64;                    // columns of one k-slice
constexpr int LW_PVS = LW_KS + 4;            // row stride of the staged pivot rows
constexpr int LW_NS = 16;                    // draws per z stage
constexpr int LW_ZS = 20;                    // row stride of the staged draws
constexpr int LW_MAXT = (LW_MAX_C_FULL + 63) / 64;  // 16-row tiles per wave in L z
constexpr int64_t LW_MAX_SLOTS = 256;        // slabs lk_glm_link_wide_work_bytes asks for at most

// row tile q of wave w: tiles are dealt 0 1 2 3 | 3 2 1 0 | 0 1 2 3 ...
__device__ __forceinline__ int lw_row_tile(int q, int wave) { return 4 * q + ((q & 1) ? 3 - wave : wave); }

__device__ __forceinline__ float lw_nan() { return __int_as_float(0x7fc00000); }

// maximum or sum over the workgroup of NV values per thread at once (one LDS exchange); red holds 4 * NV floats
template <int NV, bool MAX>
__device__ __forceinline__ void lw_block_reduce(float (&v)[NV], float* red) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int e = 0; e < NV; ++e) v[e] = MAX ? wave_max(v[e]) : wave_sum(v[e]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int e = 0; e < NV; ++e) red[wave * NV + e] = v[e];
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < NV; ++e)
    v[e] = MAX ? fmaxf(fmaxf(red[e], red[NV + e]), fmaxf(red[2 * NV + e], red[3 * NV + e]))
               : ((red[e] + red[NV + e]) + red[2 * NV + e]) + red[3 * NV + e];
}
template <bool MAX>
__device__ __forceinline__ float lw_block_reduce1(float x, float* red) {
  float v[1] = {x};
  lw_block_reduce<1, MAX>(v, red);
  return v[0];
}

// ---- 2: mc with the full covariance ----------------------------------------------------------------------------------------------
static inline size_t lw_full_lds(int64_t CP) {
  return (size_t)(CP * LW_PS + LW_PW * LW_PVS + CP + 128 + 4) * sizeof(float);
}

__global__ __launch_bounds__(256) void linkwide_mc_full_kernel(const float* __restrict__ f_mu, const float* __restrict__ f_var,
                                                               const float* __restrict__ z, int64_t B, int C, int n,
                                                               float* __restrict__ probs, int* __restrict__ info, float* work) {
  extern __shared__ float lds[];
  const int CP = (C + 31) & ~31, T = CP >> 4;
  float* pan = lds;                    // [CP - k0][36] during the factorisation, then the draws [CP][20]
  float* piv = pan + CP * LW_PS;       // [32][68]
  float* mus = piv + LW_PW * LW_PVS;   // [CP]
  float* red = mus + CP;               // [2][4 waves][16 columns]
  int* flag = (int*)(red + 128);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c16 = lane & 15;
  float* slab = work + (size_t)blockIdx.x * CP * CP;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const float* fv = f_var + b * C * C;
    if (tid == 0) *flag = 0;
    // ---- the factorisation, panel by panel -------------------------------------------------------------------------------------
    for (int k0 = 0; k0 < CP; k0 += LW_PW) {
      const int R = CP - k0, RT = R >> 4;
      __syncthreads();  // (the previous panel is stored, the flag is set)
      for (int idx = tid; idx < R * LW_PW; idx += 256) {
        const int i = idx >> 5, c = idx & 31, gi = k0 + i, gj = k0 + c;
        pan[i * LW_PS + c] = (gi < C && gj <= gi) ? fv[gi * C + gj] : (gi == gj ? 1.f : 0.f);
      }
      for (int ks = 0; ks < k0; ks += LW_KS) {
        const int klen = min(LW_KS, k0 - ks);  // 32 or 64
        __syncthreads();                       // (the previous slice's pivot rows are in registers; the panel is loaded)
        for (int idx = tid; idx < LW_PW * (LW_KS / 4); idx += 256) {
          const int c = idx >> 4, v4 = idx & 15;
          const f32x4 v = 4 * v4 < klen ? *(const f32x4*)(slab + (size_t)(k0 + c) * CP + ks + 4 * v4) : zero4;
          *(f32x4*)(piv + c * LW_PVS + 4 * v4) = v;
        }
        __syncthreads();
        f32x4 b0[4], b1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          b0[u] = *(const f32x4*)(piv + c16 * LW_PVS + 16 * u + 4 * g);
          b1[u] = *(const f32x4*)(piv + (16 + c16) * LW_PVS + 16 * u + 4 * g);
        }
        f32x4 an[4];
        auto load_a = [&](int t) {
          const float* ap = slab + (size_t)(k0 + 16 * t + c16) * CP + ks + 4 * g;
#pragma unroll
          for (int u = 0; u < 4; ++u) an[u] = 16 * u < klen ? *(const f32x4*)(ap + 16 * u) : zero4;
        };
        if (wave < RT) load_a(lw_row_tile(0, wave));
        for (int q = 0; 4 * q < RT; ++q) {
          const int t = lw_row_tile(q, wave);
          if (t >= RT) continue;  // (uniform per wave; only in the last group of four)
          f32x4 a[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) a[u] = an[u];
          const int tn = lw_row_tile(q + 1, wave);
          if (tn < RT) load_a(tn);
          float* ct = pan + (16 * t + 4 * g) * LW_PS + c16;
          f32x4 acc0 = {ct[0], ct[LW_PS], ct[2 * LW_PS], ct[3 * LW_PS]};
          f32x4 acc1 = {ct[16], ct[LW_PS + 16], ct[2 * LW_PS + 16], ct[3 * LW_PS + 16]};
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (16 * u < klen) {
#pragma unroll
              for (int m = 0; m < 4; ++m) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(-a[u][m], b0[u][m], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(-a[u][m], b1[u][m], acc1, 0, 0, 0);
              }
            }
          ct[0] = acc0[0], ct[LW_PS] = acc0[1], ct[2 * LW_PS] = acc0[2], ct[3 * LW_PS] = acc0[3];
          ct[16] = acc1[0], ct[LW_PS + 16] = acc1[1], ct[2 * LW_PS + 16] = acc1[2], ct[3 * LW_PS + 16] = acc1[3];
        }
      }
      __syncthreads();
      if (wave == 0) {  // the diagonal block: rows in the registers of lanes 0..31
        float a[LW_PW];
        float* rp = pan + (lane & 31) * LW_PS;
#pragma unroll
        for (int k4 = 0; k4 < LW_PW; k4 += 4) {
          const f32x4 v = *(const f32x4*)(rp + k4);
#pragma unroll
          for (int e = 0; e < 4; ++e) a[k4 + e] = (lane < LW_PW && k4 + e <= lane) ? v[e] : 0.f;
        }
        const int bad = chol_rows<LW_PW>(a, lane, LW_PW);  // (the identity tail factors to itself)
        if (bad) {
          if (lane == 0) *flag = k0 + bad;
        } else if (lane < LW_PW) {
#pragma unroll
          for (int k4 = 0; k4 < LW_PW; k4 += 4) {
            const f32x4 v = {a[k4], a[k4 + 1], a[k4 + 2], a[k4 + 3]};
            *(f32x4*)(rp + k4) = v;  // (zeros above the diagonal: L z reads whole tiles)
          }
        }
      }
      __syncthreads();
      if (*flag) break;  // (uniform)
      for (int i = LW_PW + tid; i < R; i += 256) {  // the rows below: L21 = A21 L11^-T, a thread per row
        float r[LW_PW];
        float* rp = pan + i * LW_PS;
#pragma unroll
        for (int k4 = 0; k4 < LW_PW; k4 += 4) {
          const f32x4 v = *(const f32x4*)(rp + k4);
          r[k4] = v[0], r[k4 + 1] = v[1], r[k4 + 2] = v[2], r[k4 + 3] = v[3];
        }
#pragma unroll
        for (int c = 0; c < LW_PW; ++c) {
          float v = r[c];
#pragma unroll
          for (int k = 0; k < c; ++k) v = fmaf(-r[k], pan[c * LW_PS + k], v);
          r[c] = v / pan[c * LW_PS + c];
        }
#pragma unroll
        for (int k4 = 0; k4 < LW_PW; k4 += 4) {
          const f32x4 v = {r[k4], r[k4 + 1], r[k4 + 2], r[k4 + 3]};
          *(f32x4*)(rp + k4) = v;
        }
      }
      __syncthreads();
      for (int idx = tid; idx < R * (LW_PW / 4); idx += 256) {
        const int i = idx >> 3, v4 = idx & 7;
        *(f32x4*)(slab + (size_t)(k0 + i) * CP + k0 + 4 * v4) = *(const f32x4*)(pan + i * LW_PS + 4 * v4);
      }
    }
    __syncthreads();  // (the last panel is stored; every thread has read the flag inside the loop)
    const int bad = *flag;
    if (bad) {
      for (int c = tid; c < C; c += 256) probs[b * C + c] = lw_nan();
      if (tid == 0) info[b] = bad;
      __syncthreads();  // (the flag is read before the next sample clears it)
      continue;
    }
    // ---- f = f_mu + L z on row tiles of 16 classes x 16 draws: register r of lane (g, c16) is class 16 I + 4 g + r, draw s0 + c16 --
    for (int c = tid; c < CP; c += 256) mus[c] = c < C ? f_mu[b * C + c] : 0.f;
    float* zs = pan;
    float run[LW_MAXT][4];
#pragma unroll
    for (int q = 0; q < LW_MAXT; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) run[q][r] = 0.f;
    for (int s0 = 0; s0 < n; s0 += LW_NS) {
      __syncthreads();  // (the previous stage and its statistics are read; mus is written)
      for (int idx = tid; idx < CP * LW_NS; idx += 256) {
        const int k = idx >> 4, c = idx & 15;
        zs[k * LW_ZS + c] = (k < C && s0 + c < n) ? z[k * n + s0 + c] : 0.f;
      }
      __syncthreads();
      f32x4 f[LW_MAXT];
      float m = -INFINITY;
#pragma unroll
      for (int q = 0; q < LW_MAXT; ++q) {
        const int I = lw_row_tile(q, wave);
        f[q] = zero4;
        if (I < T) {
          const float* mp = mus + 16 * I + 4 * g;
          f[q][0] = mp[0], f[q][1] = mp[1], f[q][2] = mp[2], f[q][3] = mp[3];
          const float* ap = slab + (size_t)(16 * I + c16) * CP + 4 * g;
          f32x4 a[4], an[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) an[u] = u <= I ? *(const f32x4*)(ap + 16 * u) : zero4;
          for (int J0 = 0; J0 <= I; J0 += 4) {  // four column tiles a step, the next four in flight
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = an[u];
#pragma unroll
            for (int u = 0; u < 4; ++u) an[u] = J0 + 4 + u <= I ? *(const f32x4*)(ap + 16 * (J0 + 4 + u)) : zero4;
#pragma unroll
            for (int u = 0; u < 4; ++u)
              if (J0 + u <= I) {
                const float* br = zs + (16 * (J0 + u) + 4 * g) * LW_ZS + c16;
#pragma unroll
                for (int mm = 0; mm < 4; ++mm) f[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][mm], br[mm * LW_ZS], f[q], 0, 0, 0);
              }
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
      for (int q = 0; q < LW_MAXT; ++q) {
        const int I = lw_row_tile(q, wave);
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
      const int cnt = min(LW_NS, n - s0);
#pragma unroll
      for (int q = 0; q < LW_MAXT; ++q) {
        if (lw_row_tile(q, wave) < T) {  // (uniform per wave)
#pragma unroll
          for (int r = 0; r < 4; ++r) f[q][r] /= sum;
          for (int nn = 0; nn < cnt; ++nn) {  // the stage's columns in ascending s (every lane of a group ends with the same sums)
#pragma unroll
            for (int r = 0; r < 4; ++r) run[q][r] += __shfl(f[q][r], (lane & 48) + nn, 64);
          }
        }
      }
    }
    if (c16 == 0) {
#pragma unroll
      for (int q = 0; q < LW_MAXT; ++q) {
        const int I = lw_row_tile(q, wave);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int cls = 16 * I + 4 * g + r;
          if (cls < C) probs[b * C + cls] = run[q][r] / (float)n;
        }
      }
    }
    if (tid == 0) info[b] = 0;
  }
}

// ---- 1: mc with the marginal variances -------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void linkwide_mc_diag_kernel(const float* __restrict__ f_mu, const float* __restrict__ f_var,
                                                               const float* __restrict__ z, int C, int n, float* __restrict__ probs,
                                                               int* __restrict__ info) {
  __shared__ float red[2][16];
  const int t = threadIdx.x;
  const int64_t b = blockIdx.x;
  float mu[LW_NCL], sd[LW_NCL], run[LW_NCL];
#pragma unroll
  for (int q = 0; q < LW_NCL; ++q) {
    const int cls = t + 256 * q;
    mu[q] = cls < C ? f_mu[b * C + cls] : 0.f;
    sd[q] = cls < C ? sqrtf(f_var[b * C + cls]) : 0.f;
    run[q] = 0.f;
  }
  for (int s0 = 0; s0 < n; s0 += 4) {
    float x[LW_NCL][4];
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int q = 0; q < LW_NCL; ++q) {
      if (256 * q >= C) continue;  // (uniform)
      const int cls = t + 256 * q;
      float zz[4] = {0.f, 0.f, 0.f, 0.f};
      if (cls < C) {
        const float* zp = z + (int64_t)cls * n + s0;
        if constexpr (VEC) {
          ld<4>(zp, zz);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (s0 + e < n) zz[e] = zp[e];
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        x[q][e] = cls < C ? fmaf(sd[q], zz[e], mu[q]) : -INFINITY;
        m[e] = fmaxf(m[e], x[q][e]);
      }
    }
    lw_block_reduce<4, true>(m, red[0]);
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < LW_NCL; ++q) {
      if (256 * q >= C) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        x[q][e] = expf(x[q][e] - m[e]);  // (0 for a class beyond C)
        sum[e] += x[q][e];
      }
    }
    lw_block_reduce<4, false>(sum, red[1]);
#pragma unroll
    for (int q = 0; q < LW_NCL; ++q) {
      if (256 * q >= C) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (s0 + e < n) run[q] += x[q][e] / sum[e];  // ascending s
    }
  }
#pragma unroll
  for (int q = 0; q < LW_NCL; ++q) {
    const int cls = t + 256 * q;
    if (cls < C) probs[b * C + cls] = run[q] / (float)n;
  }
  if (t == 0) info[b] = 0;
}

// ---- 0: probit and the Laplace bridge ----------------------------------------------------------------------------------------------
// one pass over the C x C block of a sample: wave w takes rows w, w + 4, ...; lane l keeps the sums of columns l + 64 p
template <int NCOL>
__device__ __forceinline__ void lw_bridge_pass(const float* __restrict__ fv, int C, float* rowS, float* dgS, float* colP) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float cs[NCOL];
#pragma unroll
  for (int p = 0; p < NCOL; ++p) cs[p] = 0.f;
  for (int i = wave; i < C; i += 4) {
    const float* rp = fv + (int64_t)i * C;
    float rs = 0.f;
#pragma unroll
    for (int p = 0; p < NCOL; ++p) {
      const int j = lane + 64 * p;
      if (64 * p < C) {  // (uniform)
        const float v = j < C ? rp[j] : 0.f;
        cs[p] += v;
        rs += v;
        if (j == i) dgS[i] = v;
      }
    }
    rs = wave_sum(rs);
    if (lane == 0) rowS[i] = rs;
  }
#pragma unroll
  for (int p = 0; p < NCOL; ++p)
    if (lane + 64 * p < C) colP[wave * C + lane + 64 * p] = cs[p];
}

__global__ __launch_bounds__(256) void linkwide_stream_kernel(const float* __restrict__ f_mu, const float* __restrict__ f_var, int C,
                                                              int link, int diag, float c1, float rk, float* __restrict__ probs,
                                                              int* __restrict__ info) {
  extern __shared__ float lds[];  // bridge over the full covariance: rowS [C], dgS [C], colP [4][C]
  __shared__ float red[4];
  const int t = threadIdx.x;
  const int64_t b = blockIdx.x;
  float mu[LW_NCL], row[LW_NCL], col[LW_NCL], dg[LW_NCL];
#pragma unroll
  for (int q = 0; q < LW_NCL; ++q) {
    const int cls = t + 256 * q;
    mu[q] = cls < C ? f_mu[b * C + cls] : 0.f;
    row[q] = col[q] = dg[q] = 0.f;
  }
  if (diag) {
#pragma unroll
    for (int q = 0; q < LW_NCL; ++q) {
      const int cls = t + 256 * q;
      row[q] = col[q] = dg[q] = cls < C ? f_var[b * C + cls] : 0.f;
    }
  } else if (link == LK_LINK_PROBIT) {
#pragma unroll
    for (int q = 0; q < LW_NCL; ++q) {
      const int cls = t + 256 * q;
      dg[q] = cls < C ? f_var[b * C * C + (int64_t)cls * (C + 1)] : 0.f;
    }
  } else {
    float* rowS = lds;
    float* dgS = rowS + C;
    float* colP = dgS + C;
    const float* fv = f_var + b * C * C;
    if (C <= 1024) lw_bridge_pass<16>(fv, C, rowS, dgS, colP);
    else lw_bridge_pass<64>(fv, C, rowS, dgS, colP);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < LW_NCL; ++q) {
      const int cls = t + 256 * q;
      if (cls < C) {
        row[q] = rowS[cls];
        dg[q] = dgS[cls];
        col[q] = ((colP[cls] + colP[C + cls]) + colP[2 * C + cls]) + colP[3 * C + cls];
      }
    }
  }
  float out[LW_NCL];
  if (link == LK_LINK_PROBIT) {
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < LW_NCL; ++q) {
      out[q] = t + 256 * q < C ? (1.f / sqrtf(1.f + 0.39269908169872414f * dg[q])) * mu[q] : -INFINITY;  // pi / 8
      m = fmaxf(m, out[q]);
    }
    m = lw_block_reduce1<true>(m, red);
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < LW_NCL; ++q) {
      out[q] = expf(out[q] - m);
      s += out[q];
    }
    s = lw_block_reduce1<false>(s, red);
#pragma unroll
    for (int q = 0; q < LW_NCL; ++q) out[q] /= s;
  } else {
    const float K = (float)C;
    float smu = 0.f, tot = 0.f;
#pragma unroll
    for (int q = 0; q < LW_NCL; ++q) smu += mu[q], tot += row[q];
    smu = lw_block_reduce1<false>(smu, red);
    tot = lw_block_reduce1<false>(tot, red);
    float bm[LW_NCL], var[LW_NCL];
    float vs = 0.f;
#pragma unroll
    for (int q = 0; q < LW_NCL; ++q) {
      const bool own = t + 256 * q < C;
      bm[q] = mu[q] - row[q] * (smu / tot);
      var[q] = dg[q] - row[q] * col[q] / tot;
      vs += own ? var[q] : 0.f;
    }
    if (link == LK_LINK_BRIDGE_NORM) {
      const float scale = (lw_block_reduce1<false>(vs, red) / K) / rk;
#pragma unroll
      for (int q = 0; q < LW_NCL; ++q) {
        bm[q] = bm[q] / sqrtf(scale);
        var[q] = var[q] / scale;
      }
    }
    float sneg = 0.f;
#pragma unroll
    for (int q = 0; q < LW_NCL; ++q) sneg += t + 256 * q < C ? expf(-bm[q]) : 0.f;
    sneg = lw_block_reduce1<false>(sneg, red);
    float sa = 0.f;
#pragma unroll
    for (int q = 0; q < LW_NCL; ++q) {
      out[q] = (c1 + expf(bm[q]) / (K * K) * sneg) / var[q];
      sa += t + 256 * q < C ? out[q] : 0.f;
    }
    sa = lw_block_reduce1<false>(sa, red);
#pragma unroll
    for (int q = 0; q < LW_NCL; ++q) {
      float o = out[q] / sa;
      if (o != o) o = 1.f;  // torch.nan_to_num(nan=1.0): NaN -> 1, +-inf -> the largest finite values
      else if (o > FLT_MAX) o = FLT_MAX;
      else if (o < -FLT_MAX) o = -FLT_MAX;
      out[q] = o;
    }
  }
#pragma unroll
  for (int q = 0; q < LW_NCL; ++q) {
    const int cls = t + 256 * q;
    if (cls < C) probs[b * C + cls] = out[q];
  }
  if (t == 0) info[b] = 0;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
// 0 streaming (probit, bridge), 1 mc with the marginal variances, 2 mc with the full covariance; negative: outside the contract
static int linkwide_regime(int64_t B, int64_t C, int64_t n, int link, int diag) {
  if (link < 0 || link > 3 || C < LW_MIN_C || C > LW_MAX_C || B < 0 || B >= (1ll << 31)) return -1;
  if (link != LK_LINK_MC) return 0;
  if (n < 1 || n >= (1ll << 20)) return -1;
  if (diag) return 1;
  return C <= LW_MAX_C_FULL ? 2 : -1;
}

static inline int64_t linkwide_slab_bytes(int64_t C) {
  const int64_t CP = (C + 31) / 32 * 32;
  return CP * CP * (int64_t)sizeof(float);
}

static int linkwide_check(const float* f_mu, const float* f_var, const float* z, int64_t B, int64_t C, int64_t n, int link, int diag,
                          const float* probs, const int32_t* info, const void* work, int64_t work_bytes) {
  LK_REQUIRE(link >= 0 && link <= 3, "lk_glm_link_wide_f32: link must be 0 (probit), 1 (mc), 2 (bridge) or 3 (bridge_norm), got %d",
             link);
  LK_REQUIRE(f_mu && f_var && probs && info && (z || link != LK_LINK_MC), "lk_glm_link_wide_f32: null pointer");
  LK_REQUIRE(C >= LW_MIN_C, "lk_glm_link_wide_f32: C = %lld is not above LK_LINK_MAX_C = %d: lk_glm_link_f32 serves that range",
             (long long)C, LK_LINK_MAX_C);
  const bool full = link == LK_LINK_MC && !diag;
  LK_REQUIRE(C <= LW_MAX_C, "lk_glm_link_wide_f32: C = %lld above LK_LINK_WIDE_MAX_C = %d", (long long)C, LW_MAX_C);
  LK_REQUIRE(!full || C <= LW_MAX_C_FULL,
             "lk_glm_link_wide_f32: C = %lld above LK_LINK_WIDE_MAX_C_FULL = %d (mc with the full covariance: one workgroup factors "
             "one sample)", (long long)C, LW_MAX_C_FULL);
  LK_REQUIRE(B >= 0 && B < (1ll << 31), "lk_glm_link_wide_f32: B out of range (0 <= B < 2^31)");
  LK_REQUIRE(link != LK_LINK_MC || (n >= 1 && n < (1ll << 20)),
             "lk_glm_link_wide_f32: n_samples out of range (1 <= n_samples < 2^20)");
  const float* zz = link == LK_LINK_MC ? z : nullptr;
  LK_REQUIRE((((uintptr_t)f_mu | (uintptr_t)f_var | (uintptr_t)zz | (uintptr_t)probs | (uintptr_t)info) & 15) == 0,
             "lk_glm_link_wide_f32: pointers must be 16-byte aligned");
  const unsigned __int128 bc = (unsigned __int128)B * C * 4, ib = (unsigned __int128)B * 4;
  const unsigned __int128 in_bytes[3] = {bc, diag ? bc : bc * C, zz ? (unsigned __int128)C * n * 4 : 0};
  const void* in[3] = {f_mu, f_var, zz};
  for (int k = 0; k < 3; ++k)
    LK_REQUIRE(disjoint(probs, bc, in[k], in_bytes[k]) && disjoint(info, ib, in[k], in_bytes[k]),
               "lk_glm_link_wide_f32: an output overlaps an input");
  LK_REQUIRE(disjoint(probs, bc, info, ib), "lk_glm_link_wide_f32: probs overlaps info");
  if (full && B > 0) {  // (an empty batch needs no workspace)
    const int64_t slab = linkwide_slab_bytes(C);
    LK_REQUIRE(work != nullptr, "lk_glm_link_wide_f32: null workspace (mc with the full covariance keeps L in it)");
    LK_REQUIRE(((uintptr_t)work & 15) == 0, "lk_glm_link_wide_f32: the workspace must be 16-byte aligned");
    LK_REQUIRE(work_bytes >= slab, "lk_glm_link_wide_f32: a workspace of %lld bytes holds no slab of %lld bytes (CP * CP floats)",
               (long long)work_bytes, (long long)slab);
    const int64_t have = work_bytes / slab;
    const unsigned __int128 wb = (unsigned __int128)(have < B ? have : (B > 0 ? B : 1)) * slab;  // the slabs the call uses
    for (int k = 0; k < 3; ++k)
      LK_REQUIRE(disjoint(work, wb, in[k], in_bytes[k]), "lk_glm_link_wide_f32: the workspace overlaps an input");
    LK_REQUIRE(disjoint(work, wb, probs, bc) && disjoint(work, wb, info, ib), "lk_glm_link_wide_f32: the workspace overlaps an output");
  }
  return LK_OK;
}

template <typename Kern>
static void linkwide_allow_lds(Kern kern, size_t bytes) {  // (every launch: the attribute belongs to the current device)
  if (bytes > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace lk

using namespace lk;

extern "C" int lk_glm_link_wide_f32(const float* f_mu, const float* f_var, const float* z, int64_t B, int64_t C, int64_t n_samples,
                                    int link, int diag, float* probs, int32_t* info, void* work, int64_t work_bytes, void* stream) {
  const int rc = linkwide_check(f_mu, f_var, z, B, C, n_samples, link, diag, probs, info, work, work_bytes);
  if (rc != LK_OK) return rc;
  if (B == 0) return LK_OK;
  hipStream_t st = (hipStream_t)stream;
  const int regime = linkwide_regime(B, C, n_samples, link, diag), dg = diag != 0;
  if (regime == 0) {
    const float c1 = (float)(1.0 - 2.0 / (double)C), rk = (float)sqrt((double)C / 2.0);
    const size_t lds = (link != LK_LINK_PROBIT && !dg) ? (size_t)6 * C * sizeof(float) : 0;
    linkwide_allow_lds(linkwide_stream_kernel, lds);
    hipLaunchKernelGGL(linkwide_stream_kernel, dim3((unsigned)B), dim3(256), lds, st, f_mu, f_var, (int)C, link, dg, c1, rk, probs,
                       info);
    return check_launch("linkwide_stream_kernel");
  }
  if (regime == 1) {
    if (n_samples % 4 == 0)
      hipLaunchKernelGGL(linkwide_mc_diag_kernel<true>, dim3((unsigned)B), dim3(256), 0, st, f_mu, f_var, z, (int)C, (int)n_samples,
                         probs, info);
    else
      hipLaunchKernelGGL(linkwide_mc_diag_kernel<false>, dim3((unsigned)B), dim3(256), 0, st, f_mu, f_var, z, (int)C, (int)n_samples,
                         probs, info);
    return check_launch("linkwide_mc_diag_kernel");
  }
  const int64_t have = work_bytes / linkwide_slab_bytes(C), slots = have < B ? have : B;
  const size_t lds = lw_full_lds((C + 31) / 32 * 32);
  hipLaunchKernelGGL(linkwide_mc_full_kernel, dim3((unsigned)slots), dim3(256), lds, st, f_mu, f_var, z, B, (int)C, (int)n_samples,
                     probs, info, (float*)work);
  return check_launch("linkwide_mc_full_kernel");
}

extern "C" int64_t lk_glm_link_wide_work_bytes(int64_t B, int64_t C, int link, int diag) {
  if (linkwide_regime(B, C, 1, link, diag) != 2 || B < 1) return 0;
  return (B < LW_MAX_SLOTS ? B : LW_MAX_SLOTS) * linkwide_slab_bytes(C);
}

extern "C" int lk_glm_link_wide_variant(int64_t B, int64_t C, int64_t n_samples, int link, int diag) {
  return linkwide_regime(B, C, n_samples, link, diag);
}
