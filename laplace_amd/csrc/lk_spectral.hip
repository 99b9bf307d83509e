// Dense (full-covariance) Laplace in the eigenbasis of the curvature:  H = Q diag(lam) Q^T  is decomposed once, and for a scalar
// prior precision delta the posterior precision is  Q diag(mu) Q^T,  mu_j = hfac lam_j + delta.  With R = J Q (delta-free)
//   COV   fvar[n][c][k] = sum_j R[n][c][j] R[n][k][j] / (hfac lam_j + delta)             (FullLaplace.functional_variance,
//                                                                                         laplace/baselaplace.py:1683-1684)
//   GRID  var[g][n][c] += sum_j R[n][c][j]^2 / (hfac lam_j + deltas[g])                  (the diagonal at G prior precisions: the
//                                                                                         grid search of baselaplace.py:487-561)
// so a change of the prior costs no factorisation and a grid of G priors one pass.  One tile kernel, two loaders, two epilogues.
//
// Tile: SP_TN = 32 samples x SP_TJ = 128 eigen-columns per workgroup of 4 waves; wave w owns columns 32 w .. 32 w + 31 of the
// tile.  The accumulators of v_mfma_f32_32x32x2_f32 hold, per output c, the 32 x 32 block with the eigen-columns along the ROWS
// and the samples along the COLUMNS: lane (lo, hi) owns sample n0 + lo and the 16 columns j = (r & 3) + 8 (r >> 2) + 4 hi.  The
// sum over j of a sample is then a sum over a lane's own registers, the two halves of the wave, the four waves and the column
// tiles - the class-accumulator / pair-sum structure of lk_quadconv.hip with a sample per lane.
//   * LL loader (last layer, J = I (x) [phi, 1]; neither J nor R reaches memory):  R[n][c][j] = sum_d phi[n][d] Q[c D + d][j]
//     (+ Q[C D + c][j]).  phi of the 32 samples is staged once per workgroup in LDS ([d][33], zero-padded: the B operand); the
//     A operand is the [D][32] panel of Q for output c read where it lies in the row-major Q (reference parameter order: weight
//     [C][D], then bias), 128 contiguous bytes per half-wave, SP_KU k-steps in flight.  The bias row is added to the finished sum.
//   * R loader (full-network posteriors): R [N][C][P] = Js Q is given (one lk_gemm_f32) and read into the same layout.
//   * COV epilogue: the CT (CT + 1) / 2 pair sums of a lane's sample stay in registers across the workgroup's column tiles; at
//     the end the halves meet by one shuffle, the waves in LDS, in a fixed order.  More than 10 outputs: blocks of 5, one launch
//     per block pair (10 accumulators); a diagonal block is written by exactly one of the launches that see it.
//   * GRID epilogue (the grid walk of lk_grid.hip): chunks of GC grid points, one reciprocal per (column, grid point) shared by
//     the CT outputs held (GC x CT <= 64 running sums per lane), reduced as above per chunk and added to the workgroup's OWN
//     slice of the workspace (same thread, same address: no hazard).  Any C: blocks of outputs are independent launches.
// A workgroup owns (sample tile, a contiguous range of column tiles); the ranges' partial sums go to the workspace and a second
// kernel adds them in ascending order and writes fvar (both triangles from one value: exactly symmetric) or adds to var.
// One owner per output element, no float atomics, fixed summation order: two runs give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lk_stream.h"
#include "lk_quadtile.h"

namespace lk {

constexpr int SP_TN = LK_SP_TILE_N;   // samples per tile
constexpr int SP_TJ = LK_SP_TILE_J;   // eigen-columns per tile
constexpr int SP_KU = 4;              // k-steps (two d each) of Q in flight
constexpr int SP_PAD = 33;            // row pitch of the staged phi in LDS
constexpr int SP_GMAX = 128;          // grid points per launch (the host walks larger grids in pieces)
constexpr int SP_DMAX = 896;          // LL: features whose staged tile fits LDS beside the reduction scratch
constexpr int64_t SP_PMAX = 32768;    // the eigensolver's limit
constexpr int SP_WANT_BLOCKS = 512;   // workgroups wanted before the column range stops being split

struct SpClasses {  // accumulator slot c holds output  c < na ? a0 + c : b0 + c - na
  int a0, na, b0, nb;
};

template <int CT>
struct SpCfg {
  static constexpr int NP = CT * (CT + 1) / 2;                // pair sums (COV)
  static constexpr int GC = CT == 10 ? 5 : 64 / CT;           // grid points per chunk (GRID), as GridCfg
  static constexpr int V = GC * CT;
  static constexpr int SCRATCH_COV = 4 * NP * SP_TN * 4;      // bytes: [4 waves][NP][32]
  static constexpr int SCRATCH_GRID = 4 * V * SP_TN * 4;      // bytes: [4 waves][V][32]
};

__host__ __device__ static inline int sp_dpad(int64_t D) { return (int)((D + 2 * SP_KU - 1) / (2 * SP_KU) * (2 * SP_KU)); }

template <int CT, bool LL, bool GRID>
__global__ __launch_bounds__(256) void spectral_kernel(const float* __restrict__ X, const float* __restrict__ Q,
                                                       const float* __restrict__ lam, float hfac,
                                                       const float* __restrict__ deltas, int G, int B, int C, int D, int P,
                                                       int has_bias, SpClasses cls, int split, int tiles_per, int ntj,
                                                       float* __restrict__ partial) {
  using Cfg = SpCfg<CT>;
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  const int Dp = LL ? sp_dpad(D) : 0;
  float* const sPhi = dyn;                  // [Dp][SP_PAD]
  float* const sc = dyn + Dp * SP_PAD;      // reduction scratch
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lo = lane & 31, hi = lane >> 5;
  const int tn = blockIdx.x / split, sp = blockIdx.x - tn * split;
  const int n0 = tn * SP_TN;
  const int ncls = cls.na + cls.nb;
  const int t_begin = sp * tiles_per, t_end = t_begin + tiles_per < ntj ? t_begin + tiles_per : ntj;

  if constexpr (LL) {
    for (int e = tid; e < Dp * SP_TN; e += 256) {
      const int n = e / Dp, d = e - n * Dp;
      sPhi[d * SP_PAD + n] = (n0 + n < B && d < D) ? X[(size_t)(n0 + n) * D + d] : 0.f;
    }
    __syncthreads();
  }

  float s[GRID ? 1 : Cfg::NP];
  if constexpr (!GRID) {
#pragma unroll
    for (int e = 0; e < Cfg::NP; ++e) s[e] = 0.f;
  }

  for (int t = t_begin; t < t_end; ++t) {
    const int jw = t * SP_TJ + wave * 32;
    f32x16 acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

    if constexpr (LL) {
      const bool jok = jw + lo < P;
      const size_t jcol = jok ? jw + lo : 0;
      const int nk = Dp / 2;
      // an empty slot (the last block of a C that is no multiple of the block) repeats the last output: no branch in the K loop,
      // and what it accumulates is never stored
      size_t crow[CT];
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        const int cs = c < ncls ? c : ncls - 1;
        crow[c] = (size_t)(cs < cls.na ? cls.a0 + cs : cls.b0 + cs - cls.na) * D;
      }
      float an[SP_KU][CT];
      auto fetch = [&](int k0) {
#pragma unroll
        for (int u = 0; u < SP_KU; ++u) {
          const int d = 2 * (k0 + u) + hi;
          const bool ok = jok && d < D;
          const size_t dd = ok ? d : 0;
#pragma unroll
          for (int c = 0; c < CT; ++c) {
            const float q = Q[(crow[c] + dd) * P + jcol];
            an[u][c] = ok ? q : 0.f;
          }
        }
      };
      fetch(0);
      for (int k0 = 0; k0 < nk; k0 += SP_KU) {
        float ac[SP_KU][CT];
#pragma unroll
        for (int u = 0; u < SP_KU; ++u)
#pragma unroll
          for (int c = 0; c < CT; ++c) ac[u][c] = an[u][c];
        if (k0 + SP_KU < nk) fetch(k0 + SP_KU);
#pragma unroll
        for (int u = 0; u < SP_KU; ++u) {
          const float b = sPhi[(2 * (k0 + u) + hi) * SP_PAD + lo];
#pragma unroll
          for (int c = 0; c < CT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[u][c], b, acc[c], 0, 0, 0);
        }
      }
      if (has_bias) {
#pragma unroll
        for (int c = 0; c < CT; ++c)
          if (c < ncls) {
            const size_t cc = c < cls.na ? cls.a0 + c : cls.b0 + c - cls.na;
            const float* qb = Q + ((size_t)C * D + cc) * P;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int j = jw + (r & 3) + 8 * (r >> 2) + 4 * hi;
              acc[c][r] += j < P ? qb[j] : 0.f;
            }
          }
      }
    } else {
      const bool nok = n0 + lo < B;
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < ncls) {
          const size_t cc = c < cls.na ? cls.a0 + c : cls.b0 + c - cls.na;
          const float* rr = X + ((size_t)(nok ? n0 + lo : 0) * C + cc) * P;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int j = jw + (r & 3) + 8 * (r >> 2) + 4 * hi;
            const bool ok = nok && j < P;
            const float v = rr[ok ? j : 0];
            acc[c][r] = ok ? v : 0.f;
          }
        }
    }

    // the delta-free part of this lane's 16 weights
    float base[16];
    bool ok[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = jw + (r & 3) + 8 * (r >> 2) + 4 * hi;
      ok[r] = j < P;
      base[r] = hfac * lam[ok[r] ? j : 0];
    }

    if constexpr (!GRID) {
      const float delta = deltas[0];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float w = ok[r] ? __builtin_amdgcn_rcpf(base[r] + delta) : 0.f;
        int e = 0;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
          const float tc = acc[c][r] * w;
#pragma unroll
          for (int k = c; k < CT; ++k) s[e++] += tc * acc[k][r];
        }
      }
    } else {
      constexpr int GC = Cfg::GC, V = Cfg::V;
      float* const pw = partial + (size_t)blockIdx.x * G * CT * SP_TN;
      for (int g0 = 0; g0 < G; g0 += GC) {
        float dq[GC];
#pragma unroll
        for (int gc = 0; gc < GC; ++gc) dq[gc] = deltas[g0 + gc < G ? g0 + gc : G - 1];
        float part[V];
#pragma unroll
        for (int e = 0; e < V; ++e) part[e] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float sq[CT];
#pragma unroll
          for (int c = 0; c < CT; ++c) sq[c] = acc[c][r] * acc[c][r];
#pragma unroll
          for (int gc = 0; gc < GC; ++gc) {
            const float w = ok[r] ? __builtin_amdgcn_rcpf(base[r] + dq[gc]) : 0.f;
#pragma unroll
            for (int c = 0; c < CT; ++c) part[gc * CT + c] += w * sq[c];
          }
        }
        // the two halves of the wave by a shuffle, the four waves in LDS, then this thread's own words of the slice
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float o = __shfl_xor(part[e], 32, 64);
          if (hi == 0) sc[(wave * V + e) * SP_TN + lo] = part[e] + o;
        }
        __syncthreads();
        for (int idx = tid; idx < V * SP_TN; idx += 256) {
          if (g0 + idx / (CT * SP_TN) >= G) break;
          const float v = (sc[idx] + sc[V * SP_TN + idx]) + (sc[2 * V * SP_TN + idx] + sc[3 * V * SP_TN + idx]);
          float* dst = pw + (size_t)g0 * CT * SP_TN + idx;
          *dst = t == t_begin ? v : *dst + v;
        }
        __syncthreads();
      }
    }
  }

  if constexpr (!GRID) {
    constexpr int NP = Cfg::NP;
#pragma unroll
    for (int e = 0; e < NP; ++e) {
      const float o = __shfl_xor(s[e], 32, 64);
      if (hi == 0) sc[(wave * NP + e) * SP_TN + lo] = s[e] + o;
    }
    __syncthreads();
    float* const pw = partial + (size_t)blockIdx.x * NP * SP_TN;
    for (int idx = tid; idx < NP * SP_TN; idx += 256)
      pw[idx] = (sc[idx] + sc[NP * SP_TN + idx]) + (sc[2 * NP * SP_TN + idx] + sc[3 * NP * SP_TN + idx]);
  }
}

// fvar[n][c][k] = fvar[n][k][c] = the sum over the column ranges, in ascending order; pairs this launch does not own are skipped
__global__ __launch_bounds__(256) void spectral_cov_reduce_kernel(const float* __restrict__ partial, int64_t B, int C, int CT,
                                                                  SpClasses cls, int own_a, int own_b, int split,
                                                                  float* __restrict__ fvar) {
  const int NP = CT * (CT + 1) / 2;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= B * NP) return;
  const int64_t n = e / NP;
  int p = (int)(e - n * NP), c = 0;
  while (p >= CT - c) p -= CT - c, ++c;
  const int k = c + p;
  if (k >= cls.na + cls.nb) return;
  const bool in_a = k < cls.na, in_b = c >= cls.na;
  if ((in_a && !own_a) || (in_b && !own_b)) return;
  const int64_t tn = n / SP_TN;
  const int nl = (int)(n - tn * SP_TN), pe = (int)(e - n * NP);
  float sum = 0.f;
  for (int sp = 0; sp < split; ++sp) sum += partial[((size_t)(tn * split + sp) * NP + pe) * SP_TN + nl];
  const int64_t cc = c < cls.na ? cls.a0 + c : cls.b0 + c - cls.na, kk = k < cls.na ? cls.a0 + k : cls.b0 + k - cls.na;
  fvar[(n * C + cc) * C + kk] = sum;
  fvar[(n * C + kk) * C + cc] = sum;
}

// var[g0 + g][n][c0 + c] += the sum over the column ranges, in ascending order
__global__ __launch_bounds__(256) void spectral_grid_reduce_kernel(const float* __restrict__ partial, int64_t B, int G, int CT,
                                                                   int Cl, int split, int64_t g0, int64_t Ctot, int64_t c0,
                                                                   float* __restrict__ var) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= B * G * Cl) return;
  const int64_t n = e / (G * Cl);
  const int r = (int)(e - n * G * Cl), g = r / Cl, c = r - g * Cl;
  const int64_t tn = n / SP_TN;
  const int nl = (int)(n - tn * SP_TN);
  float sum = 0.f;
  for (int sp = 0; sp < split; ++sp) sum += partial[(((size_t)(tn * split + sp) * G + g) * CT + c) * SP_TN + nl];
  var[((g0 + g) * B + n) * Ctot + c0 + c] += sum;
}

// ---- host: the plan of a shape (the ONE copy of the rules: the launchers, the workspace size and lk_spectral_variant) ----------
struct SpPlan {
  int ll, grid, ct, pairs, gc;
  int64_t P, ntn, ntj, tiles_per, split;
  size_t lds, ws;
};

static bool sp_plan(int form, int64_t N, int64_t C, int64_t DP, int64_t G, SpPlan* p) {
  const int base = form & 3, bias = (form & LK_SP_BIAS) ? 1 : 0;
  if (form < 0 || form > 7 || N < 1 || C < 1 || DP < 1 || G < 1 || C >= (1ll << 15) || N >= (1ll << 24) || G >= (1ll << 20))
    return false;
  p->ll = base == LK_SP_QUAD_LL || base == LK_SP_GRID_LL;
  p->grid = base == LK_SP_GRID_LL || base == LK_SP_GRID_R;
  if (!p->ll && bias) return false;
  if (p->ll && DP > SP_DMAX) return false;
  p->P = p->ll ? C * DP + (bias ? C : 0) : DP;
  if (p->P > SP_PMAX) return false;
  p->pairs = !p->grid && C > 10;
  p->ct = p->pairs ? 10 : grid_class_tile(C);
  p->gc = p->ct == 10 ? 5 : 64 / p->ct;
  p->ntn = (N + SP_TN - 1) / SP_TN;
  p->ntj = (p->P + SP_TJ - 1) / SP_TJ;
  int64_t want = (SP_WANT_BLOCKS + p->ntn - 1) / p->ntn;
  if (want > p->ntj) want = p->ntj;
  p->tiles_per = (p->ntj + want - 1) / want;
  p->split = (p->ntj + p->tiles_per - 1) / p->tiles_per;
  const int np = p->ct * (p->ct + 1) / 2, v = p->gc * p->ct;
  p->lds = (p->ll ? (size_t)sp_dpad(DP) * SP_PAD * 4 : 0) + (size_t)4 * (p->grid ? v : np) * SP_TN * 4;
  const int64_t gl = G < SP_GMAX ? G : SP_GMAX;
  p->ws = (size_t)(p->ntn * p->split) * SP_TN * sizeof(float) * (p->grid ? (size_t)gl * p->ct : (size_t)np);
  return true;
}

// the whole contract of the four entry points, with the messages under the caller's name
static int spectral_check_args(const char* fn, int form, const float* X, const float* Q, const float* lam, float hfac,
                               const float* deltas, int64_t G, int64_t N, int64_t C, int64_t DP, const float* out,
                               const void* ws, size_t ws_bytes, SpPlan* p) {
  const bool ll = (form & 3) == LK_SP_QUAD_LL || (form & 3) == LK_SP_GRID_LL;
  LK_REQUIRE(X && lam && deltas && out && (Q || !ll), "%s: null pointer (%s, lam, %s, %s)", fn, ll ? "phi, Q" : "R",
             G < 0 ? "delta" : "deltas", G < 0 ? "fvar" : "var");
  if (G < 0) G = 1;  // (the COV entry points: one device scalar)
  LK_REQUIRE(N >= 0 && N < (1ll << 24) && C >= 1 && C < (1ll << 15) && G >= 1 && G < (1ll << 20),
             "%s: extent out of range (0 <= %s < 2^24, 1 <= C < 2^15, 1 <= G < 2^20)", fn, ll ? "B" : "N");
  if (ll) {
    LK_REQUIRE(DP >= 1 && DP <= SP_DMAX, "%s: D out of range (1 <= D <= %d: the staged features of a tile fit LDS)", fn, SP_DMAX);
    LK_REQUIRE(C * DP + ((form & LK_SP_BIAS) ? C : 0) <= SP_PMAX, "%s: P = C D (+ C) out of range (P <= 32768, the eigensolver's limit)", fn);
  } else {
    LK_REQUIRE(DP >= 1 && DP <= SP_PMAX, "%s: P out of range (1 <= P <= 32768, the eigensolver's limit)", fn);
  }
  LK_REQUIRE(hfac > 0.f && hfac < INFINITY, "%s: hfac must be positive and finite", fn);
  if (N == 0) return LK_OK;
  if (!sp_plan(form, N, C, DP, G, p)) {
    set_error("%s: no launch form for this shape", fn);
    return LK_EINVAL;
  }
  if (ws == nullptr || ws_bytes < p->ws) {
    set_error("%s: workspace too small (%zu bytes needed)", fn, p->ws);
    return LK_EWORKSPACE;
  }
  const unsigned __int128 ob = (unsigned __int128)N * C * 4 * (p->grid ? (unsigned __int128)G : (unsigned __int128)C);
  const unsigned __int128 xb = ll ? (unsigned __int128)N * DP * 4 : (unsigned __int128)N * C * p->P * 4;
  bool clear = disjoint(out, ob, X, xb) && disjoint(out, ob, lam, (unsigned __int128)p->P * 4) &&
               disjoint(out, ob, deltas, (unsigned __int128)G * 4) && disjoint(out, ob, ws, p->ws);
  if (ll) clear = clear && disjoint(out, ob, Q, (unsigned __int128)p->P * p->P * 4);
  LK_REQUIRE(clear, "%s: the output overlaps an input or the workspace", fn);
  return LK_OK;
}

template <int CT, bool LL, bool GRID>
static int spectral_launch_one(const SpPlan& p, const float* X, const float* Q, const float* lam, float hfac, const float* deltas,
                               int G, int64_t N, int64_t C, int64_t DP, int has_bias, SpClasses cls, float* partial,
                               hipStream_t st) {
  if (p.lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&spectral_kernel<CT, LL, GRID>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
    if (e != hipSuccess) {
      set_error("spectral_kernel: cannot raise dynamic LDS limit: %s", hipGetErrorString(e));
      return LK_ELAUNCH;
    }
  }
  hipLaunchKernelGGL((spectral_kernel<CT, LL, GRID>), dim3((unsigned)(p.ntn * p.split)), dim3(256), p.lds, st, X, Q, lam, hfac,
                     deltas, G, (int)N, (int)C, (int)(LL ? DP : 0), (int)p.P, has_bias, cls, (int)p.split, (int)p.tiles_per,
                     (int)p.ntj, partial);
  return LK_OK;
}

template <bool LL, bool GRID>
static int spectral_launch_ct(const SpPlan& p, const float* X, const float* Q, const float* lam, float hfac, const float* deltas,
                              int G, int64_t N, int64_t C, int64_t DP, int has_bias, SpClasses cls, float* partial,
                              hipStream_t st) {
  switch (p.ct) {
    case 1: return spectral_launch_one<1, LL, GRID>(p, X, Q, lam, hfac, deltas, G, N, C, DP, has_bias, cls, partial, st);
    case 2: return spectral_launch_one<2, LL, GRID>(p, X, Q, lam, hfac, deltas, G, N, C, DP, has_bias, cls, partial, st);
    case 5: return spectral_launch_one<5, LL, GRID>(p, X, Q, lam, hfac, deltas, G, N, C, DP, has_bias, cls, partial, st);
    default: return spectral_launch_one<10, LL, GRID>(p, X, Q, lam, hfac, deltas, G, N, C, DP, has_bias, cls, partial, st);
  }
}

template <bool LL>
static int spectral_run_cov(const SpPlan& p, const float* X, const float* Q, const float* lam, float hfac, const float* delta,
                            int64_t N, int64_t C, int64_t DP, int has_bias, float* fvar, void* ws, hipStream_t st) {
  float* partial = static_cast<float*>(ws);
  const int np = p.ct * (p.ct + 1) / 2;
  const unsigned rblocks = (unsigned)((N * np + 255) / 256);
  auto one = [&](SpClasses cls, int own_a, int own_b) {
    const int rc = spectral_launch_ct<LL, false>(p, X, Q, lam, hfac, delta, 1, N, C, DP, has_bias, cls, partial, st);
    if (rc != LK_OK) return rc;
    hipLaunchKernelGGL(spectral_cov_reduce_kernel, dim3(rblocks), dim3(256), 0, st, partial, N, (int)C, p.ct, cls, own_a, own_b,
                       (int)p.split, fvar);
    return LK_OK;
  };
  if (!p.pairs) {
    const int rc = one(SpClasses{0, (int)C, 0, 0}, 1, 1);
    if (rc != LK_OK) return rc;
  } else {
    const int nb5 = (int)((C + 4) / 5);  // (>= 3)
    for (int I = 0; I < nb5; ++I)
      for (int J = I + 1; J < nb5; ++J) {
        const int na = 5, nb = (int)(C - 5 * J < 5 ? C - 5 * J : 5);
        const int rc = one(SpClasses{5 * I, na, 5 * J, nb}, J == I + 1, J == nb5 - 1 && I == nb5 - 2);
        if (rc != LK_OK) return rc;
      }
  }
  return check_launch("spectral_kernel");
}

template <bool LL>
static int spectral_run_grid(const SpPlan& p, const float* X, const float* Q, const float* lam, float hfac, const float* deltas,
                             int64_t G, int64_t N, int64_t C, int64_t DP, int has_bias, float* var, void* ws, hipStream_t st) {
  float* partial = static_cast<float*>(ws);
  for (int64_t c0 = 0; c0 < C; c0 += p.ct) {
    const int cl = (int)(C - c0 < p.ct ? C - c0 : p.ct);
    for (int64_t g0 = 0; g0 < G; g0 += SP_GMAX) {
      const int gl = (int)(G - g0 < SP_GMAX ? G - g0 : SP_GMAX);
      const int rc = spectral_launch_ct<LL, true>(p, X, Q, lam, hfac, deltas + g0, gl, N, C, DP, has_bias,
                                                  SpClasses{(int)c0, cl, 0, 0}, partial, st);
      if (rc != LK_OK) return rc;
      const int64_t total = N * gl * cl;
      hipLaunchKernelGGL(spectral_grid_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, partial, N, gl,
                         p.ct, cl, (int)p.split, g0, C, c0, var);
    }
  }
  return check_launch("spectral_kernel");
}

}  // namespace lk

using namespace lk;

extern "C" size_t lk_spectral_workspace_bytes(int form, int64_t N, int64_t C, int64_t D_or_P, int64_t G) {
  SpPlan p;
  return sp_plan(form, N, C, D_or_P, G, &p) ? p.ws : 0;
}

extern "C" int lk_spectral_quadform_ll_f32(const float* phi, const float* Q, const float* lam, float hfac, const float* delta,
                                           int64_t B, int64_t C, int64_t D, int has_bias, float* fvar, void* ws, size_t ws_bytes,
                                           void* stream) {
  SpPlan p;
  const int form = LK_SP_QUAD_LL | (has_bias ? LK_SP_BIAS : 0);
  const int rc = spectral_check_args("lk_spectral_quadform_ll_f32", form, phi, Q, lam, hfac, delta, -1, B, C, D, fvar, ws, ws_bytes, &p);
  if (rc != LK_OK || B == 0) return rc;
  return spectral_run_cov<true>(p, phi, Q, lam, hfac, delta, B, C, D, has_bias ? 1 : 0, fvar, ws, (hipStream_t)stream);
}

extern "C" int lk_spectral_grid_ll_f32(const float* phi, const float* Q, const float* lam, float hfac, const float* deltas,
                                       int64_t G, int64_t B, int64_t C, int64_t D, int has_bias, float* var, void* ws,
                                       size_t ws_bytes, void* stream) {
  SpPlan p;
  const int form = LK_SP_GRID_LL | (has_bias ? LK_SP_BIAS : 0);
  const int rc = spectral_check_args("lk_spectral_grid_ll_f32", form, phi, Q, lam, hfac, deltas, G < 0 ? 0 : G, B, C, D, var, ws, ws_bytes, &p);
  if (rc != LK_OK || B == 0) return rc;
  return spectral_run_grid<true>(p, phi, Q, lam, hfac, deltas, G, B, C, D, has_bias ? 1 : 0, var, ws, (hipStream_t)stream);
}

extern "C" int lk_spectral_quadform_f32(const float* R, const float* lam, float hfac, const float* delta, int64_t N, int64_t C,
                                        int64_t P, float* fvar, void* ws, size_t ws_bytes, void* stream) {
  SpPlan p;
  const int rc = spectral_check_args("lk_spectral_quadform_f32", LK_SP_QUAD_R, R, nullptr, lam, hfac, delta, -1, N, C, P, fvar, ws, ws_bytes, &p);
  if (rc != LK_OK || N == 0) return rc;
  return spectral_run_cov<false>(p, R, nullptr, lam, hfac, delta, N, C, P, 0, fvar, ws, (hipStream_t)stream);
}

extern "C" int lk_spectral_grid_f32(const float* R, const float* lam, float hfac, const float* deltas, int64_t G, int64_t N,
                                    int64_t C, int64_t P, float* var, void* ws, size_t ws_bytes, void* stream) {
  SpPlan p;
  const int rc = spectral_check_args("lk_spectral_grid_f32", LK_SP_GRID_R, R, nullptr, lam, hfac, deltas, G < 0 ? 0 : G, N, C, P, var, ws, ws_bytes, &p);
  if (rc != LK_OK || N == 0) return rc;
  return spectral_run_grid<false>(p, R, nullptr, lam, hfac, deltas, G, N, C, P, 0, var, ws, (hipStream_t)stream);
}

// CT | grid << 4 | block pairs << 5 | LL loader << 6 | split > 1 << 7 | split << 8 (12 bits) | GC << 20; `aligned` is ignored:
// every form reads single dwords
extern "C" int lk_spectral_variant(int form, int64_t N, int64_t C, int64_t D_or_P, int64_t G, int aligned) {
  (void)aligned;
  SpPlan p;
  if (!sp_plan(form, N, C, D_or_P, G, &p) || p.split >= 4096) return -1;
  return p.ct | p.grid << 4 | p.pairs << 5 | p.ll << 6 | (p.split > 1 ? 1 : 0) << 7 | (int)p.split << 8 | p.gc << 20;
}
