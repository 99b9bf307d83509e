// Per-output GLM predictive variances (the DIAGONAL of f_var) for any number of outputs, without the Jacobian and without
// the [B, C, C] block: what `diagonal_output=True` asks for, and all the probit link reads.
//
// Weight-sharing layers (Conv2d, Linear along a sequence):
//   fvar_diag[n][c] += sum_{o,i} (sum_l u[n,c,o,l] v[n,i,l])^2 w[o,i]
// The pair-sum kernel of lk_quadconv.hip keeps one accumulator tile per output for a whole super-tile because every PAIR of
// outputs meets in the epilogue; that is what bounds it to ten outputs.  The diagonal has no pair structure: an output's
// weighted tile is squared, summed to ONE number and forgotten.  So here the outputs go by in chunks of QD_CT through the
// same tile products (lk_quadtile.h), the running sums live in an LDS array [C] per wave (no registers per output — that
// array, 16 KiB per wave, is the only bound on C), and what is the same for every chunk of a super-tile is formed once:
// the weights of the lane's 16 (o, i) positions (registers) and the v panel of the 128 columns (LDS, while it fits).
//
// Plain Linear layers: fvar_diag[n][c] += sum_o u[c][n][o]^2 s[n][o],  s[n][o] = sum_i v[n][i]^2 w[o,i]  — s once per
// sample into LDS, then every output reads it with lanes across o.  Nothing of size C^2 is written by either.
#include <stdint.h>
#include <stdlib.h>

#include "lk_common.h"
#include "lk_quadtile.h"
#include "lk_split16.h"

namespace lk {

constexpr int QD_CT = 8;  // outputs per chunk: 128 accumulator registers, beside them the 16 weights and the staging registers
// most positions L at which the v panel of a super-tile (128 columns x L positions, fp32) stays in LDS across the class
// chunks: 32 KiB beside the 48 KiB tile arena and the 64 KiB of sums at C = LK_QUADDIAG_MAX_C (160 KiB per CU)
constexpr int QD_RESIDENT_MAX_L = 64;

inline bool qd_resident(int64_t L) { return L <= QD_RESIDENT_MAX_L; }
inline int qd_chunks(int64_t C) { return (int)((C + QD_CT - 1) / QD_CT); }
inline size_t qd_lds_bytes(int64_t C, int64_t L) {
  return (size_t)QcLds<QD_CT>::BYTES + (qd_resident(L) ? (size_t)128 * L * sizeof(float) : 0) + (size_t)4 * C * sizeof(float);
}

// grid = B * split workgroups of 4 waves; workgroup (n, sp) walks the super-tiles (32 rows o) x (128 columns i)
// t = sp, sp + split, ...; wave w owns columns [32 w, 32 w + 32) of the super-tile.  Inside a super-tile the outputs go by
// in chunks k = 0 .. nchunk - 1 of QD_CT; with C >= QD_CT the LAST chunk is moved back to end at C (it overlaps its
// predecessor, whose outputs it does not add again), so every chunk reads QD_CT real outputs and the tile products'
// prefetch of the next chunk never looks past the tensor.
// MODE: 0 Kronecker weights 1 / (w0[o] w1[i] + delta), 1 diagonal w0[o][i].  ARITH as in lk_quadconv.hip.  RESIDENT: the v
// panel of the super-tile is copied to LDS once (rows i0 .. i0 + 127 of v[n] are one contiguous run) and the tile products
// read it there, in the panel's own coordinates (column 32 w + lo of `ncols`).
template <int MODE, int ARITH, bool RESIDENT>
__global__ __launch_bounds__(256) void quaddiag_shared_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                              const float* __restrict__ w0, const float* __restrict__ w1,
                                                              const float* __restrict__ delta, int C, int Do, int Dk, int L,
                                                              int split, float* __restrict__ partial,
                                                              int64_t u_sample_stride, unsigned u_class_stride) {
  constexpr int CT = QD_CT;
  constexpr bool B6 = ARITH != 0;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float* panel = reinterpret_cast<float*>(lds + QcLds<CT>::BYTES);
  float* sums = reinterpret_cast<float*>(lds + QcLds<CT>::BYTES + (RESIDENT ? 128 * L * (int)sizeof(float) : 0));  // [4][C]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lo = lane & 31, hi = lane >> 5;
  // XCD-aware, as quadform_conv_kernel: the workgroups of one sample re-read u[n], v[n] and are given to ONE XCD
  int n = blockIdx.x / split, sp = blockIdx.x % split;
  if (gridDim.x % (8 * split) == 0) {
    const int xcd = blockIdx.x % 8, j = blockIdx.x / 8;
    n = xcd + 8 * (j / split), sp = j % split;
  }
  const int nOt = (Do + 31) / 32, nIg = (Dk + 127) / 128, ntiles = nOt * nIg;
  const int nchunk = (C + CT - 1) / CT, Cg = C < CT ? C : CT;
  const float* __restrict__ un = u + (size_t)n * u_sample_stride;
  const float* __restrict__ vn = v + (size_t)n * Dk * L;
  const float dlt = MODE == 0 ? delta[0] : 0.f;

  float* mysums = sums + wave * C;
  for (int c = lane; c < C; c += 64) mysums[c] = 0.f;
  __syncthreads();

  auto chunk_base = [&](int k) { return C < CT ? 0 : (k * CT + CT <= C ? k * CT : C - CT); };
  // operands of (super-tile t, chunk k): the chunk's first output is added to the sample's base pointer in 64 bits, the
  // 32-bit offsets of the tile products then span QD_CT outputs (host: QD_CT * class stride < 2^32)
  auto operands = [&](int t, int k) {
    const float* uk = un + (size_t)chunk_base(k) * u_class_stride;
    if (RESIDENT) return QcOperands{uk, panel, (t % nOt) * 32, wave * 32 + lo, u_class_stride};
    return QcOperands{uk, vn, (t % nOt) * 32, (t / nOt) * 128 + wave * 32 + lo, u_class_stride};
  };
  QcStage<CT> st;
  for (int t = sp; t < ntiles; t += split) {
    const int o0 = (t % nOt) * 32, i0 = (t / nOt) * 128, icol = i0 + wave * 32 + lo;
    const int ncols = Dk - i0 < 128 ? Dk - i0 : 128;
    const int DkT = RESIDENT ? ncols : Dk;  // the column bound in the coordinates the tile products are given
    // weights of this lane's 16 (o, i) positions: the same for every chunk of the super-tile
    float wgt[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = o0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
      const bool ok = o < Do && icol < Dk;
      if (MODE == 0) {
        const float d = w0[ok ? o : 0] * w1[ok ? icol : 0] + dlt;
        wgt[r] = ok ? __builtin_amdgcn_rcpf(d) : 0.f;
      } else {
        wgt[r] = ok ? w0[(unsigned)(o * Dk + icol)] : 0.f;
      }
    }
    if (RESIDENT) {
      // (the previous super-tile's last tile product ended with a barrier: nobody reads the panel any more)
      const float* __restrict__ src = vn + (size_t)i0 * L;
      const int count = ncols * L;
      if (B6) {  // L % 4 == 0 and v 16-byte aligned: whole float4s
        for (int e = tid; e < count / 4; e += 256)
          reinterpret_cast<f32x4*>(panel)[e] = reinterpret_cast<const f32x4*>(src)[e];
      } else {
        for (int e = tid; e < count; e += 256) panel[e] = src[e];
      }
      __syncthreads();
    }
    // the bf16 pipeline runs across chunks (and, with v in memory, across super-tiles); a resident panel is first read
    // after it has been staged, so each super-tile starts its own stream
    if (B6 && (RESIDENT || t == sp)) qc_fetch_b6<CT>(st, 0, (CT + 1) / 2, 0, 2, operands(t, 0), 0, Cg, Do, DkT, L);
    for (int k = 0; k < nchunk; ++k) {
      f32x16 acc[CT];
      if constexpr (B6) {
        const bool in_tile = k + 1 < nchunk;
        const bool has_next = in_tile || (!RESIDENT && t + split < ntiles);
        const QcOperands nxt = in_tile ? operands(t, k + 1) : operands(RESIDENT ? t : t + split, 0);
        qc_tile_gemm_b6<CT>(operands(t, k), nxt, has_next, Cg, Do, DkT, L, lds, acc, st);
      } else {
        qc_tile_gemm<CT>(operands(t, k), Cg, Do, DkT, L, lds, acc);
      }
      // each output's weighted tile squared and summed: this lane's 16 positions, ...
      float s[CT];
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        float x = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) x = __builtin_fmaf(acc[c][r] * wgt[r], acc[c][r], x);
        s[c] = x;
      }
      // ... then the 64 lanes x 8 outputs folded to one output per group of 8 lanes: each exchange halves the outputs a
      // lane still carries (4 + 2 + 1 shuffles), three more sum the group — 10 shuffles where 8 wave sums take 48
      float a4[4], a2[2];
#pragma unroll
      for (int j = 0; j < 4; ++j) a4[j] = (hi ? s[4 + j] : s[j]) + __shfl_xor(hi ? s[j] : s[4 + j], 32, 64);
      const int b4 = (lane >> 4) & 1, b3 = (lane >> 3) & 1;
#pragma unroll
      for (int j = 0; j < 2; ++j) a2[j] = (b4 ? a4[2 + j] : a4[j]) + __shfl_xor(b4 ? a4[j] : a4[2 + j], 16, 64);
      float a1 = (b3 ? a2[1] : a2[0]) + __shfl_xor(b3 ? a2[0] : a2[1], 8, 64);
      a1 += __shfl_xor(a1, 4, 64);
      a1 += __shfl_xor(a1, 2, 64);
      a1 += __shfl_xor(a1, 1, 64);
      const int c = 4 * hi + 2 * b4 + b3, cls = chunk_base(k) + c;
      // (a moved-back last chunk adds only the outputs its predecessor did not cover; this wave alone touches its sums)
      if ((lane & 7) == 0 && c < Cg && cls >= k * CT) mysums[cls] += a1;
    }
  }
  __syncthreads();
  float* __restrict__ out = partial + ((size_t)n * split + sp) * C;
  for (int c = tid; c < C; c += 256) out[c] = (sums[c] + sums[C + c]) + (sums[2 * C + c] + sums[3 * C + c]);
}

// fvar_diag[n][c] += the sums of the workgroups of sample n, in fixed order: one owner per element, no atomics
__global__ __launch_bounds__(256) void quaddiag_reduce_kernel(const float* __restrict__ partial, int64_t B, int C, int split,
                                                              float* __restrict__ fvar_diag) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= B * C) return;
  const int64_t n = e / C;
  const int c = (int)(e % C);
  float s = 0.f;
  for (int sp = 0; sp < split; ++sp) s += partial[((size_t)n * split + sp) * C + c];
  fvar_diag[e] += s;
}

// ---- plain Linear layers ---------------------------------------------------------------------------------------------------
// One workgroup per sample.  Phase 1: s[o] = sum_i v[n][i]^2 w[o,i] into LDS, a wave per row o with its lanes across i (the
// diagonal posterior's var_w[o][:] is then read contiguously).  Phase 2: a wave per output c, lanes across o:
// sum_o u[c][n][o]^2 s[o] + ub[c][n][o]^2 wb[o].  MODE as above; the bias weight is 1 / (wb[o] + delta_b) (Kronecker) or wb[o].
template <int MODE>
__global__ __launch_bounds__(256) void quaddiag_linear_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                              const float* __restrict__ w0, const float* __restrict__ w1,
                                                              const float* __restrict__ delta, int64_t B, int C, int Do, int Di,
                                                              const float* __restrict__ ub, const float* __restrict__ wb,
                                                              const float* __restrict__ delta_b, float* __restrict__ fvar_diag) {
  extern __shared__ float s_lds[];  // [Do]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = blockIdx.x;
  const float* __restrict__ vn = v + n * Di;
  const float dlt = MODE == 0 ? delta[0] : 0.f;
  for (int o = wave; o < Do; o += 4) {
    const float lo_ = MODE == 0 ? w0[o] : 0.f;
    float x = 0.f;
    for (int i = lane; i < Di; i += 64) {
      const float a = vn[i];
      const float w = MODE == 0 ? __builtin_amdgcn_rcpf(lo_ * w1[i] + dlt) : w0[(size_t)o * Di + i];
      x = __builtin_fmaf(a * a, w, x);
    }
    x = wave_sum(x);
    if (lane == 0) s_lds[o] = x;
  }
  __syncthreads();
  const float db = (ub != nullptr && MODE == 0) ? delta_b[0] : 0.f;
  for (int c = wave; c < C; c += 4) {
    const float* __restrict__ uc = u + ((size_t)c * B + n) * Do;
    const float* __restrict__ ubc = ub != nullptr ? ub + ((size_t)c * B + n) * Do : nullptr;
    float x = 0.f;
    for (int o = lane; o < Do; o += 64) {
      const float a = uc[o];
      x = __builtin_fmaf(a * a, s_lds[o], x);
      if (ubc != nullptr) {
        const float b = ubc[o];
        x = __builtin_fmaf(b * b, MODE == 0 ? __builtin_amdgcn_rcpf(wb[o] + db) : wb[o], x);
      }
    }
    x = wave_sum(x);
    if (lane == 0) fvar_diag[n * C + c] += x;
  }
}

}  // namespace lk

using namespace lk;

extern "C" size_t lk_quaddiag_shared_workspace_bytes(int64_t B, int64_t C, int64_t Do, int64_t Dk) {
  if (B < 1 || C < 1 || C > LK_QUADDIAG_MAX_C || Do < 1 || Dk < 1) return 0;
  return (size_t)B * qc_split(B, Do, Dk) * C * sizeof(float);
}

// the argument contract of the two weight-sharing entry points, checked before the first device call
static int quaddiag_shared_check(const char* what, bool pointers, int64_t B, int64_t C, int64_t Do, int64_t Dk, int64_t L,
                                 int seed_major, bool diag, const void* ws, size_t ws_bytes) {
  LK_REQUIRE(pointers && B >= 0 && C >= 1 && Do >= 1 && Dk >= 1 && L >= 1, "%s: bad arguments", what);
  LK_REQUIRE(C <= LK_QUADDIAG_MAX_C, "%s: more than %d outputs are not supported by the fused kernel", what, LK_QUADDIAG_MAX_C);
  LK_REQUIRE(B * 64 < (1ll << 31) && C * L * Do < (1ll << 29) && L * Dk < (1ll << 29) && (!diag || Do * Dk < (1ll << 31)) &&
                 (!seed_major || B * Do * L < (1ll << 28)),
             "%s: sizes out of range", what);
  LK_REQUIRE(B == 0 || (ws != nullptr && ws_bytes >= lk_quaddiag_shared_workspace_bytes(B, C, Do, Dk)), "%s: workspace too small",
             what);
  return LK_OK;
}

template <int MODE>
static int quaddiag_shared_run(const float* u, const float* v, const float* w0, const float* w1, const float* delta, int64_t B,
                               int64_t C, int64_t Do, int64_t Dk, int64_t L, int seed_major, float* fvar_diag, void* ws,
                               hipStream_t stream, const char* what) {
  if (B == 0) return LK_OK;
  // u is [B][C][Do][L] or, seed_major, [C][B][Do][L]
  const int64_t uss = seed_major ? Do * L : C * Do * L;
  const unsigned ucs = (unsigned)(seed_major ? B * Do * L : Do * L);
  const int split = qc_split(B, Do, Dk);
  float* partial = static_cast<float*>(ws);
  const dim3 grid((unsigned)(B * split));
  const bool b6 = qc_arith(L, qc_aligned16(u) && qc_aligned16(v)) == 1;
  const bool res = qd_resident(L);
  const size_t lds = qd_lds_bytes(C, L);
#define LK_QD_LAUNCH(ARITH, RES)                                                                                          \
  {                                                                                                                       \
    static bool attr_set = false;                                                                                         \
    if (!attr_set) {                                                                                                      \
      (void)hipFuncSetAttribute((const void*)quaddiag_shared_kernel<MODE, ARITH, RES>,                                    \
                                hipFuncAttributeMaxDynamicSharedMemorySize,                                               \
                                (int)qd_lds_bytes(LK_QUADDIAG_MAX_C, RES ? QD_RESIDENT_MAX_L : QD_RESIDENT_MAX_L + 1));   \
      attr_set = true;                                                                                                    \
    }                                                                                                                     \
    hipLaunchKernelGGL((quaddiag_shared_kernel<MODE, ARITH, RES>), grid, dim3(256), lds, stream, u, v, w0, w1, delta,     \
                       (int)C, (int)Do, (int)Dk, (int)L, split, partial, uss, ucs);                                       \
  }
  if (b6 && res) LK_QD_LAUNCH(1, true)
  else if (b6) LK_QD_LAUNCH(1, false)
  else if (res) LK_QD_LAUNCH(0, true)
  else LK_QD_LAUNCH(0, false)
#undef LK_QD_LAUNCH
  const int64_t total = B * C;
  hipLaunchKernelGGL(quaddiag_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, partial, B, (int)C,
                     split, fvar_diag);
  return check_launch(what);
}

extern "C" int lk_kron_quaddiag_shared_f32(const float* u, const float* v, const float* l1, const float* l2,
                                           const float* delta, int64_t B, int64_t C, int64_t Do, int64_t Dk, int64_t L,
                                           int seed_major, float* fvar_diag, void* ws, size_t ws_bytes, void* stream) {
  const char* what = "lk_kron_quaddiag_shared_f32";
  const int rc = quaddiag_shared_check(what, u && v && l1 && l2 && delta && fvar_diag, B, C, Do, Dk, L, seed_major, false, ws,
                                       ws_bytes);
  return rc != LK_OK ? rc : quaddiag_shared_run<0>(u, v, l1, l2, delta, B, C, Do, Dk, L, seed_major, fvar_diag, ws,
                                                   (hipStream_t)stream, what);
}

extern "C" int lk_diag_quaddiag_shared_f32(const float* u, const float* v, const float* var_w, int64_t B, int64_t C,
                                           int64_t Do, int64_t Dk, int64_t L, int seed_major, float* fvar_diag, void* ws,
                                           size_t ws_bytes, void* stream) {
  const char* what = "lk_diag_quaddiag_shared_f32";
  const int rc = quaddiag_shared_check(what, u && v && var_w && fvar_diag, B, C, Do, Dk, L, seed_major, true, ws, ws_bytes);
  return rc != LK_OK ? rc : quaddiag_shared_run<1>(u, v, var_w, nullptr, nullptr, B, C, Do, Dk, L, seed_major, fvar_diag, ws,
                                                   (hipStream_t)stream, what);
}

// (s[Do] lives in LDS; the grid is one workgroup per sample)
static int quaddiag_linear_check(const char* what, bool pointers, int64_t B, int64_t C, int64_t Do, int64_t Di) {
  LK_REQUIRE(pointers && B >= 0 && C >= 1 && Do >= 1 && Di >= 1, "%s: bad arguments", what);
  LK_REQUIRE(C <= LK_QUADDIAG_MAX_C, "%s: more than %d outputs are not supported by the fused kernel", what, LK_QUADDIAG_MAX_C);
  LK_REQUIRE(B < (1ll << 31) && Do <= 32768 && Di < (1ll << 31), "%s: sizes out of range", what);
  return LK_OK;
}

template <int MODE>
static int quaddiag_linear_run(const float* u, const float* v, const float* w0, const float* w1, const float* delta, int64_t B,
                               int64_t C, int64_t Do, int64_t Di, const float* ub, const float* wb, const float* delta_b,
                               float* fvar_diag, hipStream_t stream, const char* what) {
  if (B == 0) return LK_OK;
  const size_t lds = (size_t)Do * sizeof(float);
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)quaddiag_linear_kernel<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, 32768 * 4);
    attr_set = true;
  }
  hipLaunchKernelGGL((quaddiag_linear_kernel<MODE>), dim3((unsigned)B), dim3(256), lds, stream, u, v, w0, w1, delta, B, (int)C,
                     (int)Do, (int)Di, ub, wb, delta_b, fvar_diag);
  return check_launch(what);
}

extern "C" int lk_kron_quaddiag_linear_f32(const float* u, const float* v, const float* l1, const float* l2,
                                           const float* delta, int64_t B, int64_t C, int64_t Do, int64_t Di, const float* ub,
                                           const float* lb, const float* delta_b, float* fvar_diag, void* stream) {
  const char* what = "lk_kron_quaddiag_linear_f32";
  // (a bias block needs lb and delta_b)
  const int rc = quaddiag_linear_check(what, u && v && l1 && l2 && delta && fvar_diag && (ub == nullptr || (lb && delta_b)), B, C,
                                       Do, Di);
  return rc != LK_OK ? rc : quaddiag_linear_run<0>(u, v, l1, l2, delta, B, C, Do, Di, ub, lb, delta_b, fvar_diag,
                                                   (hipStream_t)stream, what);
}

extern "C" int lk_diag_quaddiag_linear_f32(const float* a, const float* g, const float* var_w, const float* var_b, int64_t B,
                                           int64_t C, int64_t Do, int64_t Di, float* fvar_diag, void* stream) {
  const char* what = "lk_diag_quaddiag_linear_f32";
  const int rc = quaddiag_linear_check(what, a && g && var_w && fvar_diag, B, C, Do, Di);
  return rc != LK_OK ? rc : quaddiag_linear_run<1>(g, a, var_w, nullptr, nullptr, B, C, Do, Di, var_b ? g : nullptr, var_b,
                                                   nullptr, fvar_diag, (hipStream_t)stream, what);
}

// Which path a shape takes (include/laplace_hip.h): arith | resident << 1 | rem << 2 | chunks << 5 | split << 15
extern "C" int lk_quaddiag_variant(int form, int64_t B, int64_t C, int64_t Do, int64_t Dk, int64_t L, int aligned16) {
  if ((form != LK_QD_KRON && form != LK_QD_DIAG) || B < 1 || C < 1 || C > LK_QUADDIAG_MAX_C || Do < 1 || Dk < 1 || L < 1)
    return -1;
  return qc_arith(L, aligned16 != 0) | (qd_resident(L) ? 2 : 0) | (int)(C % QD_CT) << 2 | qd_chunks(C) << 5 |
         qc_split(B, Do, Dk) << 15;
}
