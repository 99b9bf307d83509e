// The `nn` (weight-space sampling) predictive of a last-layer posterior: S sampled nn.Linear heads applied to the SAME feature block,
// each followed by a row softmax, averaged over the draws — without an [S][B][C] tensor in memory.
//   phi [B][D] features;  theta [S][ld] the rows of sample(): W_s [C][D] row-major at offset 0, b_s [C] at offset C D (has_bias)
//   LK_NN_HEAD_PROBS    probs[b][c] = (1 / S) sum_s softmax_c(phi_b . W_s[c] + b_s[c])       (the row maximum subtracted)
//   LK_NN_HEAD_MOMENTS  mean[b][c], var[b][c]: mean and unbiased variance over s of f_s[b][c] (torch's .var(dim=0); S == 1: NaN)
//   LK_NN_HEAD_SAMPLES  out[s][b][c] = f_s[b][c], or its row softmax
// Replaces laplace/lllaplace.py:257-314 (a vector_to_parameters scatter and a head launch per draw, a stacked [S][B][C] tensor, a
// softmax tensor of that size and a mean) and the regression moments of laplace/baselaplace.py:1344-1394.
//
// Work split.  A workgroup of 256 threads (four waves) owns a tile of R = 16 RT batch rows and a contiguous chunk of draws.  Its
// phi rows are staged in LDS once when they fit whole (row stride kc + 4 floats: the 16-byte operand reads of the 16 rows of a tile
// fall on different banks), else in K-chunks of 256 columns restaged per draw (phi is B x D and L2 resident).  theta is the HBM
// stream: every element is read once per batch tile, straight into the B-operand registers of v_mfma_f32_16x16x4_f32 (the exact fp32
// instruction: a k-ordered fmaf chain), one 16-byte load per lane per class tile and 16 columns where D % 4 == 0 and ld % 4 == 0
// (four 4-byte loads otherwise), the next 16 columns in flight under the products of the current ones.  A lane's load holds
// k = 4 g .. 4 g + 3, so instruction m of a 16-column group takes k = 4 g + m for both operands; the groups ascend: a fixed
// order, the same for every element, draw and load width.  A draw's logits never leave the accumulator registers: lane (g, c16) of
// a 16 x 16 tile holds rows 4 g .. 4 g + 3 of class c16, the row statistics of the softmax go by xor shuffles over the 16 lanes of a
// row and (regime 1) one LDS exchange across the waves, and sum_s p_s (or the Welford mean and M2) stays in registers in the same
// layout across the draws of the chunk.
// Two regimes by C (lk_nn_head_variant names the one a shape takes):
//   0  C <= 64:  a WAVE per draw.  A wave owns all NT = ceil(C / 16) class tiles (3 -> 4) of its own contiguous quarter of the
//      workgroup's draws; no barrier in the draw loop (unless phi is restaged).  R = 64 rows.
//   1  C <= 1024: a WORKGROUP per draw.  Class tile t belongs to wave t % 4; a wave holds NT = 2, 4, 8 or 16 tiles and the rows per
//      tile follow from C so that accumulators and running sums stay in registers: R = 64 (C <= 256), 32 (<= 512), 16 (<= 1024).
// The draws are split over G groups (a wave in regime 0, a workgroup in regime 1) so that a launch has about 512 workgroups at any B;
// the workgroups of one draw chunk are neighbours on one XCD (xcd_tile_order) and share theta in its L2.  G == 1: the kernel writes
// the result.  G > 1: every group writes its partial ([G][B][C] sums, or [G][2][B][C] mean / M2) to the workspace with plain
// stores and a second small launch adds them in ascending group order (Chan's update for the moments): at most two launches.
// Every output element has one owner, every reduction a fixed order, no atomics: two equal calls are bit-equal.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): no instance uses scratch.
#include "lk_common.h"
#include "lk_stream.h"  // disjoint, grid_blocks

#include <math.h>

namespace lk {

constexpr int NH_MAX_C = LK_NN_HEAD_MAX_C;
constexpr int NH_WAVE_C = 64;                   // largest C of the wave-per-draw regime
constexpr int NH_KC = 256;                      // columns of a phi stage when the rows do not fit whole
constexpr int64_t NH_PHI_BUDGET = 144 * 1024;   // bytes of LDS the phi stage may take
constexpr int64_t NH_WANT_BLOCKS = 512;         // 256 CUs x 2 workgroups

struct NhPlan {
  int wpd, nt, rt;    // waves per draw (1 or 4), class tiles per wave, 16-row tiles per workgroup
  int kc;             // columns of the phi stage (a multiple of 64); kc >= D: staged once
  int dpg, G;         // draws per group, groups
  int64_t nbt, ny;    // batch tiles, draw chunks (workgroups per batch tile)
  size_t lds;
};

static bool nh_plan(int64_t B, int64_t C, int64_t D, int64_t S, int mode, NhPlan& p) {
  if (mode < 0 || mode > 2 || C < 1 || C > NH_MAX_C || D < 1 || D >= (1ll << 20) || S < 1 || S >= (1ll << 20) || B < 0 ||
      B >= (1ll << 31))
    return false;
  const int T = (int)((C + 15) / 16);
  if (C <= NH_WAVE_C) {
    p.wpd = 1, p.nt = T == 3 ? 4 : T, p.rt = 4;
  } else {
    p.wpd = 4, p.nt = 2;
    while (4 * p.nt < T) p.nt *= 2;
    p.rt = 16 / p.nt < 4 ? 16 / p.nt : 4;
  }
  const int64_t R = 16 * p.rt, Dp = (D + 63) / 64 * 64;
  p.kc = R * (Dp + 4) * 4 <= NH_PHI_BUDGET ? (int)Dp : NH_KC;
  p.nbt = B > 0 ? (B + R - 1) / R : 1;
  const int64_t gpb = 4 / p.wpd, want = (NH_WANT_BLOCKS + p.nbt - 1) / p.nbt * gpb;
  p.dpg = (int)((S + want - 1) / want);
  p.G = (int)((S + p.dpg - 1) / p.dpg);
  p.ny = (p.G + gpb - 1) / gpb;
  p.lds = (size_t)(R * (p.kc + 4) + 2 * 4 * R) * sizeof(float);
  return true;
}

// maximum or sum over the classes of every row of the tile: RT x 4 values per lane, over the 16 lanes of a row by shuffles and, with
// four waves per draw, over the waves through red [4][R] (one barrier; the caller alternates two buffers)
template <int WPD, int RT, bool MAX>
__device__ __forceinline__ void nh_row_reduce(float (&v)[RT][4], float* red) {
  constexpr int R = 16 * RT;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c16 = lane & 15;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float x = v[rt][r];
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) {
        const float y = __shfl_xor(x, off, 64);
        x = MAX ? fmaxf(x, y) : x + y;
      }
      v[rt][r] = x;
      if (WPD == 4 && c16 == 0) red[wave * R + 16 * rt + 4 * g + r] = x;
    }
  if constexpr (WPD == 4) {
    __syncthreads();
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* q = red + 16 * rt + 4 * g + r;
        v[rt][r] = MAX ? fmaxf(fmaxf(q[0], q[R]), fmaxf(q[2 * R], q[3 * R])) : ((q[0] + q[R]) + q[2 * R]) + q[3 * R];
      }
  }
}

// the 16 columns k0 + 4 g .. + 3 of the lane's class rows: one 16-byte load a tile, or four 4-byte ones
template <int NT>
__device__ __forceinline__ void nh_load_w(f32x4 (&w)[NT], const float* wb, int64_t qstride, const bool (&ok)[NT], int k, int D,
                                          bool vec) {
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (ok[q] && k < D) {
      const float* p = wb + q * qstride + k;
      if (vec) {
        v = *(const f32x4*)p;  // (D % 4 == 0: k + 3 < D)
      } else {
        v[0] = p[0];
        if (k + 1 < D) v[1] = p[1];
        if (k + 2 < D) v[2] = p[2];
        if (k + 3 < D) v[3] = p[3];
      }
    }
    w[q] = v;
  }
}

template <int MODE, int WPD, int NT, int RT>
__global__ __launch_bounds__(256) void nn_head_kernel(const float* __restrict__ phi, const float* __restrict__ theta, int64_t B, int C,
                                                      int D, int S, int64_t ld, int has_bias, int vec, int softmax, int kc, int dpg,
                                                      int G, int nbt, float* __restrict__ out, float* __restrict__ out2,
                                                      float* __restrict__ work) {
  extern __shared__ float lds[];
  constexpr int R = 16 * RT;
  constexpr bool PROB = MODE == LK_NN_HEAD_PROBS, MOM = MODE == LK_NN_HEAD_MOMENTS;
  const int ps = kc + 4;
  float* ph = lds;            // [R][ps]
  float* red = lds + R * ps;  // [2][4][R]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c16 = lane & 15;
  const int w = xcd_tile_order((int)blockIdx.x, (int)gridDim.x);
  const int bt = w % nbt, cy = w / nbt;
  const int64_t b0 = (int64_t)bt * R;
  const int gid = WPD == 1 ? 4 * cy + wave : cy;
  const int64_t s0 = (int64_t)gid * dpg;
  const int cnt = gid >= G ? 0 : (S - s0 < dpg ? (int)(S - s0) : dpg);  // draws of this group (0: an idle wave of the last chunk)
  const bool single = kc >= D;
  const int KG = (D + 15) >> 4, KPC = kc >> 4;
  const int cls0 = 16 * (WPD == 1 ? 0 : wave) + c16;  // the lane's class in its first tile; tile q is 16 (or 64) q classes on
  constexpr int QC = WPD == 1 ? 16 : 64;
  const int64_t qstride = (int64_t)QC * D;
  bool ok[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) ok[q] = cls0 + QC * q < C;

  auto stage = [&](int kbase) {
    for (int idx = tid; idx < R * kc; idx += 256) {
      const int row = idx / kc, col = idx - row * kc, k = kbase + col;
      ph[row * ps + col] = (b0 + row < B && k < D) ? phi[(b0 + row) * D + k] : 0.f;
    }
  };
  if (single) {
    stage(0);
    __syncthreads();
  }

  float run[NT][RT][4];                   // sum_s p_s, or the running mean
  float m2[MOM ? NT : 1][RT][4];          // Welford's sum of squared deviations
#pragma unroll
  for (int q = 0; q < NT; ++q)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        run[q][rt][r] = 0.f;
        m2[MOM ? q : 0][rt][r] = 0.f;
      }

  for (int i = 0; i < dpg; ++i) {  // (uniform over the workgroup; a group past its draws only keeps the barriers)
    const bool active = i < cnt;
    const int64_t s = s0 + i;
    const float* wb = theta + (active ? s * ld : 0) + (int64_t)cls0 * D;
    bool live[NT];
    f32x4 acc[NT][RT];
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      live[q] = active && ok[q];
      const float bias = (live[q] && has_bias) ? theta[s * ld + (int64_t)C * D + cls0 + QC * q] : 0.f;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[q][rt] = f32x4{bias, bias, bias, bias};
    }
    f32x4 cur[NT], nxt[NT];
    nh_load_w<NT>(cur, wb, qstride, live, 4 * g, D, vec);
    for (int kg = 0; kg < KG; ++kg) {
      if (!single && kg % KPC == 0) {
        __syncthreads();  // (the previous stage is read)
        stage(16 * kg);
        __syncthreads();
      }
      if (kg + 1 < KG) nh_load_w<NT>(nxt, wb, qstride, live, 16 * (kg + 1) + 4 * g, D, vec);
      const float* ap = ph + c16 * ps + 16 * (single ? kg : kg % KPC) + 4 * g;
      f32x4 a[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) a[rt] = *(const f32x4*)(ap + 16 * rt * ps);
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int q = 0; q < NT; ++q)
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) acc[q][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt][m], cur[q][m], acc[q][rt], 0, 0, 0);
      if (kg + 1 < KG) {
#pragma unroll
        for (int q = 0; q < NT; ++q) cur[q] = nxt[q];
      }
    }
    if (!active) continue;  // (a wave per draw: no barrier below; four waves a draw: `active` is uniform)

    if (PROB || (MODE == LK_NN_HEAD_SAMPLES && softmax)) {
      float st[RT][4];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float m = -INFINITY;
#pragma unroll
          for (int q = 0; q < NT; ++q)
            if (ok[q]) m = fmaxf(m, acc[q][rt][r]);
          st[rt][r] = m;
        }
      nh_row_reduce<WPD, RT, true>(st, red);
      float sm[RT][4];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float t = 0.f;
#pragma unroll
          for (int q = 0; q < NT; ++q) {
            const float e = ok[q] ? expf(acc[q][rt][r] - st[rt][r]) : 0.f;
            acc[q][rt][r] = e;
            t += e;
          }
          sm[rt][r] = t;
        }
      nh_row_reduce<WPD, RT, false>(sm, red + 4 * R);
#pragma unroll
      for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[q][rt][r] /= sm[rt][r];
    }
    if constexpr (PROB) {
#pragma unroll
      for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int r = 0; r < 4; ++r) run[q][rt][r] += acc[q][rt][r];
    } else if constexpr (MOM) {
      const float inv = 1.f / (float)(i + 1);
#pragma unroll
      for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float f = acc[q][rt][r], d = f - run[q][rt][r];
            run[q][rt][r] += d * inv;
            m2[q][rt][r] = fmaf(d, f - run[q][rt][r], m2[q][rt][r]);
          }
    } else {
#pragma unroll
      for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int64_t b = b0 + 16 * rt + 4 * g + r;
            if (ok[q] && b < B) out[(s * B + b) * C + cls0 + QC * q] = acc[q][rt][r];
          }
    }
  }

  if (MODE == LK_NN_HEAD_SAMPLES || cnt == 0) return;
  const int64_t BC = B * C;
#pragma unroll
  for (int q = 0; q < NT; ++q)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t b = b0 + 16 * rt + 4 * g + r;
        if (!ok[q] || b >= B) continue;
        const int64_t e = b * C + cls0 + QC * q;
        if (PROB) {
          if (G == 1) out[e] = run[q][rt][r] / (float)S;
          else work[gid * BC + e] = run[q][rt][r];
        } else if (G == 1) {
          out[e] = run[q][rt][r];
          out2[e] = m2[MOM ? q : 0][rt][r] / (float)(S - 1);
        } else {
          work[2 * gid * BC + e] = run[q][rt][r];
          work[(2 * gid + 1) * BC + e] = m2[MOM ? q : 0][rt][r];
        }
      }
}

// the partials of the G draw groups in ascending group order: a thread per output element
template <int MODE>
__global__ __launch_bounds__(256) void nn_head_finish_kernel(const float* __restrict__ work, int64_t BC, int S, int dpg, int G,
                                                             float* __restrict__ out, float* __restrict__ out2) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < BC; e += (int64_t)gridDim.x * 256) {
    if (MODE == LK_NN_HEAD_PROBS) {
      float t = 0.f;
      for (int k = 0; k < G; ++k) t += work[k * BC + e];
      out[e] = t / (float)S;
    } else {
      float mean = work[e], M2 = work[BC + e], n = (float)(dpg < S ? dpg : S);
      for (int k = 1; k < G; ++k) {  // Chan, Golub, LeVeque: (n, mean, M2) + (nk, mk, M2k)
        const float nk = (float)(S - k * dpg < dpg ? S - k * dpg : dpg), mk = work[2 * k * BC + e], d = mk - mean, tot = n + nk;
        mean += d * (nk / tot);
        M2 += work[(2 * k + 1) * BC + e] + d * d * (n * nk / tot);
        n = tot;
      }
      out[e] = mean;
      out2[e] = M2 / (float)(S - 1);
    }
  }
}

static int64_t nh_work_bytes(const NhPlan& p, int64_t B, int64_t C, int mode) {
  if (mode == LK_NN_HEAD_SAMPLES || p.G == 1) return 0;
  return (int64_t)p.G * (mode == LK_NN_HEAD_MOMENTS ? 2 : 1) * B * C * 4;
}

template <typename Kern>
static void nh_allow_lds(Kern kern, size_t bytes) {  // (every launch: the attribute belongs to the current device)
  if (bytes > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

static int nh_check(const float* phi, const float* theta, int64_t B, int64_t C, int64_t D, int64_t S, int64_t ld, int has_bias,
                    int mode, const float* out, const float* out2, const void* work, int64_t work_bytes, NhPlan& p, int64_t& need) {
  LK_REQUIRE(mode >= 0 && mode <= 2, "lk_nn_head_f32: mode must be 0 (probs), 1 (moments) or 2 (samples), got %d", mode);
  const bool mom = mode == LK_NN_HEAD_MOMENTS;
  LK_REQUIRE(phi && theta && out && (out2 || !mom), "lk_nn_head_f32: null pointer");
  LK_REQUIRE(C >= 1 && C <= NH_MAX_C, "lk_nn_head_f32: C = %lld outside 1 <= C <= LK_NN_HEAD_MAX_C = %d", (long long)C, NH_MAX_C);
  LK_REQUIRE(D >= 1 && D < (1ll << 20), "lk_nn_head_f32: D out of range (1 <= D < 2^20)");
  LK_REQUIRE(S >= 1 && S < (1ll << 20), "lk_nn_head_f32: S out of range (1 <= S < 2^20)");
  LK_REQUIRE(B >= 0 && B < (1ll << 31), "lk_nn_head_f32: B out of range (0 <= B < 2^31)");
  const int64_t P = C * D + (has_bias ? C : 0);
  LK_REQUIRE(ld >= P, "lk_nn_head_f32: ld = %lld below the %lld parameters of a draw", (long long)ld, (long long)P);
  const float* o2 = mom ? out2 : nullptr;
  LK_REQUIRE((((uintptr_t)phi | (uintptr_t)theta | (uintptr_t)out | (uintptr_t)o2) & 15) == 0,
             "lk_nn_head_f32: pointers must be 16-byte aligned");
  (void)nh_plan(B, C, D, S, mode, p);
  need = nh_work_bytes(p, B, C, mode);
  if (need) {
    LK_REQUIRE(work, "lk_nn_head_f32: null workspace (%lld bytes needed: lk_nn_head_work_bytes)", (long long)need);
    LK_REQUIRE(((uintptr_t)work & 15) == 0, "lk_nn_head_f32: the workspace must be 16-byte aligned");
    if (work_bytes < need) {
      set_error("lk_nn_head_f32: workspace of %lld bytes, %lld needed", (long long)work_bytes, (long long)need);
      return LK_EWORKSPACE;
    }
  }
  const unsigned __int128 bc = (unsigned __int128)B * C * 4;
  const unsigned __int128 out_bytes = mode == LK_NN_HEAD_SAMPLES ? bc * S : bc;
  const unsigned __int128 in_bytes[2] = {(unsigned __int128)B * D * 4, ((unsigned __int128)(S - 1) * ld + P) * 4};
  const void* in[2] = {phi, theta};
  for (int k = 0; k < 2; ++k) {
    LK_REQUIRE(disjoint(out, out_bytes, in[k], in_bytes[k]) && (!o2 || disjoint(o2, bc, in[k], in_bytes[k])),
               "lk_nn_head_f32: an output overlaps an input");
    LK_REQUIRE(!need || disjoint(work, need, in[k], in_bytes[k]), "lk_nn_head_f32: the workspace overlaps an input");
  }
  LK_REQUIRE(!o2 || disjoint(out, bc, o2, bc), "lk_nn_head_f32: mean overlaps var");
  LK_REQUIRE(!need || (disjoint(work, need, out, out_bytes) && (!o2 || disjoint(work, need, o2, bc))),
             "lk_nn_head_f32: the workspace overlaps an output");
  return LK_OK;
}

}  // namespace lk

using namespace lk;

extern "C" int lk_nn_head_f32(const float* phi, const float* theta, int64_t B, int64_t C, int64_t D, int64_t S, int64_t ld,
                              int has_bias, int mode, int softmax, float* out, float* out2, void* work, int64_t work_bytes,
                              void* stream) {
  NhPlan p;
  int64_t need = 0;
  const int chk = nh_check(phi, theta, B, C, D, S, ld, has_bias, mode, out, out2, work, work_bytes, p, need);
  if (chk != LK_OK) return chk;
  const bool mom = mode == LK_NN_HEAD_MOMENTS;
  float* o2 = mom ? out2 : nullptr;
  if (B == 0) return LK_OK;

  hipStream_t st = (hipStream_t)stream;
  const int vec = D % 4 == 0 && ld % 4 == 0;
  const unsigned blocks = (unsigned)(p.nbt * p.ny);
  float* wk = need ? (float*)work : nullptr;
#define LK_NH_LAUNCH(MODE, WPD, NT, RT)                                                                                          \
  do {                                                                                                                           \
    nh_allow_lds(nn_head_kernel<MODE, WPD, NT, RT>, p.lds);                                                                      \
    hipLaunchKernelGGL((nn_head_kernel<MODE, WPD, NT, RT>), dim3(blocks), dim3(256), p.lds, st, phi, theta, B, (int)C, (int)D,   \
                       (int)S, ld, has_bias != 0, vec, softmax != 0, p.kc, p.dpg, p.G, (int)p.nbt, out, o2, wk);                 \
  } while (0)
#define LK_NH_SHAPE(MODE)                                                    \
  do {                                                                       \
    if (p.wpd == 1) {                                                        \
      if (p.nt == 1) LK_NH_LAUNCH(MODE, 1, 1, 4);                            \
      else if (p.nt == 2) LK_NH_LAUNCH(MODE, 1, 2, 4);                       \
      else LK_NH_LAUNCH(MODE, 1, 4, 4);                                      \
    } else if (p.nt == 2) LK_NH_LAUNCH(MODE, 4, 2, 4);                       \
    else if (p.nt == 4) LK_NH_LAUNCH(MODE, 4, 4, 4);                         \
    else if (p.nt == 8) LK_NH_LAUNCH(MODE, 4, 8, 2);                         \
    else LK_NH_LAUNCH(MODE, 4, 16, 1);                                       \
  } while (0)
  if (mode == LK_NN_HEAD_PROBS) LK_NH_SHAPE(LK_NN_HEAD_PROBS);
  else if (mom) LK_NH_SHAPE(LK_NN_HEAD_MOMENTS);
  else LK_NH_SHAPE(LK_NN_HEAD_SAMPLES);
#undef LK_NH_SHAPE
#undef LK_NH_LAUNCH
  int rc = check_launch("nn_head_kernel");
  if (rc != LK_OK || !need) return rc;
  const int64_t BC = B * C;
  const unsigned fb = (unsigned)grid_blocks(BC);
  if (mom)
    hipLaunchKernelGGL(nn_head_finish_kernel<LK_NN_HEAD_MOMENTS>, dim3(fb), dim3(256), 0, st, wk, BC, (int)S, p.dpg, p.G, out, o2);
  else
    hipLaunchKernelGGL(nn_head_finish_kernel<LK_NN_HEAD_PROBS>, dim3(fb), dim3(256), 0, st, wk, BC, (int)S, p.dpg, p.G, out, o2);
  return check_launch("nn_head_finish_kernel");
}

extern "C" int64_t lk_nn_head_work_bytes(int64_t B, int64_t C, int64_t D, int64_t S, int mode) {
  NhPlan p;
  return nh_plan(B, C, D, S, mode, p) ? nh_work_bytes(p, B, C, mode) : 0;
}

extern "C" int lk_nn_head_variant(int64_t B, int64_t C, int64_t D, int64_t S, int mode) {
  NhPlan p;
  if (!nh_plan(B, C, D, S, mode, p)) return -1;
  return (p.wpd == 4) | p.nt << 1 | p.rt << 6 | (p.kc < D) << 9 | p.G << 10;
}
