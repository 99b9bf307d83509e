// The JOINT GLM predictive covariance of one nn.Linear layer over a batch, without the [B, C, P] Jacobian:
//   cov[(n, c), (m, k)] += sum_o u[c][n][o] u[k][m][o] T[n][m][o]  +  sum_o ub[c][n][o] ub[k][m][o] bw[o]
//   T[n][m][o] = sum_i v[n][i] v[m][i] w[o][i]
//   MODE 0 (Kron):  w[o][i] = 1 / (l1[o] l2[i] + delta),  bw[o] = 1 / (lb[o] + delta_b);  u, v, ub: eigenbasis projections
//   MODE 1 (diag):  w[o][i] = var_w[o][i],                bw[o] = var_b[o];               u = ub = g, v = a
// cov is [B C][B C] row-major, row n C + c.  In the eigenbasis the rows of a Linear layer's Jacobian are rank one, so the cross-sample
// term factorises as the per-sample one does (quadform_linear_kernel, lk_kron.hip): B^2 Do Di multiply-adds whatever C is.
// Replaces laplace/utils/matrix.py:406-461 as called by laplace/baselaplace.py:1837-1843 (every row of Js [B C, P] rotated through
// both eigenbases and back, 4 (Do^2 Di + Do Di^2) flop a row, a second [B C, P] tensor and a [B C, P] x [P, B C] product) and the
// einsum of laplace/baselaplace.py:2117-2122.
//
// Work split.  A workgroup of 256 threads (four waves) owns a block of 16 x 16 sample pairs (n-tile <= m-tile: the upper block
// triangle only) and a contiguous range of the 32-wide tiles of Do.  T is a GEMM whose rows are the 256 pairs of the block, whose
// columns are the 32 o of a tile and whose reduction index is i: v_mfma_f32_32x32x2_f32 (the exact fp32 instruction), eight row
// tiles of 32 pairs (2 n x 16 m), two a wave.  The two v panels [16][128 of Di] and the weight tile [32 o][128 of Di] are staged in
// LDS (row stride 132 floats) per chunk of Di; Kron mode forms the weight tile there, one reciprocal per element per workgroup and
// chunk.  The A operand is formed in registers, v[n][i] * v[m][i], one multiply per element per k-step; a lane's 16-byte LDS reads
// hold i = 8 q + 4 h .. + 3 (h the lane's half), so instruction j of a group of four takes k = 8 q + 4 h + j for both operands: a
// fixed order.  T stays in the accumulators across the whole i loop and never reaches memory.
// Epilogue, per Do tile: lane (h, o) holds T of 32 pairs at its o.  For each of the C x C output pairs the 32 products
// (u[c][n][o] u[k][m][o]) T are summed over the 32 lanes of o by a transposing butterfly (31 shuffles for 32 sums, each sum the
// same five-level tree) which leaves sum q in lane bitrev5(q): every lane owns ONE sample pair of the block and keeps its C x C
// running sums across the Do tiles.  The bias block goes through the same fold with T = bw[o] into running sums of its own (its
// terms can be orders of magnitude smaller than the weight block's, lk_kron.hip) and is added at the end.
// Few sample pairs (small B): the Do tiles are split over S workgroups per pair block; their partial sums go to the workspace with
// plain stores and a second small launch adds them in ascending order.  cov[r][c] and cov[c][r] are written from one value by one
// thread (the pairs below the diagonal of a diagonal block are computed and dropped): no atomics, every reduction in a fixed order,
// two equal calls are bit-equal and a symmetric cov stays exactly symmetric.
// C is a template tier (1, 2, 4; C = 3 runs in tier 4 with the fourth output masked).  B, Do, Di are free: tails are masked.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md has the table; no instance uses scratch.
#include "lk_common.h"
#include "lk_stream.h"  // disjoint, grid_blocks

#include <math.h>

namespace lk {

constexpr int J_MAX_C = LK_JOINT_MAX_C;
constexpr int JT = 16;                      // samples per side of a pair block
constexpr int JKC = 128;                    // columns of Di staged per chunk
constexpr int JPS = JKC + 4;                // LDS row stride
constexpr int JOT = 32;                     // o per tile
constexpr int64_t J_WANT_BLOCKS = 512;      // 256 CUs x 2 workgroups
constexpr int64_t J_MAX_GRID = 1 << 20;     // the workgroups walk the (pair block, split) items beyond this
constexpr int64_t J_MAX_D = 1ll << 30;

struct JPlan {
  int ct;             // template tier of C
  int64_t nt, npb;    // sample tiles, pair blocks (upper block triangle)
  int ndt, S, tps;    // Do tiles, splits of them over the grid, tiles per split
  int64_t items;      // npb * S
};

static bool j_plan(int mode, int64_t B, int64_t C, int64_t Do, int64_t Di, JPlan& p) {
  if (mode < 0 || mode > 1 || C < 1 || C > J_MAX_C || B < 0 || B >= (1ll << 31) || B * C >= (1ll << 31) || Do < 1 || Do > J_MAX_D ||
      Di < 1 || Di > J_MAX_D)
    return false;
  p.ct = C == 1 ? 1 : (C == 2 ? 2 : 4);
  p.nt = (B + JT - 1) / JT;
  p.npb = p.nt * (p.nt + 1) / 2;
  p.ndt = (int)((Do + JOT - 1) / JOT);
  int64_t S = 1;
  if (p.npb > 0 && p.npb < J_WANT_BLOCKS) S = (J_WANT_BLOCKS + p.npb - 1) / p.npb;
  if (S > p.ndt) S = p.ndt;
  p.tps = (int)((p.ndt + S - 1) / S);
  p.S = (p.ndt + p.tps - 1) / p.tps;
  p.items = p.npb * p.S;
  return true;
}

static int64_t j_work_bytes(const JPlan& p, int64_t C) {
  return p.S > 1 ? p.items * (JT * JT) * 2 * C * C * (int64_t)sizeof(float) : 0;  // [S][npb][256 pairs][weight, bias][C][C]
}

// pair block pb of the upper block triangle, m-major: pb = tm (tm + 1) / 2 + tn, tn <= tm
__device__ __forceinline__ void j_block(int64_t pb, int64_t& tn, int64_t& tm) {
  int64_t t = (int64_t)((sqrt(8.0 * (double)pb + 1.0) - 1.0) * 0.5);
  while (t * (t + 1) / 2 > pb) --t;
  while ((t + 1) * (t + 2) / 2 <= pb) ++t;
  tm = t;
  tn = pb - t * (t + 1) / 2;
}

// cov[r][c] += val and its mirror, by the one owner of the two elements; in a diagonal block the pairs below the diagonal are dropped
__device__ __forceinline__ void j_emit(float* __restrict__ cov, int64_t B, int C, int64_t n, int64_t m, int c, int k, float val) {
  if (n >= B || m >= B) return;
  const int64_t N = B * C, row = n * C + c, col = m * C + k;
  if (row > col) return;
  cov[row * N + col] += val;
  if (row != col) cov[col * N + row] += val;
}

// x[q], q < 32, summed over the 32 lanes of a half wave: the total of q ends in x[0] of lane bitrev5(q).  At offset 16 >> s a lane
// keeps the entries whose bit 0 equals its lane bit and hands the others to its partner: 31 shuffles, five additions per total.
__device__ __forceinline__ float j_fold32(float (&x)[32], int lane) {
#pragma unroll
  for (int s = 0; s < 5; ++s) {
    const int off = 16 >> s;
    const bool up = (lane & off) != 0;
#pragma unroll
    for (int t = 0; t < (16 >> s); ++t) {
      const float keep = up ? x[2 * t + 1] : x[2 * t], send = up ? x[2 * t] : x[2 * t + 1];
      x[t] = keep + __shfl_xor(send, off, 64);
    }
  }
  return x[0];
}

// run[c][k] += sum over the tile's o of (u[c][n][o] u[k][m][o]) t for the lane's pair; t[rt][j]: the lane's 32 pairs at its o
template <int CT>
__device__ __forceinline__ void j_fold(const float* __restrict__ u, int64_t B, int C, int64_t Do, int64_t o, bool ook, int64_t n0,
                                       int64_t m0, int wave, int lane, const f32x16 (&t)[2], float (&run)[CT][CT]) {
  const int h = lane >> 5;
  float un[CT][2][2], um[CT][8];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int jn = 0; jn < 2; ++jn) {
        const int64_t n = n0 + 2 * (2 * wave + rt) + jn;
        un[c][rt][jn] = (c < C && ook && n < B) ? u[((int64_t)c * B + n) * Do + o] : 0.f;
      }
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) {
      const int64_t m = m0 + 8 * (mi >> 2) + 4 * h + (mi & 3);
      um[c][mi] = (c < C && ook && m < B) ? u[((int64_t)c * B + m) * Do + o] : 0.f;
    }
  }
#pragma unroll
  for (int c = 0; c < CT; ++c)
#pragma unroll
    for (int k = 0; k < CT; ++k) {
      if (c >= C || k >= C) continue;  // (uniform)
      float x[32];
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int j = 0; j < 16; ++j) x[16 * rt + j] = (un[c][rt][j >> 3] * um[k][4 * ((j >> 2) & 1) + (j & 3)]) * t[rt][j];
      run[c][k] += j_fold32(x, lane);
    }
}

template <int MODE, int CT>
__global__ __launch_bounds__(256) void joint_linear_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                           const float* __restrict__ w0, const float* __restrict__ w1,
                                                           const float* __restrict__ delta, int64_t B, int C, int64_t Do, int64_t Di,
                                                           const float* __restrict__ ub, const float* __restrict__ lb,
                                                           const float* __restrict__ delta_b, float* __restrict__ cov,
                                                           float* __restrict__ work, int64_t npb, int S, int tps, int ndt,
                                                           int64_t items) {
  __shared__ __attribute__((aligned(16))) float vn[JT * JPS];
  __shared__ __attribute__((aligned(16))) float vm[JT * JPS];
  __shared__ __attribute__((aligned(16))) float wt[JOT * JPS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, l32 = lane & 31;
  const float d = MODE == 0 ? delta[0] : 0.f;
  const float db = (MODE == 0 && ub) ? delta_b[0] : 0.f;
  // the pair this lane owns after the folds: sum q = bitrev5(l32), q = 16 rt + j
  const int q = (int)(__brev((unsigned)l32) >> 27), qrt = q >> 4, qj = q & 15;
  const int own_n = 2 * (2 * wave + qrt) + (qj >> 3), own_m = 8 * ((qj >> 2) & 1) + 4 * h + (qj & 3);

  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t pb = item % npb;
    const int s = (int)(item / npb);
    int64_t tn, tm;
    j_block(pb, tn, tm);
    const int64_t n0 = tn * JT, m0 = tm * JT;
    float run[CT][CT], runb[CT][CT];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
      for (int k = 0; k < CT; ++k) run[c][k] = runb[c][k] = 0.f;

    const int ot1 = (s + 1) * tps < ndt ? (s + 1) * tps : ndt;
    for (int ot = s * tps; ot < ot1; ++ot) {
      const int64_t o0 = (int64_t)ot * JOT, o = o0 + l32;
      const bool ook = o < Do;
      f32x16 acc[2];
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][r] = acc[1][r] = 0.f;
      for (int64_t i0 = 0; i0 < Di; i0 += JKC) {
        const int kq = (int)(((Di - i0 < JKC ? Di - i0 : JKC) + 7) >> 3), cw = 8 * kq;  // groups of 8 columns, staged width
        __syncthreads();  // (the previous stage is read)
        for (int idx = tid; idx < JT * cw; idx += 256) {
          const int row = idx / cw, col = idx - row * cw;
          const int64_t i = i0 + col;
          vn[row * JPS + col] = (n0 + row < B && i < Di) ? v[(n0 + row) * Di + i] : 0.f;
          vm[row * JPS + col] = (m0 + row < B && i < Di) ? v[(m0 + row) * Di + i] : 0.f;
        }
        for (int idx = tid; idx < JOT * cw; idx += 256) {
          const int row = idx / cw, col = idx - row * cw;
          const int64_t i = i0 + col, oo = o0 + row;
          float w = 0.f;
          if (oo < Do && i < Di) w = MODE == 0 ? 1.f / (w0[oo] * w1[i] + d) : w0[oo * Di + i];
          wt[row * JPS + col] = w;
        }
        __syncthreads();
        const float* bp = wt + l32 * JPS + 4 * h;
        const float* mp = vm + (l32 & 15) * JPS + 4 * h;
        const float* np0 = vn + (4 * wave + (l32 >> 4)) * JPS + 4 * h;
        const float* np1 = np0 + 2 * JPS;
        for (int g = 0; g < kq; ++g) {
          const f32x4 b = *(const f32x4*)(bp + 8 * g), am = *(const f32x4*)(mp + 8 * g);
          const f32x4 a0 = *(const f32x4*)(np0 + 8 * g), a1 = *(const f32x4*)(np1 + 8 * g);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j] * am[j], b[j], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j] * am[j], b[j], acc[1], 0, 0, 0);
          }
        }
      }
      j_fold<CT>(u, B, C, Do, o, ook, n0, m0, wave, lane, acc, run);
      if (ub) {
        const float bw = ook ? (MODE == 0 ? 1.f / (lb[o] + db) : lb[o]) : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][r] = acc[1][r] = bw;
        j_fold<CT>(ub, B, C, Do, o, ook, n0, m0, wave, lane, acc, runb);
      }
    }

    const int64_t n = n0 + own_n, m = m0 + own_m;
    if (S == 1) {
#pragma unroll
      for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int k = 0; k < CT; ++k)
          if (c < C && k < C) j_emit(cov, B, C, n, m, c, k, run[c][k] + runb[c][k]);
    } else {
      float* wp = work + (item * (JT * JT) + own_n * JT + own_m) * (2 * C * C);
#pragma unroll
      for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int k = 0; k < CT; ++k)
          if (c < C && k < C) {
            wp[c * C + k] = run[c][k];
            wp[C * C + c * C + k] = runb[c][k];
          }
    }
  }
}

// the partial sums of the S splits in ascending order, the bias block in a sum of its own: a thread per element of the block triangle
__global__ __launch_bounds__(256) void joint_finish_kernel(const float* __restrict__ work, int64_t B, int C, int64_t npb, int S,
                                                           float* __restrict__ cov) {
  const int CC = C * C;
  const int64_t total = npb * (JT * JT) * CC;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int ck = (int)(e % CC), pr = (int)((e / CC) % (JT * JT));
    const int64_t pb = e / ((int64_t)CC * JT * JT);
    float t = 0.f, tb = 0.f;
    for (int s = 0; s < S; ++s) {
      const float* wp = work + (((int64_t)s * npb + pb) * (JT * JT) + pr) * (2 * CC);
      t += wp[ck];
      tb += wp[CC + ck];
    }
    int64_t tn, tm;
    j_block(pb, tn, tm);
    j_emit(cov, B, C, tn * JT + pr / JT, tm * JT + pr % JT, ck / C, ck % C, t + tb);
  }
}

// the guards of both entry points (fn: the name the refusal carries); w_bytes: the bytes of the weight operand(s) behind w0 / w1
static int j_check(const char* fn, int mode, const float* u, const float* v, const float* w0, const float* w1, const float* delta,
                   int64_t B, int64_t C, int64_t Do, int64_t Di, const float* ub, const float* lb, const float* delta_b,
                   const float* cov, const void* ws, int64_t ws_bytes, JPlan& p, int64_t& need) {
  LK_REQUIRE(u && v && w0 && cov && (mode == 1 || (w1 && delta)), "%s: null pointer", fn);
  LK_REQUIRE(!ub || (lb && (mode == 1 || delta_b)), "%s: the bias block needs lb and delta_b", fn);
  LK_REQUIRE(C >= 1 && C <= J_MAX_C, "%s: C = %lld outside 1 <= C <= LK_JOINT_MAX_C = %d", fn, (long long)C, J_MAX_C);
  LK_REQUIRE(B >= 0 && B < (1ll << 31) && B * C < (1ll << 31), "%s: B = %lld, C = %lld: B * C out of range (0 <= B, B * C < 2^31)",
             fn, (long long)B, (long long)C);
  LK_REQUIRE(Do >= 1 && Do <= J_MAX_D && Di >= 1 && Di <= J_MAX_D, "%s: Do, Di out of range (1 <= Do, Di <= 2^30)", fn);
  (void)j_plan(mode, B, C, Do, Di, p);
  need = j_work_bytes(p, C);
  if (need) {
    if (!ws || ws_bytes < need) {
      set_error("%s: workspace of %lld bytes, %lld needed (lk_joint_linear_workspace_bytes)", fn, (long long)(ws ? ws_bytes : 0),
                (long long)need);
      return LK_EWORKSPACE;
    }
  }
  const unsigned __int128 n4 = sizeof(float), bc = (unsigned __int128)B * C;
  const unsigned __int128 cov_bytes = bc * bc * n4, u_bytes = bc * Do * n4;
  const void* in[8] = {u, v, w0, w1, delta, ub, lb, delta_b};
  const unsigned __int128 in_bytes[8] = {u_bytes, (unsigned __int128)B * Di * n4, (mode == 0 ? 1 : (unsigned __int128)Di) * Do * n4,
                                         (unsigned __int128)Di * n4, n4, u_bytes, (unsigned __int128)Do * n4, n4};
  for (int k = 0; k < 8; ++k) {
    if (!in[k]) continue;
    LK_REQUIRE(disjoint(cov, cov_bytes, in[k], in_bytes[k]), "%s: cov overlaps an input", fn);
    LK_REQUIRE(!need || disjoint(ws, need, in[k], in_bytes[k]), "%s: the workspace overlaps an input", fn);
  }
  LK_REQUIRE(!need || disjoint(ws, need, cov, cov_bytes), "%s: the workspace overlaps cov", fn);
  return LK_OK;
}

template <int MODE>
static int j_launch(const char* fn, const float* u, const float* v, const float* w0, const float* w1, const float* delta, int64_t B,
                    int64_t C, int64_t Do, int64_t Di, const float* ub, const float* lb, const float* delta_b, float* cov, void* ws,
                    int64_t ws_bytes, void* stream) {
  JPlan p;
  int64_t need = 0;
  const int chk = j_check(fn, MODE, u, v, w0, w1, delta, B, C, Do, Di, ub, lb, delta_b, cov, ws, ws_bytes, p, need);
  if (chk != LK_OK) return chk;
  if (B == 0) return LK_OK;
  hipStream_t st = (hipStream_t)stream;
  float* wk = need ? (float*)ws : nullptr;
  const unsigned blocks = (unsigned)(p.items < J_MAX_GRID ? p.items : J_MAX_GRID);
#define LK_J_LAUNCH(CT)                                                                                                         \
  hipLaunchKernelGGL((joint_linear_kernel<MODE, CT>), dim3(blocks), dim3(256), 0, st, u, v, w0, w1, delta, B, (int)C, Do, Di, ub, \
                     lb, delta_b, cov, wk, p.npb, p.S, p.tps, p.ndt, p.items)
  if (p.ct == 1) LK_J_LAUNCH(1);
  else if (p.ct == 2) LK_J_LAUNCH(2);
  else LK_J_LAUNCH(4);
#undef LK_J_LAUNCH
  const int rc = check_launch("joint_linear_kernel");
  if (rc != LK_OK || !need) return rc;
  hipLaunchKernelGGL(joint_finish_kernel, dim3((unsigned)grid_blocks(p.npb * (JT * JT) * C * C)), dim3(256), 0, st, wk, B, (int)C,
                     p.npb, p.S, cov);
  return check_launch("joint_finish_kernel");
}

}  // namespace lk

using namespace lk;

extern "C" int lk_kron_joint_linear_f32(const float* u, const float* v, const float* l1, const float* l2, const float* delta,
                                        int64_t B, int64_t C, int64_t Do, int64_t Di, const float* ub, const float* lb,
                                        const float* delta_b, float* cov, void* ws, int64_t ws_bytes, void* stream) {
  return j_launch<0>("lk_kron_joint_linear_f32", u, v, l1, l2, delta, B, C, Do, Di, ub, lb, delta_b, cov, ws, ws_bytes, stream);
}

extern "C" int lk_diag_joint_linear_f32(const float* a, const float* g, const float* var_w, const float* var_b, int64_t B, int64_t C,
                                        int64_t Do, int64_t Di, float* cov, void* ws, int64_t ws_bytes, void* stream) {
  return j_launch<1>("lk_diag_joint_linear_f32", g, a, var_w, nullptr, nullptr, B, C, Do, Di, var_b ? g : nullptr, var_b, nullptr,
                     cov, ws, ws_bytes, stream);
}

extern "C" int64_t lk_joint_linear_workspace_bytes(int64_t B, int64_t C, int64_t Do, int64_t Di) {
  JPlan p;
  return j_plan(0, B, C, Do, Di, p) ? j_work_bytes(p, C) : 0;
}

extern "C" int lk_joint_linear_variant(int mode, int64_t B, int64_t C, int64_t Do, int64_t Di) {
  JPlan p;
  if (!j_plan(mode, B, C, Do, Di, p)) return -1;
  return p.ct | (p.S > 1) << 3 | (p.S < (1 << 20) ? p.S : (1 << 20) - 1) << 4;
}
