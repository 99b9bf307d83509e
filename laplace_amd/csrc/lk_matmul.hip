// Batched matrix product of two traced tensors (hand-written attention q @ k^T and p @ v, attention pooling, bilinear heads) for
// the seed-batched reverse sweep.  With the cotangent g of out = a @ b for all S seeds stacked, g [S][NB][M][N], and ONE a [NB][M][K]
// and b [NB][K][N] per sample matrix shared by all seeds:
//   da[s][n] = g[s][n] b[n]^T   [M][K]   (reduction depth N)
//   db[s][n] = a[n]^T g[s][n]   [K][N]   (reduction depth M)
// Replaces, in the reverse pass of laplace/curvature/curvlinops.py:87-100 and curvature.py:88-129 through a matmul as stock torch
// runs it once per seed: two bmm calls per seed.  Batched over the seeds in torch the product either materialises the per-sample
// operand S times or needs a permuted copy of g; here g is read where the sweep leaves it (seed-major) and nothing is copied.
//
// One kernel template, two modes (MODE 0: da, MODE 1: db).  A workgroup of 4 waves owns one 64 x 64 tile of the output of ONE
// sample matrix n and loops over the seeds of its slice INSIDE: the panel of the per-sample operand the tile needs (64 rows of b
// for da, 64 columns of a for db, the whole reduction depth) is staged into LDS ONCE and reused by every seed while the depth is at
// most MM_RES_DEPTH = 128 (RESIDENT: 128 x 68 floats = 34 KiB of LDS, which leaves room for four workgroups per CU); deeper
// reductions restage it in 16-deep chunks per seed, like lk_gemm.hip.  g goes through LDS in 16-deep chunks.  Products run on the
// exact fp32 matrix instruction (v_mfma_f32_32x32x2_f32, as lk_gemm.hip and lk_attn.hip), the reduction index ascends in a fixed
// order, every output element has one owner and is stored once with a plain store: two equal calls give the same bits.  Sizes need
// not be multiples of anything (loads are guarded and zero-filled, stores guarded).  4-byte accesses only: no alignment beyond a
// float's is asked for.  The seeds are split over grid.y when the tiles alone leave the device short of waves.  One launch per
// requested output.  Nothing assumes packed fp32.
// Minimal traffic: g once per requested output, a / b once, the outputs once.
#include "lk_stream.h"

namespace lk {

constexpr int MM_RES_DEPTH = 128;  // deepest reduction whose operand panel stays in LDS across the seeds
constexpr int MM_LD = 64 + 4;      // row stride of the LDS tiles (as lk_gemm.hip)

// MODE 0: out[s][n] [P = M][Q = K] = g[s][n] [M][N] . o[n]^T, o = b [K][N], depth D = N
// MODE 1: out[s][n] [P = K][Q = N] = o[n]^T . g[s][n] [M][N], o = a [M][K], depth D = M
template <int MODE, bool RESIDENT>
__global__ __launch_bounds__(256) void matmul_vjp_kernel(const float* __restrict__ g, const float* __restrict__ o, int64_t S,
                                                         int64_t NB, int M, int K, int N, int tq, int tiles, int64_t s_per,
                                                         float* __restrict__ out) {
  __shared__ float sO[RESIDENT ? MM_RES_DEPTH : 16][MM_LD];  // [d][tile index]
  __shared__ float sG[16][MM_LD];                            // [d][tile index]
  const int P = MODE == 0 ? M : K, Q = MODE == 0 ? K : N, D = MODE == 0 ? N : M;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t n = (int64_t)blockIdx.x / tiles;
  const int tile = (int)((int64_t)blockIdx.x % tiles);
  const int p0 = (tile / tq) * 64, q0 = (tile % tq) * 64;
  const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
  const bool active = p0 + wi < P && q0 + wj < Q;  // (uniform over the wave: a wave with nothing to own skips the products)
  const float* on = o + n * (MODE == 0 ? (int64_t)K * N : (int64_t)M * K);
  const int64_t s_begin = (int64_t)blockIdx.y * s_per;
  const int64_t s_end = s_begin + s_per < S ? s_begin + s_per : S;

  // rows [d0, d0 + nd) of the operand panel -> sO[r0 ..]; the fast index of the load follows memory
  auto stage_o = [&](int d0, int nd, int r0) {
    for (int idx = tid; idx < nd * 64; idx += 256) {
      int dd, t;
      float v = 0.f;
      if (MODE == 0) {  // b[q0 + t][d]: d is contiguous
        dd = idx % nd, t = idx / nd;
        if (d0 + dd < D && q0 + t < Q) v = on[(int64_t)(q0 + t) * N + d0 + dd];
      } else {          // a[d][p0 + t]: t is contiguous
        t = idx & 63, dd = idx >> 6;
        if (d0 + dd < D && p0 + t < P) v = on[(int64_t)(d0 + dd) * K + p0 + t];
      }
      sO[r0 + dd][t] = v;
    }
  };

  if constexpr (RESIDENT) stage_o(0, (D + 15) / 16 * 16, 0);  // (D <= MM_RES_DEPTH; visible after the first barrier of the loop)
  for (int64_t s = s_begin; s < s_end; ++s) {
    const float* gs = g + (s * NB + n) * ((int64_t)M * N);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int d0 = 0; d0 < D; d0 += 16) {
      __syncthreads();  // (the previous chunk's reads are done)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int idx = e * 256 + tid;
        int dd, t;
        float v = 0.f;
        if (MODE == 0) {  // g[p0 + t][d]: d is contiguous
          dd = idx & 15, t = idx >> 4;
          if (d0 + dd < D && p0 + t < P) v = gs[(int64_t)(p0 + t) * N + d0 + dd];
        } else {          // g[d][q0 + t]: t is contiguous
          t = idx & 63, dd = idx >> 6;
          if (d0 + dd < D && q0 + t < Q) v = gs[(int64_t)(d0 + dd) * N + q0 + t];
        }
        sG[dd][t] = v;
      }
      if constexpr (!RESIDENT) stage_o(d0, 16, 0);
      __syncthreads();
      if (active) {
        const int ro = RESIDENT ? d0 : 0;
#pragma unroll
        for (int k2 = 0; k2 < 16; k2 += 2) {
          const float x = sG[k2 + (lane >> 5)][(MODE == 0 ? wi : wj) + (lane & 31)];
          const float y = sO[ro + k2 + (lane >> 5)][(MODE == 0 ? wj : wi) + (lane & 31)];
          acc = MODE == 0 ? __builtin_amdgcn_mfma_f32_32x32x2f32(x, y, acc, 0, 0, 0)
                          : __builtin_amdgcn_mfma_f32_32x32x2f32(y, x, acc, 0, 0, 0);
        }
      }
    }
    const int j = q0 + wj + (lane & 31);
    if (active && j < Q) {
      float* os = out + (s * NB + n) * ((int64_t)P * Q);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = p0 + wi + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (i < P) os[(int64_t)i * Q + j] = acc[r];
      }
    }
  }
}

// ---- host: the contract and the path of a shape ----------------------------------------------------------------------------------
struct MatmulPlan {
  int want_da, want_db;
  int res_da, res_db;      // the operand panel stays in LDS across the seeds (N / M <= MM_RES_DEPTH)
  int wide;                // an element offset of g or an output does not fit 31 bits (64-bit offsets throughout)
  int tq_da, tiles_da;     // tiles along K, tiles of one sample matrix
  int tq_db, tiles_db;     // tiles along N, tiles of one sample matrix
  int64_t blocks_da, blocks_db;  // workgroups of grid.x
  int64_t s_per;           // seeds per grid.y slice (one value for both launches)
};

// the shape part of the contract (shared with lk_matmul_vjp_variant), with the messages under the caller's name
static int matmul_check_shape(const char* fn, int64_t S, int64_t NB, int64_t M, int64_t K, int64_t N, bool want_da, bool want_db,
                              MatmulPlan* p) {
  LK_REQUIRE(want_da || want_db, "%s: no output (da and db are both null)", fn);
  const int64_t lim = 1ll << 24;
  LK_REQUIRE(S >= 1 && NB >= 0 && M >= 1 && K >= 1 && N >= 1 && M < lim && K < lim && N < lim,
             "%s: extent out of range (1 <= S, 0 <= NB, 1 <= M, K, N < 2^24)", fn);
  const unsigned __int128 sn = (unsigned __int128)S * (unsigned __int128)NB, cap = (unsigned __int128)1 << 40;
  LK_REQUIRE(sn * M * N < cap && sn * M * K < cap && sn * K * N < cap,
             "%s: extent out of range (S * NB * M * N, S * NB * M * K and S * NB * K * N < 2^40)", fn);
  const int64_t tm = (M + 63) / 64, tk = (K + 63) / 64, tn = (N + 63) / 64;
  LK_REQUIRE(tm * tk < (1ll << 31) && tk * tn < (1ll << 31) && NB * tm * tk < (1ll << 31) && NB * tk * tn < (1ll << 31),
             "%s: too many tiles (NB * ceil(M / 64) * ceil(K / 64) and NB * ceil(K / 64) * ceil(N / 64) < 2^31)", fn);
  p->want_da = want_da, p->want_db = want_db;
  p->res_da = N <= MM_RES_DEPTH, p->res_db = M <= MM_RES_DEPTH;
  const int64_t big = 1ll << 31;
  p->wide = S * NB * M * N >= big || S * NB * M * K >= big || S * NB * K * N >= big;
  p->tq_da = (int)tk, p->tiles_da = (int)(tm * tk), p->blocks_da = NB * tm * tk;
  p->tq_db = (int)tn, p->tiles_db = (int)(tk * tn), p->blocks_db = NB * tk * tn;
  int64_t fewest = want_da ? p->blocks_da : p->blocks_db;
  if (want_da && want_db && p->blocks_db < fewest) fewest = p->blocks_db;
  p->s_per = seeds_per_slice(S, fewest * 4);
  return LK_OK;
}

static int matmul_check(const float* g, const float* a, const float* b, int64_t S, int64_t NB, int64_t M, int64_t K, int64_t N,
                        const float* da, const float* db, MatmulPlan* p) {
  LK_REQUIRE(g && a && b, "lk_matmul_vjp_f32: null pointer");
  const int rc = matmul_check_shape("lk_matmul_vjp_f32", S, NB, M, K, N, da != nullptr, db != nullptr, p);
  if (rc != LK_OK) return rc;
  const unsigned __int128 ab = (unsigned __int128)NB * M * K * 4, bb = (unsigned __int128)NB * K * N * 4;
  const unsigned __int128 gb = (unsigned __int128)S * NB * M * N * 4, dab = ab * S, dbb = bb * S;
  bool clear = true;
  if (da) clear = clear && disjoint(da, dab, g, gb) && disjoint(da, dab, a, ab) && disjoint(da, dab, b, bb);
  if (db) clear = clear && disjoint(db, dbb, g, gb) && disjoint(db, dbb, a, ab) && disjoint(db, dbb, b, bb);
  LK_REQUIRE(clear, "lk_matmul_vjp_f32: an output overlaps an input");
  LK_REQUIRE(!(da && db) || disjoint(da, dab, db, dbb), "lk_matmul_vjp_f32: da overlaps db");
  return LK_OK;
}

}  // namespace lk

using namespace lk;

extern "C" int lk_matmul_vjp_f32(const float* g, const float* a, const float* b, int64_t S, int64_t NB, int64_t M, int64_t K,
                                 int64_t N, float* da, float* db, void* stream) {
  MatmulPlan p;
  const int rc = matmul_check(g, a, b, S, NB, M, K, N, da, db, &p);
  if (rc != LK_OK) return rc;
  if (NB == 0) return LK_OK;
  hipStream_t st = (hipStream_t)stream;
  const unsigned gy = (unsigned)((S + p.s_per - 1) / p.s_per);
#define LK_MM(MODE, RES, O, BLOCKS, TQ, TILES, OUT)                                                                           \
  hipLaunchKernelGGL((matmul_vjp_kernel<MODE, RES>), dim3((unsigned)(BLOCKS), gy), dim3(256), 0, st, g, O, S, NB, (int)M, (int)K, \
                     (int)N, TQ, TILES, p.s_per, OUT)
  if (da) {
    if (p.res_da) LK_MM(0, true, b, p.blocks_da, p.tq_da, p.tiles_da, da);
    else LK_MM(0, false, b, p.blocks_da, p.tq_da, p.tiles_da, da);
  }
  if (db) {
    if (p.res_db) LK_MM(1, true, a, p.blocks_db, p.tq_db, p.tiles_db, db);
    else LK_MM(1, false, a, p.blocks_db, p.tq_db, p.tiles_db, db);
  }
#undef LK_MM
  return check_launch("matmul_vjp_kernel");
}

// da << 0 | db << 1 | resident(da) << 2 | resident(db) << 3 | seed-split << 4 | wide << 5 | workgroups << 6
extern "C" int lk_matmul_vjp_variant(int64_t S, int64_t NB, int64_t M, int64_t K, int64_t N, int want_da, int want_db) {
  MatmulPlan p;
  if (matmul_check_shape("lk_matmul_vjp_variant", S, NB, M, K, N, want_da != 0, want_db != 0, &p) != LK_OK) return -1;
  int64_t wg = (want_da ? p.blocks_da : 0) + (want_db ? p.blocks_db : 0);
  if (wg > (1 << 24) - 1) wg = (1 << 24) - 1;
  return p.want_da | p.want_db << 1 | (p.want_da && p.res_da) << 2 | (p.want_db && p.res_db) << 3 | (p.s_per < S ? 1 : 0) << 4 |
         p.wide << 5 | (int)wg << 6;
}
