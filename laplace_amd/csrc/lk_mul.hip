// Element-wise product of two traced tensors (squeeze-and-excitation gates x * gate[B, C, 1, 1], GLU / SwiGLU / GeGLU
// silu(w1 x) * w3 x, self-gating h * sigmoid(h)) for the seed-batched reverse sweep.  With the cotangent g of out = a * b for all S
// seeds stacked, g [S][R][L], and ONE a [R][L] and b per sample row shared by all seeds:
//   full form (b_row == 0, b [R][L])   da[s][r][l] = g[s][r][l] * b[r][l]     db[s][r][l] = g[s][r][l] * a[r][l]
//   row gate  (b_row == 1, b [R])      da[s][r][l] = g[s][r][l] * b[r]        db[s][r]    = sum_l g[s][r][l] * a[r][l]
// Replaces, in the reverse pass of laplace/curvature/curvlinops.py:87-100 and curvature.py:88-129 through a product as stock torch
// runs it once per seed: g * b, g * a and - for a gate - a sum over the trailing dims, five passes over [S*B, ...] tensors.  Here
// one launch serves all seeds, g is read ONCE for both outputs, and a and b are read once per sample row and stay in registers
// across the seed loop.
//
// One kernel template (vector access, grid cap and overlap check: lk_stream.h), two bodies:
//   * row gate: a group of W lanes (a power of two <= 64, so a group never leaves its wave) owns one row; the row sum is a fixed
//     xor-shuffle tree over the group, lane 0 of the group stores it.  a of the row stays in registers while the row fits
//     (MUL_NV vectors per lane: RESIDENT); longer rows re-read it per seed.  The grid strides over the rows with at most
//     STREAM_MAX_BLOCKS workgroups.
//   * full form: the same without the tree - a lane owns one vector of the flattened [R * L] and keeps its a and b.
// 16-byte loads and stores where L % 4 == 0 and every pointer is 16-byte aligned, 4-byte ones otherwise.  Few rows: the seeds
// are split over grid.y (a and b are then read once per slice).  Every output element has one owner, stores are plain vector
// stores, there is no atomic: repeated runs give the same bits.  Plain fp32: one rounding per product (da, and db of the full
// form, equal the fp32 product exactly); the row sum adds in a fixed order.  Nothing assumes packed fp32.
// Minimal traffic: g once (4 S R L bytes), a and b once, and the outputs asked for.
#include "lk_stream.h"

namespace lk {

constexpr int MUL_NV = 8;  // vectors of a row a lane keeps in registers (RESIDENT)

// da / db may be null (uniform over the grid); `seed_stride` = R * L; `units`: rows (ROW) or vectors of the flattened [R * L]
template <int VEC, bool ROW, bool RESIDENT>
__global__ __launch_bounds__(256) void mul_vjp_kernel(const float* __restrict__ g, const float* __restrict__ a,
                                                      const float* __restrict__ b, int64_t S, int64_t R, int L, int W,
                                                      int64_t s_per, int64_t units, float* __restrict__ da,
                                                      float* __restrict__ db) {
  const int64_t seed_stride = R * (int64_t)L;
  const int64_t s_begin = (int64_t)blockIdx.y * s_per;
  const int64_t s_end = s_begin + s_per < S ? s_begin + s_per : S;
  if constexpr (!ROW) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < units; t += (int64_t)gridDim.x * 256) {
      const int64_t o = t * VEC;
      float av[VEC], bv[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) av[e] = bv[e] = 0.f;
      if (db != nullptr) ld<VEC>(a + o, av);
      if (da != nullptr) ld<VEC>(b + o, bv);
#pragma unroll 2
      for (int64_t s = s_begin; s < s_end; ++s) {
        float gv[VEC], d[VEC];
        ld<VEC>(g + s * seed_stride + o, gv);
        if (da != nullptr) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) d[e] = gv[e] * bv[e];
          st<VEC>(da + s * seed_stride + o, d);
        }
        if (db != nullptr) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) d[e] = gv[e] * av[e];
          st<VEC>(db + s * seed_stride + o, d);
        }
      }
    }
  } else {
    const int rpb = 256 / W;  // rows per workgroup
    const int lane = threadIdx.x & (W - 1);
    const int nvec_row = L / VEC;
    // (the trip count is uniform over the workgroup: dead groups stay in the shuffles and touch no memory)
    for (int64_t row0 = (int64_t)blockIdx.x * rpb; row0 < units; row0 += (int64_t)gridDim.x * rpb) {
      const int64_t row = row0 + threadIdx.x / W;
      const bool live = row < R;
      const int nvec = live ? nvec_row : 0;
      const int64_t base = (live ? row : 0) * (int64_t)L;
      const float bv = live ? b[row] : 0.f;
      if constexpr (RESIDENT) {
        float av[MUL_NV][VEC];
#pragma unroll
        for (int k = 0; k < MUL_NV; ++k) {
          const int i = k * W + lane;
#pragma unroll
          for (int e = 0; e < VEC; ++e) av[k][e] = 0.f;
          if (db != nullptr && i < nvec) ld<VEC>(a + base + (int64_t)i * VEC, av[k]);
        }
        for (int64_t s = s_begin; s < s_end; ++s) {
          const float* gs = g + s * seed_stride + base;
          float acc = 0.f;
#pragma unroll
          for (int k = 0; k < MUL_NV; ++k) {
            const int i = k * W + lane;
            if (i < nvec) {
              float gv[VEC], d[VEC];
              ld<VEC>(gs + (int64_t)i * VEC, gv);
#pragma unroll
              for (int e = 0; e < VEC; ++e) {
                d[e] = gv[e] * bv;
                acc += gv[e] * av[k][e];
              }
              if (da != nullptr) st<VEC>(da + s * seed_stride + base + (int64_t)i * VEC, d);
            }
          }
          if (db != nullptr) {
            for (int o = W >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
            if (live && lane == 0) db[s * R + row] = acc;
          }
        }
      } else {
        for (int64_t s = s_begin; s < s_end; ++s) {
          const float* gs = g + s * seed_stride + base;
          float acc = 0.f;
#pragma unroll 4
          for (int i = lane; i < nvec; i += W) {  // (nvec < 2^30 and W <= 64: no overflow)
            float gv[VEC], av[VEC], d[VEC];
            ld<VEC>(gs + (int64_t)i * VEC, gv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) av[e] = 0.f;
            if (db != nullptr) ld<VEC>(a + base + (int64_t)i * VEC, av);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              d[e] = gv[e] * bv;
              acc += gv[e] * av[e];
            }
            if (da != nullptr) st<VEC>(da + s * seed_stride + base + (int64_t)i * VEC, d);
          }
          if (db != nullptr) {
            for (int o = W >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
            if (live && lane == 0) db[s * R + row] = acc;
          }
        }
      }
    }
  }
}

// ---- host: the contract and the path of a shape ----------------------------------------------------------------------------------
struct MulPlan {
  int row;       // 1: row gate, 0: full form
  int vec;       // 16-byte accesses
  int W;         // row gate: lanes per row (1 in the full form)
  int resident;  // a of a row stays in registers (always in the full form: one vector per lane)
  int wide;      // an element offset of g does not fit 31 bits (the kernel indexes with 64 bits throughout)
  int64_t s_per; // seeds per grid.y slice
  int64_t units; // rows, or vectors of the flattened [R * L]
  int64_t blocks;
};

// the shape part of the contract (shared with lk_mul_variant), with the messages under the caller's name
static int mul_check_shape(const char* fn, int64_t S, int64_t R, int64_t L, int b_row, bool want_da, bool want_db, bool aligned,
                           MulPlan* p) {
  LK_REQUIRE(b_row == 0 || b_row == 1, "%s: b_row must be 0 (b is [R][L]) or 1 (b is [R])", fn);
  LK_REQUIRE(want_da || want_db, "%s: no output (da and db are both null)", fn);
  LK_REQUIRE(S >= 1 && R >= 0 && L >= 1 && L < (1ll << 30), "%s: extent out of range (1 <= S, 0 <= R, 1 <= L < 2^30)", fn);
  LK_REQUIRE((unsigned __int128)S * (unsigned __int128)R * (unsigned __int128)L < ((unsigned __int128)1 << 40),
             "%s: extent out of range (S * R * L < 2^40)", fn);
  p->row = b_row;
  p->vec = aligned && L % 4 == 0;
  p->wide = S * R * L >= (1ll << 31);
  const int64_t nvec = p->vec ? L / 4 : L;
  if (b_row) {
    p->W = pow2_ceil(nvec, 64);
    p->resident = nvec <= (int64_t)p->W * MUL_NV;
    p->units = R;
    const int rpb = 256 / p->W;
    p->blocks = (R + rpb - 1) / rpb;
  } else {
    p->W = 1;
    p->resident = 1;
    p->units = R * nvec;
    p->blocks = (p->units + 255) / 256;
  }
  if (p->blocks > STREAM_MAX_BLOCKS) p->blocks = STREAM_MAX_BLOCKS;
  p->s_per = seeds_per_slice(S, p->blocks * 4);
  return LK_OK;
}

static int mul_check(const float* g, const float* a, const float* b, int64_t S, int64_t R, int64_t L, int b_row, const float* da,
                     const float* db, MulPlan* p) {
  LK_REQUIRE(g && a && b, "lk_mul_vjp_f32: null pointer");
  const uintptr_t bits = (uintptr_t)g | (uintptr_t)a | (uintptr_t)b | (uintptr_t)da | (uintptr_t)db;
  const int rc = mul_check_shape("lk_mul_vjp_f32", S, R, L, b_row, da != nullptr, db != nullptr, (bits & 15) == 0, p);
  if (rc != LK_OK) return rc;
  const unsigned __int128 rl = (unsigned __int128)R * L * 4, gb = rl * S, bb = b_row ? (unsigned __int128)R * 4 : rl;
  const unsigned __int128 dbb = b_row ? (unsigned __int128)S * R * 4 : gb;
  bool clear = true;
  if (da) clear = clear && disjoint(da, gb, g, gb) && disjoint(da, gb, a, rl) && disjoint(da, gb, b, bb);
  if (db) clear = clear && disjoint(db, dbb, g, gb) && disjoint(db, dbb, a, rl) && disjoint(db, dbb, b, bb);
  LK_REQUIRE(clear, "lk_mul_vjp_f32: an output overlaps an input");
  LK_REQUIRE(!(da && db) || disjoint(da, gb, db, dbb), "lk_mul_vjp_f32: da overlaps db");
  return LK_OK;
}

}  // namespace lk

using namespace lk;

extern "C" int lk_mul_vjp_f32(const float* g, const float* a, const float* b, int64_t S, int64_t R, int64_t L, int b_row,
                              float* da, float* db, void* stream) {
  MulPlan p;
  const int rc = mul_check(g, a, b, S, R, L, b_row, da, db, &p);
  if (rc != LK_OK) return rc;
  if (R == 0) return LK_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)p.blocks, (unsigned)((S + p.s_per - 1) / p.s_per));
#define LK_MUL(V, ROW, RES)                                                                                                  \
  hipLaunchKernelGGL((mul_vjp_kernel<V, ROW, RES>), grid, dim3(256), 0, st, g, a, b, S, R, (int)L, p.W, p.s_per, p.units, da, db)
  if (!p.row) {
    if (p.vec) LK_MUL(4, false, true);
    else LK_MUL(1, false, true);
  } else if (p.vec) {
    if (p.resident) LK_MUL(4, true, true);
    else LK_MUL(4, true, false);
  } else {
    if (p.resident) LK_MUL(1, true, true);
    else LK_MUL(1, true, false);
  }
#undef LK_MUL
  return check_launch("mul_vjp_kernel");
}

// form | vec << 1 | log2(lanes per row) << 2 | resident << 5 | seed-split << 6 | wide << 7 | da << 8 | db << 9 | workgroups << 10
extern "C" int lk_mul_variant(int64_t S, int64_t R, int64_t L, int b_row, int want_da, int want_db, int aligned) {
  MulPlan p;
  if (mul_check_shape("lk_mul_variant", S, R, L, b_row, want_da != 0, want_db != 0, aligned != 0, &p) != LK_OK) return -1;
  int lg = 0;
  while ((1 << lg) < p.W) ++lg;
  return p.row | p.vec << 1 | lg << 2 | p.resident << 5 | (p.s_per < S ? 1 : 0) << 6 | p.wide << 7 | (want_da ? 1 : 0) << 8 |
         (want_db ? 1 : 0) << 9 | (int)p.blocks << 10;
}
