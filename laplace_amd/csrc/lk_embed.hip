// Per-sample Jacobian, diagonal GGN / EF and diagonal GLM predictive of an nn.Embedding weight W[V][D] for all seeds of a
// reverse sweep.  With token ids ids[B][T] and the cotangent g[S][B][T][D] of the module's output the Jacobian is a segmented sum:
//   J[b][s][v*D + d] = sum over {t : ids[b][t] == v} of g[s][b][t][d]
// Replaces the embedding columns of the jacrev materialisation of CurvatureInterface.jacobians
// (laplace/curvature/curvature.py:88-129) and, without forming them, of GGNInterface.diag / EFInterface.diag
// (curvature.py:413-433, 494-505) and of the diagonal functional variance (laplace/baselaplace.py, DiagLaplace).
//
// The hazards are a token repeated inside a row and one token in many rows.  Nothing here adds into memory that another thread
// may add into: torch sorts the ids (stable), equal ids become a RUN of adjacent sorted positions, and the thread group at the
// first position of a run (the run HEAD: position 0, or a key that differs from the position before it) walks the run; every
// other group exits.  One owner per output element, ascending t then ascending b, no atomics: two launches give the same bits.
// No host sync, no compaction: heads are found from the sorted keys alone.
//
// Lanes run across d (a row of g is D contiguous floats): 16-byte accesses where D % 4 == 0 and every pointer / row pitch is
// 16-byte aligned, 4-byte otherwise.  These are streaming kernels: bytes that must move = 4 * S*B*T*D of g once.
#include "lk_stream.h"

namespace lk {

// a token id the kernels write for: inside the table and not the padding row (the host never sees the ids)
__device__ __forceinline__ bool emb_live(int64_t id, int V, int64_t pad) { return id >= 0 && id < V && id != pad; }

// the sample of sorted position j (flattened b-major position order[j]); -1 for an index outside [0, N)
__device__ __forceinline__ int emb_row(const int64_t* __restrict__ order, int64_t j, int N, int T) {
  const int64_t o = order[j];
  return (o >= 0 && o < N) ? (int)o / T : -1;
}

// seeds whose loads a lane keeps in flight together: the heads are found through a chain of dependent loads of the keys, so
// a wave must move more than one row of g per head to hide it.  The seed index is CLAMPED, never branched on (a branch around
// each load would make the compiler wait for every load before the next)
constexpr int EMB_SC = 4;

// ---- Jacobian: a wave per sorted position; the head of an (id, b) run sums it for the seeds of its grid.y slice ----
template <int VEC>
__global__ __launch_bounds__(256) void jac_embed_kernel(const float* __restrict__ g, const int64_t* __restrict__ order,
                                                        const int64_t* __restrict__ sid, int S, int s_per, int N, int T, int D,
                                                        int V, int64_t pad, float* __restrict__ Js, int64_t P, int64_t col0) {
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (j >= N) return;
  const int64_t id = sid[j];
  if (!emb_live(id, V, pad)) return;
  const int b = emb_row(order, j, N, T);
  if (b < 0) return;
  if (j > 0 && sid[j - 1] == id && emb_row(order, j - 1, N, T) == b) return;  // not a run head
  int64_t e = j + 1;  // (a run lies inside one row: at most T positions)
  while (e < N && sid[e] == id && emb_row(order, e, N, T) == b) ++e;
  const int s_end = (int)min((int64_t)S, ((int64_t)blockIdx.y + 1) * s_per);
  const int64_t seed = (int64_t)N * D;
  float* out = Js + (int64_t)b * S * P + col0 + id * D;
  for (int s0 = (int)blockIdx.y * s_per; s0 < s_end; s0 += EMB_SC) {  // (grid.y * s_per >= S > blockIdx.y * s_per)
    for (int d = lane * VEC; d < D; d += 64 * VEC) {
      float acc[EMB_SC][VEC];
#pragma unroll
      for (int u = 0; u < EMB_SC; ++u)
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[u][k] = 0.f;
      for (int64_t q = j; q < e; ++q) {
        const float* gq = g + order[q] * D + d;
        float v[EMB_SC][VEC];
#pragma unroll
        for (int u = 0; u < EMB_SC; ++u) ld<VEC>(gq + min(s0 + u, s_end - 1) * seed, v[u]);
#pragma unroll
        for (int u = 0; u < EMB_SC; ++u)
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[u][k] += v[u][k];
      }
#pragma unroll
      for (int u = 0; u < EMB_SC; ++u)
        if (s0 + u < s_end) st<VEC>(out + (int64_t)(s0 + u) * P + d, acc[u]);
    }
  }
}

// ---- diagonal: a workgroup per sorted position; the head of an id run (across all samples) owns h[id*D ...] ----
// DL lanes (a power of two <= 16: 256 contiguous bytes of a row with 16-byte accesses) across the d vectors of grid.y's chunk,
// R = 1024 / DL >= 64 row slots: a frequent token is one long run, which the slots of every chunk's workgroup share.  The run [j, j1) is cut into
// R equal position ranges; slot r sums the (id, b) sub-runs whose first position lies in its range (it walks past the range's
// end to finish one), squares each per seed and accumulates.  The slots are then added through LDS in ascending r.
constexpr int EMB_DIAG_THREADS = 1024, EMB_DIAG_LANES = 16;

template <int VEC>
__global__ __launch_bounds__(EMB_DIAG_THREADS) void diag_embed_kernel(const float* __restrict__ g,
                                                                      const int64_t* __restrict__ order,
                                                                      const int64_t* __restrict__ sid, int S, int N, int T, int D,
                                                                      int V, int64_t pad, float alpha, float* __restrict__ h,
                                                                      int DL) {
  __shared__ float red[EMB_DIAG_THREADS * VEC];
  const int64_t j = blockIdx.x;
  const int64_t id = sid[j];
  if (!emb_live(id, V, pad)) return;         // (uniform over the workgroup)
  if (j > 0 && sid[j - 1] == id) return;     // not a run head
  int64_t lo = j + 1, hi = N;                // the ids are sorted: first position past the run
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (sid[mid] == id) lo = mid + 1; else hi = mid;
  }
  const int64_t j1 = lo, len = j1 - j;
  const int R = EMB_DIAG_THREADS / DL, r = threadIdx.x / DL, l = threadIdx.x & (DL - 1);
  const int d = (blockIdx.y * DL + l) * VEC;
  const bool active = d < D;
  const int64_t seed = (int64_t)N * D;
  float acc[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
  if (active) {
    const int64_t c0 = j + len * r / R, c1 = j + len * (r + 1) / R;
    int64_t p = c0;
    while (p < c1) {
      const int b = emb_row(order, p, N, T);
      if (b < 0 || (p > j && emb_row(order, p - 1, N, T) == b)) {  // inside a sub-run that an earlier position heads
        ++p;
        continue;
      }
      int64_t q = p + 1;
      while (q < j1 && emb_row(order, q, N, T) == b) ++q;
      for (int s0 = 0; s0 < S; s0 += EMB_SC) {
        float sum[EMB_SC][VEC];
#pragma unroll
        for (int u = 0; u < EMB_SC; ++u)
#pragma unroll
          for (int k = 0; k < VEC; ++k) sum[u][k] = 0.f;
        for (int64_t x = p; x < q; ++x) {
          const float* gx = g + order[x] * D + d;
          float v[EMB_SC][VEC];
#pragma unroll
          for (int u = 0; u < EMB_SC; ++u) ld<VEC>(gx + min(s0 + u, S - 1) * seed, v[u]);
#pragma unroll
          for (int u = 0; u < EMB_SC; ++u)
#pragma unroll
            for (int k = 0; k < VEC; ++k) sum[u][k] += v[u][k];
        }
#pragma unroll
        for (int u = 0; u < EMB_SC; ++u)
          if (s0 + u < S)  // (uniform; ascending s)
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] += sum[u][k] * sum[u][k];
      }
      p = q;
    }
  }
#pragma unroll
  for (int k = 0; k < VEC; ++k) red[threadIdx.x * VEC + k] = acc[k];
  __syncthreads();
  if (r == 0 && active) {
    float tot[VEC], old[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) tot[k] = 0.f;
    for (int rr = 0; rr < R; ++rr)
#pragma unroll
      for (int k = 0; k < VEC; ++k) tot[k] += red[(rr * DL + l) * VEC + k];
    float* hp = h + id * D + d;
    ld<VEC>(hp, old);
#pragma unroll
    for (int k = 0; k < VEC; ++k) old[k] += alpha * tot[k];
    st<VEC>(hp, old);
  }
}

// ---- diagonal predictive: a workgroup per sample; ids sorted per row (order_row: positions t of the row) ----
// fvar[b][c][k] += sum over the row's runs, over d, of r_c[d] * r_k[d] * var[id*D + d], r_c the run sum of class c.  The (c, k)
// pairs are tiled QC x QK; the QC + QK run sums of a lane's d vector sit in registers.  Wave w owns the sorted positions
// p = w, w + 4, ...; a fixed xor-shuffle tree reduces the lanes, the four waves are added through LDS in ascending order.
constexpr int EMB_QC = 16, EMB_QK = 4;

template <int VEC>
__global__ __launch_bounds__(256) void diag_quadform_embed_kernel(const float* __restrict__ g,
                                                                  const int64_t* __restrict__ order_row,
                                                                  const int64_t* __restrict__ sid_row, int C, int B, int T, int D,
                                                                  int V, int64_t pad, const float* __restrict__ var,
                                                                  float* __restrict__ fvar) {
  __shared__ float red[4][EMB_QC * EMB_QK];
  const int b = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t* ord = order_row + (int64_t)b * T;
  const int64_t* sid = sid_row + (int64_t)b * T;
  const int64_t cls = (int64_t)B * T * D;  // stride of a class in g
  const float* gb = g + (int64_t)b * T * D;
  for (int c0 = 0; c0 < C; c0 += EMB_QC) {
    for (int k0 = 0; k0 < C; k0 += EMB_QK) {
      float acc[EMB_QC][EMB_QK];
#pragma unroll
      for (int i = 0; i < EMB_QC; ++i)
#pragma unroll
        for (int jj = 0; jj < EMB_QK; ++jj) acc[i][jj] = 0.f;
      for (int p = w; p < T; p += 4) {
        const int64_t id = sid[p];
        if (!emb_live(id, V, pad) || (p > 0 && sid[p - 1] == id)) continue;
        int q = p + 1;
        while (q < T && sid[q] == id) ++q;
        for (int d = lane * VEC; d < D; d += 64 * VEC) {
          float rc[EMB_QC][VEC], rk[EMB_QK][VEC], vv[VEC];
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
#pragma unroll
            for (int i = 0; i < EMB_QC; ++i) rc[i][e] = 0.f;
#pragma unroll
            for (int jj = 0; jj < EMB_QK; ++jj) rk[jj][e] = 0.f;
          }
          for (int x = p; x < q; ++x) {
            const int64_t t = ord[x];
            if (t < 0 || t >= T) continue;
            const float* gt = gb + t * D + d;
#pragma unroll
            for (int i = 0; i < EMB_QC; ++i) {
              if (c0 + i < C) {
                float v[VEC];
                ld<VEC>(gt + (c0 + i) * cls, v);
#pragma unroll
                for (int e = 0; e < VEC; ++e) rc[i][e] += v[e];
              }
            }
#pragma unroll
            for (int jj = 0; jj < EMB_QK; ++jj) {
              if (k0 + jj < C) {
                float v[VEC];
                ld<VEC>(gt + (k0 + jj) * cls, v);
#pragma unroll
                for (int e = 0; e < VEC; ++e) rk[jj][e] += v[e];
              }
            }
          }
          ld<VEC>(var + id * D + d, vv);
#pragma unroll
          for (int e = 0; e < VEC; ++e)
#pragma unroll
            for (int i = 0; i < EMB_QC; ++i)
#pragma unroll
              for (int jj = 0; jj < EMB_QK; ++jj) acc[i][jj] += rc[i][e] * rk[jj][e] * vv[e];
        }
      }
#pragma unroll
      for (int i = 0; i < EMB_QC; ++i)
#pragma unroll
        for (int jj = 0; jj < EMB_QK; ++jj) {
          const float v = wave_sum(acc[i][jj]);
          if (lane == 0) red[w][i * EMB_QK + jj] = v;
        }
      __syncthreads();
      if (threadIdx.x < EMB_QC * EMB_QK) {
        const int i = threadIdx.x / EMB_QK, jj = threadIdx.x % EMB_QK;
        if (c0 + i < C && k0 + jj < C) {
          const float tot = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
          fvar[((int64_t)b * C + c0 + i) * C + k0 + jj] += tot;
        }
      }
      __syncthreads();
    }
  }
}

struct EmbedPlan {
  int vec;     // floats per access: 4 or 1
  int DL;      // lanes across the d vectors of the diagonal kernel
  int slots;   // its row slots: the parts a long run is cut into
  int chunks;  // its grid.y
};

static inline bool emb_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

static void embed_plan(int64_t D, bool aligned, EmbedPlan* p) {
  p->vec = (D % 4 == 0 && aligned) ? 4 : 1;
  const int64_t units = D / p->vec;
  p->DL = pow2_ceil(units, EMB_DIAG_LANES);
  p->slots = EMB_DIAG_THREADS / p->DL;
  p->chunks = (int)((units + p->DL - 1) / p->DL);
}

// Every argument check of the three entry points, before the first HIP call (the extern "C" bodies hold none): the contract they
// share (S: seeds or classes) and, below, what each adds; the checkers fill the launch plan.
static int embed_check(const char* who, const void* g, const void* order, const void* sid, const void* out, int64_t S, int64_t B,
                       int64_t T, int64_t D, int64_t V) {
  LK_REQUIRE(S >= 1 && S < (1ll << 31) && B >= 0 && T >= 1 && D >= 1 && V >= 1,
             "%s: bad extents (1 <= S < 2^31, 0 <= B, 1 <= T, 1 <= D, 1 <= V)", who);
  LK_REQUIRE(B == 0 || (g && order && sid && out), "%s: null pointer", who);  // (an empty batch has no storage to point to)
  LK_REQUIRE(B < (1ll << 31) && T < (1ll << 31) && D < (1ll << 31) && V < (1ll << 31) && B * T < (1ll << 31) &&
                 V * D < (1ll << 31),
             "%s: extent too large (B*T < 2^31, V*D < 2^31)", who);
  return LK_OK;
}

static int jac_embed_check(const float* g, const int64_t* order, const int64_t* sid, int64_t S, int64_t B, int64_t T, int64_t D,
                           int64_t V, const float* Js, int64_t P, int64_t col0, EmbedPlan* p) {
  const int rc = embed_check("lk_jac_embed_f32", g, order, sid, Js, S, B, T, D, V);
  if (rc != LK_OK) return rc;
  LK_REQUIRE(col0 >= 0 && col0 + V * D <= P, "lk_jac_embed_f32: column range outside Js (0 <= col0, col0 + V*D <= P)");
  embed_plan(D, emb_aligned(g) && emb_aligned(Js) && P % 4 == 0 && col0 % 4 == 0, p);
  return LK_OK;
}

static int diag_embed_check(const float* g, const int64_t* order, const int64_t* sid, int64_t S, int64_t B, int64_t T, int64_t D,
                            int64_t V, const float* h, EmbedPlan* p) {
  const int rc = embed_check("lk_diag_embed_f32", g, order, sid, h, S, B, T, D, V);
  if (rc != LK_OK) return rc;
  embed_plan(D, emb_aligned(g) && emb_aligned(h), p);
  LK_REQUIRE(p->chunks <= 65535, "lk_diag_embed_f32: D too large for grid.y (at most 65535 * 16 vectors of d)");
  return LK_OK;
}

static int quad_embed_check(const float* g, const int64_t* order, const int64_t* sid, int64_t C, int64_t B, int64_t T, int64_t D,
                            int64_t V, const float* var, const float* fvar, EmbedPlan* p) {
  const int rc = embed_check("lk_diag_quadform_embed_f32", g, order, sid, fvar, C, B, T, D, V);
  if (rc != LK_OK) return rc;
  LK_REQUIRE(B == 0 || var, "lk_diag_quadform_embed_f32: null pointer (var)");
  LK_REQUIRE(C <= 32768, "lk_diag_quadform_embed_f32: too many classes (C <= 32768: C*C < 2^31)");
  embed_plan(D, emb_aligned(g) && emb_aligned(var), p);
  return LK_OK;
}

}  // namespace lk

using namespace lk;

extern "C" int lk_embed_variant(int64_t S, int64_t B, int64_t T, int64_t D, int aligned) {
  if (!(S >= 1 && S < (1ll << 31) && B >= 0 && T >= 1 && D >= 1 && B < (1ll << 31) && T < (1ll << 31) && D < (1ll << 31) &&
        B * T < (1ll << 31)))
    return -1;
  EmbedPlan p;
  embed_plan(D, aligned != 0, &p);
  return (p.vec == 4 ? 1 : 0) | p.slots << 1 | p.DL << 12 | (p.chunks > 2047 ? 2047 : p.chunks) << 20;
}

extern "C" int lk_jac_embed_f32(const float* g, const int64_t* order, const int64_t* sorted_ids, int64_t S, int64_t B, int64_t T,
                                int64_t D, int64_t V, int64_t padding_idx, float* Js, int64_t P, int64_t col0, void* stream) {
  EmbedPlan p;
  const int rc = jac_embed_check(g, order, sorted_ids, S, B, T, D, V, Js, P, col0, &p);
  if (rc != LK_OK) return rc;
  if (B == 0) return LK_OK;
  const int N = (int)(B * T);
  const int s_per = seeds_per_slice(S, N);  // (all seeds in one wave unless the positions alone leave the device short of waves)
  const dim3 grid((unsigned)(((int64_t)N + 3) / 4), (unsigned)((S + s_per - 1) / s_per));
  if (p.vec == 4)
    hipLaunchKernelGGL(jac_embed_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, g, order, sorted_ids, (int)S, s_per, N,
                       (int)T, (int)D, (int)V, padding_idx, Js, P, col0);
  else
    hipLaunchKernelGGL(jac_embed_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, g, order, sorted_ids, (int)S, s_per, N,
                       (int)T, (int)D, (int)V, padding_idx, Js, P, col0);
  return check_launch("jac_embed_kernel");
}

extern "C" int lk_diag_embed_f32(const float* g, const int64_t* order, const int64_t* sorted_ids, int64_t S, int64_t B, int64_t T,
                                 int64_t D, int64_t V, int64_t padding_idx, float alpha, float* h, void* stream) {
  EmbedPlan p;
  const int rc = diag_embed_check(g, order, sorted_ids, S, B, T, D, V, h, &p);
  if (rc != LK_OK) return rc;
  if (B == 0) return LK_OK;
  const int N = (int)(B * T);
  const dim3 grid((unsigned)N, (unsigned)p.chunks);
  if (p.vec == 4)
    hipLaunchKernelGGL(diag_embed_kernel<4>, grid, dim3(EMB_DIAG_THREADS), 0, (hipStream_t)stream, g, order, sorted_ids, (int)S, N,
                       (int)T, (int)D, (int)V, padding_idx, alpha, h, p.DL);
  else
    hipLaunchKernelGGL(diag_embed_kernel<1>, grid, dim3(EMB_DIAG_THREADS), 0, (hipStream_t)stream, g, order, sorted_ids, (int)S, N,
                       (int)T, (int)D, (int)V, padding_idx, alpha, h, p.DL);
  return check_launch("diag_embed_kernel");
}

extern "C" int lk_diag_quadform_embed_f32(const float* g, const int64_t* order_row, const int64_t* sorted_ids_row, int64_t C,
                                          int64_t B, int64_t T, int64_t D, int64_t V, int64_t padding_idx, const float* var,
                                          float* fvar, void* stream) {
  EmbedPlan p;
  const int rc = quad_embed_check(g, order_row, sorted_ids_row, C, B, T, D, V, var, fvar, &p);
  if (rc != LK_OK) return rc;
  if (B == 0) return LK_OK;
  if (p.vec == 4)
    hipLaunchKernelGGL(diag_quadform_embed_kernel<4>, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, g, order_row,
                       sorted_ids_row, (int)C, (int)B, (int)T, (int)D, (int)V, padding_idx, var, fvar);
  else
    hipLaunchKernelGGL(diag_quadform_embed_kernel<1>, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, g, order_row,
                       sorted_ids_row, (int)C, (int)B, (int)T, (int)D, (int)V, padding_idx, var, fvar);
  return check_launch("diag_quadform_embed_kernel");
}
