// Squeeze-and-excitation gate out = x * gate[B, C, 1, 1] on NHWC feature maps for the NHWC reverse sweep (SE-ResNet, MobileNetV3,
// EfficientNet, RegNetY blocks).  N = S B maps, seed-major; P = H W positions; C channels innermost.  The cotangent g of the
// product, [N][P][C], is an fp32 map or the two fp16 planes of a ONE-scale split tensor read as it lies:
// value = (float(h) + float(l)) * 2^-sexp[0], exactly as lk_cat_vjp_nhwc_f32 and SplitTensor.float() form it.
//   reduce  ds[s][b][c]    = sum_p g[s B + b][p][c] * x[b][p][c]               x [B][P][C], one copy per sample for all seeds
//   VJP     dx[s B + b][p][c] = g[s B + b][p][c] * gate[b][c] + r[s B + b][c]  gate [B][C]; r [N][C] or null: the cotangent of
//           the pooled tensor, already divided by P (the AdaptiveAvgPool2d(1) that opens the gate branch reads the same map)
// Replaces, on the NHWC sweep, the reverse pass of laplace/curvature/curvlinops.py:87-100 through such a block as the NCHW route
// runs it: lk_mul_vjp_f32 on an NCHW copy, the pooling cotangent expanded to [N][P][C], and the add of the two.
//
// One thread layout for both kernels: a workgroup of 256 threads is CL lanes across the channel vectors (a power of two <= 64)
// times PG = 256 / CL position groups, so that the lanes of a position read adjacent addresses and - where CL covers the C of a
// position - the whole workgroup one contiguous stretch.  16-byte fp32 accesses (8-byte ones of four halves) where C % 4 == 0 and
// every base is aligned, 4-byte ones (2-byte of the planes) otherwise.
//   * reduce: a workgroup owns one (sample, tile of CL channel vectors); a thread adds its positions p = pg, pg + PG, ... in that
//     order in fp32, the PG partial sums meet in a fixed tree over LDS, position group 0 stores.  x of the thread's positions stays
//     in registers across the seed loop while there are at most GATE_NV of them (RESIDENT); otherwise it is re-read per seed.
//     Few (sample, tile) units: the seeds go over grid.y (x is then read once per slice).
//   * VJP: a workgroup owns (map, channel tile, chunk of PG * GATE_PP positions); gate of the sample and r of the map are loaded
//     once per unit and stay in registers along the positions.  max|dx| goes to `amax` as the bit pattern of a non-negative
//     float, at most one atomicMax per workgroup (one that cannot raise the word only reads it).
// Every output element has one owner, stores are plain vector stores, the sums run in a fixed order, no atomic touches data:
// repeated runs give the same bits.  With r null dx is the fp32 product (one rounding).  Offsets are 64-bit throughout.
// Minimal traffic: g once, x / gate (and r) once per sample (map), the outputs once.
#include "lk_stream.h"

namespace lk {

constexpr int GATE_NV = 16;  // positions of x a thread keeps in registers (RESIDENT)
constexpr int GATE_PP = 8;   // positions a thread of the VJP walks per unit

struct GateG {  // the cotangent: f32 non-null, or the planes with their scale word
  const float* f32;
  const _Float16* h;
  const _Float16* l;
  const int* sexp;
};

// VEC adjacent channels of g at element offset `at`; scale is a power of two, so the product is exact
template <int VEC, bool SPLIT>
__device__ __forceinline__ void gate_ld_g(const GateG& G, int64_t at, float scale, float (&v)[VEC]) {
  if constexpr (!SPLIT) {
    ld<VEC>(G.f32 + at, v);
  } else {
    ld_split<VEC>(G.h + at, G.l + at, scale, v);
  }
}

// ---- reduce: ds[s][b][c] = sum_p g[s B + b][p][c] x[b][p][c] --------------------------------------------------------------------
// `nvc`: channel vectors of a position (C / VEC); `tiles`: tiles of CL of them; `units` = B * tiles
template <int VEC, bool SPLIT, bool RESIDENT>
__global__ __launch_bounds__(256) void gate_reduce_kernel(GateG G, const float* __restrict__ x, int64_t S, int64_t B, int P, int C,
                                                          int CL, int nvc, int tiles, int64_t s_per, int64_t units,
                                                          float* __restrict__ ds) {
  __shared__ float red[256 * VEC];
  const int PG = 256 / CL;
  const int cl = threadIdx.x & (CL - 1), pg = threadIdx.x / CL;
  const float scale = SPLIT ? ldexpf(1.f, -G.sexp[0]) : 1.f;
  const int64_t s_begin = (int64_t)blockIdx.y * s_per;
  const int64_t s_end = s_begin + s_per < S ? s_begin + s_per : S;
  const int64_t map = (int64_t)P * C;
  // (every trip count below is uniform over the workgroup: dead lanes stay in the barriers and touch no memory)
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t b = u / tiles;
    const int cvi = (int)(u - b * tiles) * CL + cl;
    const bool live = cvi < nvc;
    const int np = live ? P : 0;  // (a dead lane walks no position)
    const int64_t xo = b * map + (int64_t)cvi * VEC;
    float xv[RESIDENT ? GATE_NV : 1][VEC];
    if constexpr (RESIDENT) {
#pragma unroll
      for (int k = 0; k < GATE_NV; ++k) {
        const int p = pg + k * PG;
#pragma unroll
        for (int e = 0; e < VEC; ++e) xv[k][e] = 0.f;
        if (p < np) ld<VEC>(x + xo + (int64_t)p * C, xv[k]);
      }
    }
    for (int64_t s = s_begin; s < s_end; ++s) {
      const int64_t go = (s * B + b) * map + (int64_t)cvi * VEC;
      float acc[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
      if constexpr (RESIDENT) {
#pragma unroll
        for (int k = 0; k < GATE_NV; ++k) {
          const int p = pg + k * PG;
          if (p < np) {
            float gv[VEC];
            gate_ld_g<VEC, SPLIT>(G, go + (int64_t)p * C, scale, gv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] += gv[e] * xv[k][e];
          }
        }
      } else {
#pragma unroll 4
        for (int p = pg; p < np; p += PG) {  // (P < 2^30 and PG <= 256: no overflow)
          float gv[VEC], xw[VEC];
          gate_ld_g<VEC, SPLIT>(G, go + (int64_t)p * C, scale, gv);
          ld<VEC>(x + xo + (int64_t)p * C, xw);
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc[e] += gv[e] * xw[e];
        }
      }
      // the PG partial sums of a channel vector: a fixed tree over LDS (thread t holds group t / CL of lane t % CL)
#pragma unroll
      for (int e = 0; e < VEC; ++e) red[e * 256 + threadIdx.x] = acc[e];
      __syncthreads();
      for (int half = PG >> 1; half > 0; half >>= 1) {
        if (pg < half) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) red[e * 256 + threadIdx.x] += red[e * 256 + threadIdx.x + half * CL];
        }
        __syncthreads();
      }
      if (pg == 0 && live) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = red[e * 256 + threadIdx.x];
        st<VEC>(ds + (s * B + b) * C + (int64_t)cvi * VEC, acc);
      }
      __syncthreads();  // (red is written again by the next seed)
    }
  }
}

// at most one atomic per workgroup: the maximum of |dx| over its lanes (non-negative floats order like their bit patterns), by
// a shuffle tree per wave and four words of LDS.  The word only grows, so a workgroup whose maximum does not exceed what the word
// already holds reads and leaves (a stale read costs an atomic, never a wrong result).  One atomic per wave had the up to 8192
// waves of a launch, which finish together, queue up on one address for longer than the kernel streams its data.
__device__ __forceinline__ void gate_block_amax(float m, unsigned* __restrict__ amax) {
  __shared__ unsigned wmax[4];
  unsigned b = wave_max_bits(m);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = b;
  __syncthreads();
  if (threadIdx.x == 0 && amax != nullptr) {
    b = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
    if (b > __hip_atomic_load(amax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(amax, b);
  }
}

// ---- VJP: dx[n][p][c] = g[n][p][c] gate[n % B][c] + r[n][c] ----------------------------------------------------------------------
// `chunks`: chunks of PG * GATE_PP positions of a map; `units` = N * tiles * chunks
template <int VEC, bool SPLIT, bool HAS_R>
__global__ __launch_bounds__(256) void gate_vjp_kernel(GateG G, const float* __restrict__ gate, const float* __restrict__ r,
                                                       int64_t B, int P, int C, int CL, int nvc, int tiles, int chunks,
                                                       int64_t units, float* __restrict__ dx, unsigned* __restrict__ amax) {
  const int PG = 256 / CL;
  const int cl = threadIdx.x & (CL - 1), pg = threadIdx.x / CL;
  const float scale = SPLIT ? ldexpf(1.f, -G.sexp[0]) : 1.f;
  const int64_t map = (int64_t)P * C, per_map = (int64_t)tiles * chunks;
  float vmax = 0.f;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t n = u / per_map;
    const int w = (int)(u - n * per_map);
    const int tile = w / chunks, chunk = w - tile * chunks;
    const int cvi = tile * CL + cl;
    if (cvi >= nvc) continue;
    const int64_t b = n % B;
    float gt[VEC], rv[VEC];
    ld<VEC>(gate + b * C + (int64_t)cvi * VEC, gt);
    if constexpr (HAS_R) ld<VEC>(r + n * C + (int64_t)cvi * VEC, rv);
    const int64_t o = n * map + (int64_t)cvi * VEC;
    const int64_t p0 = (int64_t)chunk * PG * GATE_PP + pg;  // (< P + 2048 < 2^31)
#pragma unroll
    for (int k = 0; k < GATE_PP; ++k) {
      const int64_t p = p0 + (int64_t)k * PG;
      if (p < P) {
        float gv[VEC], d[VEC];
        gate_ld_g<VEC, SPLIT>(G, o + p * C, scale, gv);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          if constexpr (HAS_R) d[e] = gv[e] * gt[e] + rv[e];
          else d[e] = gv[e] * gt[e];
          vmax = fmaxf(vmax, fabsf(d[e]));
        }
        st<VEC>(dx + o + p * C, d);
      }
    }
  }
  gate_block_amax(vmax, amax);  // (every thread gets here: a dead lane leaves its unit, not the kernel)
}

// ---- host: the contract and the path of a shape ----------------------------------------------------------------------------------
struct GatePlan {
  int vec;       // 16-byte fp32 accesses, 8-byte ones of the planes
  int CL;        // lanes across the channel vectors (256 / CL position groups)
  int nvc;       // channel vectors of a position
  int tiles;     // tiles of CL channel vectors
  int chunks;    // VJP: chunks of PG * GATE_PP positions of a map (1 for the reduce)
  int resident;  // reduce: x of a thread's positions stays in registers across the seed loop
  int wide;      // an element offset of g does not fit 31 bits (the kernels index with 64 bits throughout)
  int64_t s_per; // reduce: seeds per grid.y slice (S for the VJP)
  int64_t units, blocks;
};

// the shape part of the contract (shared with lk_gate_variant), with the messages under the caller's name
static int gate_check_shape(const char* fn, bool vjp, int64_t S, int64_t B, int64_t P, int64_t C, bool aligned, GatePlan* p) {
  LK_REQUIRE(S >= 1 && B >= 0 && P >= 1 && P < (1ll << 30) && C >= 1 && C < (1ll << 30),
             "%s: extent out of range (1 <= S, 0 <= B, 1 <= P < 2^30, 1 <= C < 2^30)", fn);
  LK_REQUIRE((unsigned __int128)S * (unsigned __int128)B * (unsigned __int128)P * (unsigned __int128)C < ((unsigned __int128)1 << 40),
             "%s: extent out of range (S * B * P * C < 2^40)", fn);
  p->vec = aligned && C % 4 == 0;
  p->nvc = (int)(p->vec ? C / 4 : C);
  p->CL = pow2_ceil(p->nvc, 64);
  p->tiles = (p->nvc + p->CL - 1) / p->CL;
  p->wide = S * B * P * C >= (1ll << 31);
  const int64_t PG = 256 / p->CL;
  if (vjp) {
    p->chunks = (int)((P + PG * GATE_PP - 1) / (PG * GATE_PP));
    p->resident = 0;
    p->units = S * B * p->tiles * p->chunks;  // (< 2^40: a unit holds at least one element)
    p->blocks = p->units < STREAM_MAX_BLOCKS ? p->units : STREAM_MAX_BLOCKS;
    p->s_per = S;
  } else {
    p->chunks = 1;
    p->resident = P <= PG * GATE_NV;
    p->units = B * p->tiles;
    p->blocks = p->units < STREAM_MAX_BLOCKS ? p->units : STREAM_MAX_BLOCKS;
    p->s_per = seeds_per_slice(S, p->blocks * 4);
  }
  return LK_OK;
}

// the cotangent's two forms: exactly one of the fp32 pointer and the plane triple
static int gate_check_g(const char* fn, const float* g, const void* g_h, const void* g_l, const int* sexp, bool* aligned) {
  const bool planes = g_h != nullptr || g_l != nullptr || sexp != nullptr;
  LK_REQUIRE(g != nullptr || planes, "%s: null pointer (g: an fp32 map, or the planes g_h and g_l with sexp)", fn);
  LK_REQUIRE(!(g != nullptr && planes), "%s: both forms of g given (an fp32 map, or the planes g_h and g_l with sexp)", fn);
  LK_REQUIRE(g != nullptr || (g_h && g_l && sexp), "%s: null pointer (the split form of g needs g_h, g_l and sexp)", fn);
  *aligned = g != nullptr ? ((uintptr_t)g & 15) == 0 : (((uintptr_t)g_h | (uintptr_t)g_l) & 7) == 0;
  return LK_OK;
}

static bool gate_clear_of_g(const void* out, unsigned __int128 out_bytes, const float* g, const void* g_h, const void* g_l,
                            const int* sexp, unsigned __int128 elems) {
  if (g) return disjoint(out, out_bytes, g, elems * 4);
  return disjoint(out, out_bytes, g_h, elems * 2) && disjoint(out, out_bytes, g_l, elems * 2) &&
         disjoint(out, out_bytes, sexp, 4);
}

static int gate_check_reduce(const float* g, const void* g_h, const void* g_l, const int* sexp, const float* x, int64_t S,
                             int64_t B, int64_t P, int64_t C, const float* ds, GatePlan* p) {
  bool aligned;
  int rc = gate_check_g("lk_gate_reduce_nhwc_f32", g, g_h, g_l, sexp, &aligned);
  if (rc != LK_OK) return rc;
  LK_REQUIRE(x && ds, "lk_gate_reduce_nhwc_f32: null pointer (x, ds)");
  aligned = aligned && (((uintptr_t)x | (uintptr_t)ds) & 15) == 0;
  rc = gate_check_shape("lk_gate_reduce_nhwc_f32", false, S, B, P, C, aligned, p);
  if (rc != LK_OK) return rc;
  const unsigned __int128 xe = (unsigned __int128)B * P * C, ob = (unsigned __int128)S * B * C * 4;
  LK_REQUIRE(gate_clear_of_g(ds, ob, g, g_h, g_l, sexp, xe * S) && disjoint(ds, ob, x, xe * 4),
             "lk_gate_reduce_nhwc_f32: ds overlaps an input");
  return LK_OK;
}

static int gate_check_vjp(const float* g, const void* g_h, const void* g_l, const int* sexp, const float* gate, const float* r,
                          int64_t S, int64_t B, int64_t P, int64_t C, const float* dx, const unsigned* amax, GatePlan* p) {
  bool aligned;
  int rc = gate_check_g("lk_gate_vjp_nhwc_f32", g, g_h, g_l, sexp, &aligned);
  if (rc != LK_OK) return rc;
  LK_REQUIRE(gate && dx, "lk_gate_vjp_nhwc_f32: null pointer (gate, dx)");
  aligned = aligned && (((uintptr_t)gate | (uintptr_t)r | (uintptr_t)dx) & 15) == 0;
  rc = gate_check_shape("lk_gate_vjp_nhwc_f32", true, S, B, P, C, aligned, p);
  if (rc != LK_OK) return rc;
  const unsigned __int128 ge = (unsigned __int128)S * B * P * C, ob = ge * 4;
  bool clear = gate_clear_of_g(dx, ob, g, g_h, g_l, sexp, ge) && disjoint(dx, ob, gate, (unsigned __int128)B * C * 4);
  if (r) clear = clear && disjoint(dx, ob, r, (unsigned __int128)S * B * C * 4);
  if (amax) clear = clear && disjoint(dx, ob, amax, 4);
  LK_REQUIRE(clear, "lk_gate_vjp_nhwc_f32: dx overlaps an input or the amax word");
  return LK_OK;
}

static GateG gate_operand(const float* g, const void* g_h, const void* g_l, const int* sexp) {
  GateG G;
  G.f32 = g, G.h = static_cast<const _Float16*>(g_h), G.l = static_cast<const _Float16*>(g_l), G.sexp = sexp;
  return G;
}

}  // namespace lk

using namespace lk;

extern "C" int lk_gate_reduce_nhwc_f32(const float* g, const void* g_h, const void* g_l, const int* sexp, const float* x, int64_t S,
                                       int64_t B, int64_t P, int64_t C, float* ds, void* stream) {
  GatePlan p;
  const int rc = gate_check_reduce(g, g_h, g_l, sexp, x, S, B, P, C, ds, &p);
  if (rc != LK_OK) return rc;
  if (B == 0) return LK_OK;
  const GateG G = gate_operand(g, g_h, g_l, sexp);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)p.blocks, (unsigned)((S + p.s_per - 1) / p.s_per));
#define LK_GATE_R(V, SP, RES)                                                                                                \
  hipLaunchKernelGGL((gate_reduce_kernel<V, SP, RES>), grid, dim3(256), 0, st, G, x, S, B, (int)P, (int)C, p.CL, p.nvc, p.tiles, \
                     p.s_per, p.units, ds)
#define LK_GATE_R2(V, SP)             \
  do {                                \
    if (p.resident) LK_GATE_R(V, SP, true); \
    else LK_GATE_R(V, SP, false);     \
  } while (0)
  if (p.vec) {
    if (g) LK_GATE_R2(4, false);
    else LK_GATE_R2(4, true);
  } else {
    if (g) LK_GATE_R2(1, false);
    else LK_GATE_R2(1, true);
  }
#undef LK_GATE_R2
#undef LK_GATE_R
  return check_launch("gate_reduce_kernel");
}

extern "C" int lk_gate_vjp_nhwc_f32(const float* g, const void* g_h, const void* g_l, const int* sexp, const float* gate,
                                    const float* r, int64_t S, int64_t B, int64_t P, int64_t C, float* dx, unsigned* amax,
                                    void* stream) {
  GatePlan p;
  const int rc = gate_check_vjp(g, g_h, g_l, sexp, gate, r, S, B, P, C, dx, amax, &p);
  if (rc != LK_OK) return rc;
  if (B == 0) return LK_OK;
  const GateG G = gate_operand(g, g_h, g_l, sexp);
  hipStream_t st = (hipStream_t)stream;
#define LK_GATE_V(V, SP, HR)                                                                                                  \
  hipLaunchKernelGGL((gate_vjp_kernel<V, SP, HR>), dim3((unsigned)p.blocks), dim3(256), 0, st, G, gate, r, B, (int)P, (int)C, p.CL, \
                     p.nvc, p.tiles, p.chunks, p.units, dx, amax)
#define LK_GATE_V2(V, SP)          \
  do {                             \
    if (r) LK_GATE_V(V, SP, true); \
    else LK_GATE_V(V, SP, false);  \
  } while (0)
  if (p.vec) {
    if (g) LK_GATE_V2(4, false);
    else LK_GATE_V2(4, true);
  } else {
    if (g) LK_GATE_V2(1, false);
    else LK_GATE_V2(1, true);
  }
#undef LK_GATE_V2
#undef LK_GATE_V
  return check_launch("gate_vjp_kernel");
}

// vec | resident << 1 | seed-split << 2 | wide << 3 | log2(lanes across the channel vectors) << 4 | workgroups of grid.x << 8
extern "C" int lk_gate_variant(int vjp, int64_t S, int64_t B, int64_t P, int64_t C, int aligned) {
  GatePlan p;
  if (vjp != 0 && vjp != 1) return -1;
  if (gate_check_shape("lk_gate_variant", vjp != 0, S, B, P, C, aligned != 0, &p) != LK_OK) return -1;
  int lg = 0;
  while ((1 << lg) < p.CL) ++lg;
  return p.vec | p.resident << 1 | (p.s_per < S ? 1 : 0) << 2 | p.wide << 3 | lg << 4 | (int)p.blocks << 8;
}
