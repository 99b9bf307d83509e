// Channel concatenation (torch.cat along dim 1 of [B, C, H, W] maps: DenseNet blocks, Inception branches, U-shaped skips) on
// NHWC feature maps for the seed-batched reverse sweep.  Rows are the R = N H W pixels of a map; a SLICE is channels
// [c0, c0 + Cs) of a map with Ct channels.
//   forward  dst[r Ct + c0 + c] = src[r Cs + c]                      one launch per source, into one [R][Ct] allocation
//   VJP      dst[r Cs + c]      = sum_p value_p[r Ct + c0 + c]       the slice of the SUM of up to LK_CAT_MAX_PARTS cotangent
//            parts, each an fp32 map or the two fp16 planes of a ONE-scale split tensor, value = (float(h) + float(l)) * 2^-sexp[0]
//            exactly as SplitTensor.float() forms it; the sum runs in fp32, left to right in the listed order
// Replaces, on the NHWC sweep, the reverse pass of laplace/curvature/curvlinops.py:87-100 and curvature.py:88-129 through a
// concatenation as stock torch runs it: a .float() per split part, a sum over the whole [R][Ct] map, a strided
// narrow().contiguous() per source and a pass for max|.|.
//
// Both kernels are streaming copies: lanes along the channels of the slice, 16 bytes per lane (16-byte loads and stores of fp32,
// 8-byte loads of four halves) where Ct, c0 and Cs are multiples of 4 and the pointers are aligned, one element per lane
// otherwise; a grid of at most 256 CUs x 8 workgroups strides over the lanes.  Only the slice of every part is read.  Every dst
// element has one owner, stores are plain, repeated runs give the same bits.  `amax` receives max|dst| as the bit pattern of a
// non-negative float through atomicMax, one atomic per wave (wave_amax of lk_stream.h).
// Minimal traffic of the VJP: R Cs (4 + 4 n_f32 + 4 n_split) bytes; of the forward: 8 R Cs bytes.
#include "lk_stream.h"

namespace lk {

struct CatParts {  // by value: device pointers of the parts (f32[p] non-null: an fp32 map; else planes h[p], l[p] and sexp[p])
  const float* f32[LK_CAT_MAX_PARTS];
  const _Float16* h[LK_CAT_MAX_PARTS];
  const _Float16* l[LK_CAT_MAX_PARTS];
  const int* sexp[LK_CAT_MAX_PARTS];
};

// ---- forward: a lane per VEC channels of a source row ---------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(256) void cat_fwd_kernel(const float* __restrict__ src, ColSliceGeom q, float* __restrict__ dst) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < q.lanes; t += (int64_t)gridDim.x * 256) {
    int64_t r;
    int c;
    col_where<VEC>(q, t, r, c);
    float v[VEC];
    ld<VEC>(src + t * VEC, v);  // (the source is the contiguous [R][Cs] map: its lanes lie in order)
    st<VEC>(dst + r * q.Ct + q.c0 + c, v);
  }
}

// ---- VJP: a lane per VEC channels of a dst row; NP parts, summed left to right --------------------------------------------------
template <int VEC, int NP>
__global__ __launch_bounds__(256) void cat_vjp_kernel(CatParts P, ColSliceGeom q, float* __restrict__ dst,
                                                      unsigned* __restrict__ amax) {
  float scale[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) scale[p] = P.f32[p] != nullptr ? 1.f : ldexpf(1.f, -P.sexp[p][0]);
  float vmax = 0.f;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < q.lanes; t += (int64_t)gridDim.x * 256) {
    int64_t r;
    int c;
    col_where<VEC>(q, t, r, c);
    const int64_t at = r * q.Ct + q.c0 + c;
    float v[NP][VEC];
#pragma unroll
    for (int p = 0; p < NP; ++p) {  // (which kind a part is is the same in every lane; all loads are issued before the sum)
      if (P.f32[p] != nullptr) ld<VEC>(P.f32[p] + at, v[p]);
      else ld_split<VEC>(P.h[p] + at, P.l[p] + at, scale[p], v[p]);
    }
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      acc[e] = v[0][e];
#pragma unroll
      for (int p = 1; p < NP; ++p) acc[e] = acc[e] + v[p][e];
      vmax = fmaxf(vmax, fabsf(acc[e]));
    }
    st<VEC>(dst + t * VEC, acc);
  }
  wave_amax(vmax, amax);
}

// ---- host: the contract and the path of a shape ----------------------------------------------------------------------------------
struct CatPlan {
  int vec;
  int64_t lanes, blocks;
};

// the part of the contract both entry points share, with the messages under the caller's name
static int cat_check_shape(const char* fn, int64_t R, int64_t Ct, int64_t c0, int64_t Cs, bool aligned, CatPlan* p) {
  LK_REQUIRE(Cs >= 1 && c0 >= 0 && Ct < (1ll << 30) && c0 <= Ct && Cs <= Ct - c0,
             "%s: slice out of range (1 <= Cs, 0 <= c0, c0 + Cs <= Ct < 2^30)", fn);
  LK_REQUIRE(R >= 0 && (unsigned __int128)R * (unsigned __int128)Ct < ((unsigned __int128)1 << 40),
             "%s: extent out of range (0 <= R, R * Ct < 2^40)", fn);
  p->vec = aligned && Ct % 4 == 0 && c0 % 4 == 0 && Cs % 4 == 0;
  p->lanes = R * (p->vec ? Cs / 4 : Cs);
  p->blocks = grid_blocks(p->lanes);
  return LK_OK;
}

static ColSliceGeom cat_geometry(const CatPlan& p, int64_t Ct, int64_t c0, int64_t Cs) {
  ColSliceGeom q;
  q.Ct = Ct, q.c0 = c0, q.Cs = Cs, q.lanes = p.lanes;
  q.CV = (int)(p.vec ? Cs / 4 : Cs);
  q.big = p.lanes >= (1ll << 31);
  q.cv_div = make_fastdiv(q.CV);
  return q;
}

static int cat_check_fwd(const float* src, int64_t R, int64_t Cs, const float* dst, int64_t Ct, int64_t c0, CatPlan* p) {
  LK_REQUIRE(src && dst, "lk_cat_fwd_nhwc_f32: null pointer");
  const bool aligned = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
  const int rc = cat_check_shape("lk_cat_fwd_nhwc_f32", R, Ct, c0, Cs, aligned, p);
  if (rc != LK_OK) return rc;
  LK_REQUIRE(disjoint(src, (unsigned __int128)R * Cs * 4, dst, (unsigned __int128)R * Ct * 4),
             "lk_cat_fwd_nhwc_f32: dst overlaps src");
  return LK_OK;
}

static int cat_check_vjp(int nparts, const float* const* f32, const void* const* hi, const void* const* lo,
                         const int* const* sexp, int64_t R, int64_t Ct, int64_t c0, int64_t Cs, const float* dst,
                         CatPlan* p, int* split_mask) {
  LK_REQUIRE(nparts >= 1 && nparts <= LK_CAT_MAX_PARTS,
             "lk_cat_vjp_nhwc_f32: nparts out of range (1 <= nparts <= LK_CAT_MAX_PARTS = 4)");
  LK_REQUIRE(f32 && hi && lo && sexp && dst, "lk_cat_vjp_nhwc_f32: null pointer");
  uintptr_t bits16 = (uintptr_t)dst, bits8 = 0;
  *split_mask = 0;
  for (int i = 0; i < nparts; ++i) {
    LK_REQUIRE(f32[i] || (hi[i] && lo[i] && sexp[i]),
               "lk_cat_vjp_nhwc_f32: a part is an fp32 map (f32) or, where f32 is null, the planes hi and lo with sexp");
    if (f32[i]) {
      bits16 |= (uintptr_t)f32[i];
    } else {
      bits8 |= (uintptr_t)hi[i] | (uintptr_t)lo[i];
      *split_mask |= 1 << i;
    }
  }
  const bool aligned = (bits16 & 15) == 0 && (bits8 & 7) == 0;
  const int rc = cat_check_shape("lk_cat_vjp_nhwc_f32", R, Ct, c0, Cs, aligned, p);
  if (rc != LK_OK) return rc;
  const unsigned __int128 db = (unsigned __int128)R * Cs * 4, pe = (unsigned __int128)R * Ct;
  bool clear = true;
  for (int i = 0; i < nparts; ++i) {
    if (f32[i]) clear = clear && disjoint(dst, db, f32[i], pe * 4);
    else clear = clear && disjoint(dst, db, hi[i], pe * 2) && disjoint(dst, db, lo[i], pe * 2);
  }
  LK_REQUIRE(clear, "lk_cat_vjp_nhwc_f32: dst overlaps a part");
  return LK_OK;
}

}  // namespace lk

using namespace lk;

extern "C" int lk_cat_fwd_nhwc_f32(const float* src, int64_t R, int64_t Cs, float* dst, int64_t Ct, int64_t c0, void* stream) {
  CatPlan p;
  const int rc = cat_check_fwd(src, R, Cs, dst, Ct, c0, &p);
  if (rc != LK_OK) return rc;
  if (R == 0) return LK_OK;
  const ColSliceGeom q = cat_geometry(p, Ct, c0, Cs);
  hipStream_t st = (hipStream_t)stream;
  if (p.vec) hipLaunchKernelGGL((cat_fwd_kernel<4>), dim3((unsigned)p.blocks), dim3(256), 0, st, src, q, dst);
  else hipLaunchKernelGGL((cat_fwd_kernel<1>), dim3((unsigned)p.blocks), dim3(256), 0, st, src, q, dst);
  return check_launch("cat_fwd_kernel");
}

extern "C" int lk_cat_vjp_nhwc_f32(int nparts, const float* const* f32, const void* const* hi, const void* const* lo,
                                   const int* const* sexp, int64_t R, int64_t Ct, int64_t c0, int64_t Cs, float* dst,
                                   unsigned* amax, void* stream) {
  CatPlan p;
  int split_mask;
  const int rc = cat_check_vjp(nparts, f32, hi, lo, sexp, R, Ct, c0, Cs, dst, &p, &split_mask);
  if (rc != LK_OK) return rc;
  if (R == 0) return LK_OK;
  const ColSliceGeom q = cat_geometry(p, Ct, c0, Cs);
  CatParts P;
  for (int i = 0; i < LK_CAT_MAX_PARTS; ++i) {
    const bool split = i < nparts && f32[i] == nullptr;
    P.f32[i] = i < nparts ? f32[i] : nullptr;
    P.h[i] = split ? static_cast<const _Float16*>(hi[i]) : nullptr;
    P.l[i] = split ? static_cast<const _Float16*>(lo[i]) : nullptr;
    P.sexp[i] = split ? sexp[i] : nullptr;
  }
  hipStream_t st = (hipStream_t)stream;
#define LK_CAT_VJP(V, N) \
  hipLaunchKernelGGL((cat_vjp_kernel<V, N>), dim3((unsigned)p.blocks), dim3(256), 0, st, P, q, dst, amax)
#define LK_CAT_VJP_N(N)          \
  do {                           \
    if (p.vec) LK_CAT_VJP(4, N); \
    else LK_CAT_VJP(1, N);       \
  } while (0)
  switch (nparts) {
    case 1: LK_CAT_VJP_N(1); break;
    case 2: LK_CAT_VJP_N(2); break;
    case 3: LK_CAT_VJP_N(3); break;
    default: LK_CAT_VJP_N(4); break;
  }
#undef LK_CAT_VJP_N
#undef LK_CAT_VJP
  return check_launch("cat_vjp_kernel");
}

// vec | nparts << 1 | split_mask << 4 | 64-bit lane index << 8 | workgroups of the grid << 12
extern "C" int lk_cat_variant(int nparts, int split_mask, int64_t R, int64_t Ct, int64_t c0, int64_t Cs, int aligned) {
  CatPlan p;
  if (nparts < 1 || nparts > LK_CAT_MAX_PARTS || split_mask < 0 || split_mask >= (1 << nparts)) return -1;
  if (cat_check_shape("lk_cat_variant", R, Ct, c0, Cs, aligned != 0, &p) != LK_OK) return -1;
  return p.vec | nparts << 1 | split_mask << 4 | (p.lanes >= (1ll << 31) ? 1 : 0) << 8 | (int)p.blocks << 12;
}
