// Static slicing (Tensor.chunk / split / narrow / x[:, a:b] / x[:, 0]: CSP stages, packed qkv projections, class tokens) for
// the seed-batched reverse sweeps - the transpose of csrc/lk_cat.hip.  A slice along dim d of a contiguous [N, ...] tensor is a
// column range of the row matrix [R = N prod(dims before d)][Ct = prod(dims from d)]; a PIECE is columns [c0, c0 + cs) of it.
//   forward  dst[r Cs + c] = src[r Ct + c0 + c]                       one launch, into a contiguous [R][Cs]
//   VJP      dst[r Ct + c] = sum over the pieces p with c0[p] <= c < c0[p] + cs[p] of value_p[r cs[p] + c - c0[p]], +0.0f where
//            no piece covers c.  Piece p is a contiguous [R][cs[p]] fp32 map or the two fp16 planes of a ONE-scale split tensor,
//            value = (float(h) + float(l)) * 2^-sexp[0] exactly as SplitTensor.float() forms it.  The sum starts from the value
//            of the first covering piece and adds the later ones in fp32 in the listed order.
// Replaces, in the reverse pass of laplace/curvature/curvlinops.py:87-100 and curvature.py:88-129 through a slice as stock torch
// runs it: a zero fill of the whole [R][Ct] tensor and a strided read-modify-write per slice, then a sum of the full-width
// tensors and a pass for max|.|.
//
// Both kernels are streaming copies in the style of lk_cat.hip: lanes along the columns of dst, 16 bytes per lane (16-byte loads
// and stores of fp32, 8-byte loads of four halves) where Ct and every c0 and cs are multiples of 4 and the pointers are aligned -
// a vector then never straddles a piece boundary -, one element per lane otherwise; a grid of at most 256 CUs x 8 workgroups
// strides over the lanes.  Every dst element has one owner, stores are plain, repeated runs give the same bits.  `amax` receives
// max|dst| as the bit pattern of a non-negative float through atomicMax, one atomic per wave (wave_amax of lk_stream.h).
// Minimal traffic of the VJP: 4 R Ct bytes written plus every piece read once; of the forward: 8 R Cs bytes.
#include "lk_stream.h"

namespace lk {

struct SlicePieces {  // by value: device pointers and column ranges of the pieces (f32[p] non-null: an fp32 map; else planes)
  const float* f32[LK_SLICE_MAX_PIECES];
  const _Float16* h[LK_SLICE_MAX_PIECES];
  const _Float16* l[LK_SLICE_MAX_PIECES];
  const int* sexp[LK_SLICE_MAX_PIECES];
  int c0[LK_SLICE_MAX_PIECES];
  int cs[LK_SLICE_MAX_PIECES];
};

// ---- forward: a lane per VEC columns of a dst row ---------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(256) void slice_fwd_kernel(const float* __restrict__ src, ColSliceGeom q, float* __restrict__ dst) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < q.lanes; t += (int64_t)gridDim.x * 256) {
    int64_t r;
    int c;
    col_where<VEC>(q, t, r, c);
    float v[VEC];
    ld<VEC>(src + r * q.Ct + q.c0 + c, v);
    st<VEC>(dst + t * VEC, v);  // (dst is the contiguous [R][Cs] map: its lanes lie in order)
  }
}

// ---- VJP: a lane per VEC columns of a dst row [R][Ct]; NP pieces, the covering ones summed in the listed order --------------------
template <int VEC, int NP>
__global__ __launch_bounds__(256) void slice_vjp_kernel(SlicePieces P, ColSliceGeom q, float* __restrict__ dst,
                                                        unsigned* __restrict__ amax) {
  float scale[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) scale[p] = P.f32[p] != nullptr ? 1.f : ldexpf(1.f, -P.sexp[p][0]);
  float vmax = 0.f;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < q.lanes; t += (int64_t)gridDim.x * 256) {
    int64_t r;
    int c;
    col_where<VEC>(q, t, r, c);
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    bool have = false;
#pragma unroll
    for (int p = 0; p < NP; ++p) {  // (with VEC == 4 every boundary is a multiple of 4: a lane lies inside a piece or outside it)
      const int cp = c - P.c0[p];
      if (cp >= 0 && cp < P.cs[p]) {
        const int64_t at = r * P.cs[p] + cp;
        float v[VEC];
        if (P.f32[p] != nullptr) ld<VEC>(P.f32[p] + at, v);
        else ld_split<VEC>(P.h[p] + at, P.l[p] + at, scale[p], v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = have ? acc[e] + v[e] : v[e];
        have = true;
      }
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) vmax = fmaxf(vmax, fabsf(acc[e]));
    st<VEC>(dst + t * VEC, acc);  // (dst is the contiguous [R][Ct] map: its lanes lie in order)
  }
  wave_amax(vmax, amax);
}

// ---- host: the contract and the path of a shape ----------------------------------------------------------------------------------
struct SlicePlan {
  int vec;
  int64_t lanes, blocks;
};

// the extent both entry points share, with the messages under the caller's name
static int slice_check_extent(const char* fn, int64_t R, int64_t Ct) {
  LK_REQUIRE(Ct >= 1 && Ct < (1ll << 30), "%s: row length out of range (1 <= Ct < 2^30)", fn);
  LK_REQUIRE(R >= 0 && (unsigned __int128)R * (unsigned __int128)Ct < ((unsigned __int128)1 << 40),
             "%s: extent out of range (0 <= R, R * Ct < 2^40)", fn);
  return LK_OK;
}

static int slice_check_range(const char* fn, int64_t Ct, int64_t c0, int64_t cs) {
  LK_REQUIRE(cs >= 1 && c0 >= 0 && c0 <= Ct && cs <= Ct - c0, "%s: slice out of range (1 <= cs, 0 <= c0, c0 + cs <= Ct < 2^30)", fn);
  return LK_OK;
}

static void slice_plan(SlicePlan* p, int64_t R, int64_t width, bool vec) {
  p->vec = vec;
  p->lanes = R * (vec ? width / 4 : width);
  p->blocks = grid_blocks(p->lanes);
}

static ColSliceGeom slice_geometry(const SlicePlan& p, int64_t Ct, int64_t c0, int64_t Cs, int64_t width) {
  ColSliceGeom q;
  q.Ct = Ct, q.c0 = c0, q.Cs = Cs, q.lanes = p.lanes;
  q.CV = (int)(p.vec ? width / 4 : width);
  q.big = p.lanes >= (1ll << 31);
  q.cv_div = make_fastdiv(q.CV);
  return q;
}

// the shape part of the VJP's contract (shared with lk_slice_variant)
static int slice_check_vjp_shape(const char* fn, int npieces, const int64_t* c0, const int64_t* cs, int64_t R, int64_t Ct,
                                 bool aligned, SlicePlan* p) {
  int rc = slice_check_extent(fn, R, Ct);
  if (rc != LK_OK) return rc;
  bool vec = aligned && Ct % 4 == 0;
  for (int i = 0; i < npieces; ++i) {
    rc = slice_check_range(fn, Ct, c0[i], cs[i]);
    if (rc != LK_OK) return rc;
    vec = vec && c0[i] % 4 == 0 && cs[i] % 4 == 0;
  }
  slice_plan(p, R, Ct, vec);
  return LK_OK;
}

static int slice_check_fwd(const float* src, int64_t R, int64_t Ct, int64_t c0, int64_t Cs, const float* dst, SlicePlan* p) {
  LK_REQUIRE(src && dst, "lk_slice_fwd_f32: null pointer");
  int rc = slice_check_extent("lk_slice_fwd_f32", R, Ct);
  if (rc != LK_OK) return rc;
  rc = slice_check_range("lk_slice_fwd_f32", Ct, c0, Cs);
  if (rc != LK_OK) return rc;
  LK_REQUIRE(disjoint(dst, (unsigned __int128)R * Cs * 4, src, (unsigned __int128)R * Ct * 4),
             "lk_slice_fwd_f32: dst overlaps src");
  const bool aligned = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
  slice_plan(p, R, Cs, aligned && Ct % 4 == 0 && c0 % 4 == 0 && Cs % 4 == 0);
  return LK_OK;
}

static int slice_check_vjp(int npieces, const float* const* f32, const void* const* hi, const void* const* lo,
                           const int* const* sexp, const int64_t* c0, const int64_t* cs, int64_t R, int64_t Ct, const float* dst,
                           SlicePlan* p) {
  LK_REQUIRE(npieces >= 1 && npieces <= LK_SLICE_MAX_PIECES,
             "lk_slice_vjp_f32: npieces out of range (1 <= npieces <= LK_SLICE_MAX_PIECES = 8)");
  LK_REQUIRE(f32 && hi && lo && sexp && c0 && cs && dst, "lk_slice_vjp_f32: null pointer");
  uintptr_t bits16 = (uintptr_t)dst, bits8 = 0;
  for (int i = 0; i < npieces; ++i) {
    LK_REQUIRE(f32[i] || (hi[i] && lo[i] && sexp[i]),
               "lk_slice_vjp_f32: a piece is an fp32 map (f32) or, where f32 is null, the planes hi and lo with sexp");
    if (f32[i]) bits16 |= (uintptr_t)f32[i];
    else bits8 |= (uintptr_t)hi[i] | (uintptr_t)lo[i];
  }
  const int rc = slice_check_vjp_shape("lk_slice_vjp_f32", npieces, c0, cs, R, Ct, (bits16 & 15) == 0 && (bits8 & 7) == 0, p);
  if (rc != LK_OK) return rc;
  const unsigned __int128 db = (unsigned __int128)R * Ct * 4;
  bool clear = true;
  for (int i = 0; i < npieces; ++i) {
    const unsigned __int128 pe = (unsigned __int128)R * cs[i];
    if (f32[i]) clear = clear && disjoint(dst, db, f32[i], pe * 4);
    else clear = clear && disjoint(dst, db, hi[i], pe * 2) && disjoint(dst, db, lo[i], pe * 2);
  }
  LK_REQUIRE(clear, "lk_slice_vjp_f32: dst overlaps a piece");
  return LK_OK;
}

}  // namespace lk

using namespace lk;

extern "C" int lk_slice_fwd_f32(const float* src, int64_t R, int64_t Ct, int64_t c0, int64_t Cs, float* dst, void* stream) {
  SlicePlan p;
  const int rc = slice_check_fwd(src, R, Ct, c0, Cs, dst, &p);
  if (rc != LK_OK) return rc;
  if (R == 0) return LK_OK;
  const ColSliceGeom q = slice_geometry(p, Ct, c0, Cs, Cs);
  hipStream_t st = (hipStream_t)stream;
  if (p.vec) hipLaunchKernelGGL((slice_fwd_kernel<4>), dim3((unsigned)p.blocks), dim3(256), 0, st, src, q, dst);
  else hipLaunchKernelGGL((slice_fwd_kernel<1>), dim3((unsigned)p.blocks), dim3(256), 0, st, src, q, dst);
  return check_launch("slice_fwd_kernel");
}

extern "C" int lk_slice_vjp_f32(int npieces, const float* const* f32, const void* const* hi, const void* const* lo,
                                const int* const* sexp, const int64_t* c0, const int64_t* cs, int64_t R, int64_t Ct, float* dst,
                                unsigned* amax, void* stream) {
  SlicePlan p;
  const int rc = slice_check_vjp(npieces, f32, hi, lo, sexp, c0, cs, R, Ct, dst, &p);
  if (rc != LK_OK) return rc;
  if (R == 0) return LK_OK;
  const ColSliceGeom q = slice_geometry(p, Ct, 0, Ct, Ct);
  SlicePieces P;
  for (int i = 0; i < LK_SLICE_MAX_PIECES; ++i) {
    const bool used = i < npieces, split = used && f32[i] == nullptr;
    P.f32[i] = used ? f32[i] : nullptr;
    P.h[i] = split ? static_cast<const _Float16*>(hi[i]) : nullptr;
    P.l[i] = split ? static_cast<const _Float16*>(lo[i]) : nullptr;
    P.sexp[i] = split ? sexp[i] : nullptr;
    P.c0[i] = used ? (int)c0[i] : 0;
    P.cs[i] = used ? (int)cs[i] : 0;
  }
  hipStream_t st = (hipStream_t)stream;
#define LK_SLICE_VJP(V, N) \
  hipLaunchKernelGGL((slice_vjp_kernel<V, N>), dim3((unsigned)p.blocks), dim3(256), 0, st, P, q, dst, amax)
#define LK_SLICE_VJP_N(N)          \
  do {                             \
    if (p.vec) LK_SLICE_VJP(4, N); \
    else LK_SLICE_VJP(1, N);       \
  } while (0)
  switch (npieces) {
    case 1: LK_SLICE_VJP_N(1); break;
    case 2: LK_SLICE_VJP_N(2); break;
    case 3: LK_SLICE_VJP_N(3); break;
    case 4: LK_SLICE_VJP_N(4); break;
    case 5: LK_SLICE_VJP_N(5); break;
    case 6: LK_SLICE_VJP_N(6); break;
    case 7: LK_SLICE_VJP_N(7); break;
    default: LK_SLICE_VJP_N(8); break;
  }
#undef LK_SLICE_VJP_N
#undef LK_SLICE_VJP
  return check_launch("slice_vjp_kernel");
}

// vec | npieces << 1 | split_mask << 5 | 64-bit lane index << 13 | workgroups of the grid << 14
extern "C" int lk_slice_variant(int npieces, int split_mask, const int64_t* c0, const int64_t* cs, int64_t R, int64_t Ct,
                                int aligned) {
  SlicePlan p;
  if (npieces < 1 || npieces > LK_SLICE_MAX_PIECES || split_mask < 0 || split_mask >= (1 << npieces) || !c0 || !cs) return -1;
  if (slice_check_vjp_shape("lk_slice_variant", npieces, c0, cs, R, Ct, aligned != 0, &p) != LK_OK) return -1;
  return p.vec | npieces << 1 | split_mask << 5 | (p.lanes >= (1ll << 31) ? 1 : 0) << 13 | (int)p.blocks << 14;
}
