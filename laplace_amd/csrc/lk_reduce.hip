// Maximum over positions (x.amax(2), x.max(2)[0], AdaptiveMaxPool1d(1): what text CNNs, PointNets and 1-D ResNets end in) for the
// seed-batched reverse sweep.  The operand is a contiguous fp32 [outer][L][inner], L the product of the reduced dims.
//   forward  y[o][i] = max_l x[o][l][i];  idx[o][i] = the first l that holds it;  cnt[o][i] = how many l compare equal to it
//            (torch's comparison: 0.0 == -0.0).  A row with a NaN gives NaN in y; its idx and cnt are unspecified.
//   VJP      g [S][outer][inner] -> dx [S][outer][L][inner] for all seeds in one launch
//            first (max(dim), the adaptive max pools):  dx = (l == idx) ? g : +0.0
//            even  (amax: x, y, cnt given):             dx = (x == y) ? g / cnt : +0.0
// Replaces, in the reverse pass of laplace/curvature/curvlinops.py:87-100 and curvature.py:88-129 through such a reduction as
// stock torch runs it, a zero fill of the whole [S][outer][L][inner] tensor and a scatter per seed.
//
// Forward, inner == 1: a group of W lanes (a power of two <= 64, sized from L) owns a row, strides over it and reduces
// (value, index, count) items with a fixed xor-shuffle tree; the items are ordered "larger value, then smaller index" and equal
// values add their counts, which is commutative and associative, so the result does not depend on the tree.  inner > 1: a lane
// per (outer, inner vector) walks l with stride inner, coalesced across lanes; 16-byte accesses where inner % 4 == 0 and the
// pointers are aligned.  A reduction is never split over workgroups.
// VJP: a lane per VEC adjacent elements of a [outer][L][inner] map (along L where inner == 1, along inner otherwise); idx or
// x, y and cnt of the lane's elements are read once and reused across the seed loop.  Every dx element has one owner and is
// written (the caller fills nothing), stores are plain, repeated runs give the same bits.  Few lanes: the seeds are split over
// grid.y.  Minimal traffic of the VJP: 4 S (outer inner)(L + 1) bytes.
#include "lk_stream.h"

namespace lk {

typedef int i32x4 __attribute__((ext_vector_type(4)));

template <int VEC>
__device__ __forceinline__ void ldi(const int* __restrict__ p, int (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const i32x4 t = *reinterpret_cast<const i32x4*>(p);
    v[0] = t[0], v[1] = t[1], v[2] = t[2], v[3] = t[3];
  } else {
    v[0] = *p;
  }
}
template <int VEC>
__device__ __forceinline__ void sti(int* __restrict__ p, const int (&v)[VEC]) {
  if constexpr (VEC == 4) {
    i32x4 t;
    t[0] = v[0]; t[1] = v[1]; t[2] = v[2]; t[3] = v[3];
    *reinterpret_cast<i32x4*>(p) = t;
  } else {
    *p = v[0];
  }
}

// the running maximum of some positions: value, first position, number of positions that compare equal
struct MaxItem {
  float v;
  int i, c;
};
// larger value, then smaller index; equal values (0.0 == -0.0) add their counts and keep the value at the smaller index; a NaN
// wins over every number.  Commutative and associative on NaN-free items.
__device__ __forceinline__ MaxItem max_merge(const MaxItem& a, const MaxItem& b) {
  if (a.v != a.v) return a;
  if (b.v != b.v) return b;
  if (a.v == b.v) {
    MaxItem r;
    r.v = a.i < b.i ? a.v : b.v;
    r.i = min(a.i, b.i);
    r.c = a.c + b.c;
    return r;
  }
  return a.v > b.v ? a : b;
}
// the next position l (larger than every one merged so far) joins the item
__device__ __forceinline__ void max_step(MaxItem& m, float x, int l) {
  if (m.v != m.v) return;
  if (x == m.v) {
    m.c += 1;
    if (m.i > l) m.i = l;  // (only the empty item: its index is INT_MAX)
  } else if (x > m.v || x != x) {
    m.v = x, m.i = l, m.c = 1;
  }
}
__device__ __forceinline__ MaxItem max_empty() {
  MaxItem m;
  m.v = -__builtin_huge_valf(), m.i = 0x7fffffff, m.c = 0;
  return m;
}

// ---- forward, inner == 1: W lanes per row, row groups handed out by a grid stride --------------------------------------------------
__global__ __launch_bounds__(256) void maxred_fwd_row_kernel(const float* __restrict__ x, int64_t R, int L, int W,
                                                             int64_t groups, float* __restrict__ y, int* __restrict__ idx,
                                                             int* __restrict__ cnt) {
  const int per = 256 / W, lane = threadIdx.x & (W - 1);
  for (int64_t gidx = blockIdx.x; gidx < groups; gidx += gridDim.x) {  // (uniform over the workgroup: the shuffles are safe)
    const int64_t row = gidx * per + threadIdx.x / W;
    const bool live = row < R;  // (dead groups stay in the shuffles and touch no memory)
    const float* xr = x + (live ? row * L : 0);
    MaxItem m = max_empty();
    const int n = live ? L : 0;
#pragma unroll 4
    for (int l = lane; l < n; l += W) max_step(m, xr[l], l);  // (L < 2^30: l + W stays below 2^31)
    for (int off = W >> 1; off > 0; off >>= 1) {
      MaxItem o;
      o.v = __shfl_xor(m.v, off, 64), o.i = __shfl_xor(m.i, off, 64), o.c = __shfl_xor(m.c, off, 64);
      m = max_merge(m, o);
    }
    if (live && lane == 0) y[row] = m.v, idx[row] = m.i, cnt[row] = m.c;
  }
}

// ---- forward, inner > 1: a lane per VEC adjacent columns of an [outer][inner] result -------------------------------------------
struct MaxredGeom {
  int64_t lanes;
  int L, inner;
  int IV;   // lanes along inner (forward, VJP of inner > 1) or along L (VJP of inner == 1)
  int big;  // the lane index does not fit 31 bits: 64-bit division
  FastDiv iv_div, l_div;
};

template <int VEC>
__global__ __launch_bounds__(256) void maxred_fwd_col_kernel(const float* __restrict__ x, MaxredGeom q, float* __restrict__ y,
                                                             int* __restrict__ idx, int* __restrict__ cnt) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < q.lanes; t += (int64_t)gridDim.x * 256) {
    int64_t o;
    int iv;
    if (!q.big) {
      const int oi = fdiv((int)t, q.iv_div);
      o = oi, iv = (int)t - oi * q.IV;
    } else {
      o = t / q.IV, iv = (int)(t - o * q.IV);
    }
    const float* xp = x + o * q.L * q.inner + (int64_t)iv * VEC;
    MaxItem m[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) m[e] = max_empty();
#pragma unroll 4
    for (int l = 0; l < q.L; ++l) {
      float v[VEC];
      ld<VEC>(xp + (int64_t)l * q.inner, v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) max_step(m[e], v[e], l);
    }
    float yv[VEC];
    int iw[VEC], cw[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) yv[e] = m[e].v, iw[e] = m[e].i, cw[e] = m[e].c;
    st<VEC>(y + t * VEC, yv);  // (the results are contiguous [outer][inner] maps: their lanes lie in order)
    sti<VEC>(idx + t * VEC, iw);
    sti<VEC>(cnt + t * VEC, cw);
  }
}

// ---- VJP: a lane per VEC adjacent elements of [outer][L][inner]; ROW: inner == 1 (the vector runs along L) ------------------------
template <int VEC, bool ROW, bool EVEN>
__global__ __launch_bounds__(256) void maxred_vjp_kernel(const float* __restrict__ g, const int* __restrict__ idx,
                                                         const float* __restrict__ x, const float* __restrict__ y,
                                                         const int* __restrict__ cnt, int S, int s_per, MaxredGeom q,
                                                         int64_t g_stride, int64_t dx_stride, float* __restrict__ dx) {
  const int s_begin = blockIdx.y * s_per, s_end = min(S, s_begin + s_per);
  constexpr int MV = ROW ? 1 : VEC;  // values of the [outer][inner] maps a lane needs
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < q.lanes; t += (int64_t)gridDim.x * 256) {
    int64_t mo;  // the lane's first element of the [outer][inner] maps
    int l;       // the position of the lane's first element
    if (!q.big) {
      const int r = fdiv((int)t, q.iv_div), iv = (int)t - r * q.IV;
      if constexpr (ROW) {
        mo = r, l = iv * VEC;
      } else {
        const int o = fdiv(r, q.l_div);
        l = r - o * q.L, mo = (int64_t)o * q.inner + (int64_t)iv * VEC;
      }
    } else {
      const int64_t r = t / q.IV;
      const int iv = (int)(t - r * q.IV);
      if constexpr (ROW) {
        mo = r, l = iv * VEC;
      } else {
        const int64_t o = r / q.L;
        l = (int)(r - o * q.L), mo = o * q.inner + (int64_t)iv * VEC;
      }
    }
    bool hit[VEC];
    float rc[MV];  // even: 1 / cnt is not formed - the quotient g / cnt is, per seed
    if constexpr (EVEN) {
      float xv[VEC], yv[MV];
      int cv[MV];
      ld<VEC>(x + t * VEC, xv);
      ld<MV>(y + mo, yv);
      ldi<MV>(cnt + mo, cv);
#pragma unroll
      for (int e = 0; e < VEC; ++e) hit[e] = xv[e] == yv[ROW ? 0 : e];
#pragma unroll
      for (int e = 0; e < MV; ++e) rc[e] = (float)cv[e];
    } else {
      int iw[MV];
      ldi<MV>(idx + mo, iw);
#pragma unroll
      for (int e = 0; e < VEC; ++e) hit[e] = ROW ? (l + e == iw[0]) : (l == iw[ROW ? 0 : e]);
#pragma unroll
      for (int e = 0; e < MV; ++e) rc[e] = 1.f;
    }
#pragma unroll 4
    for (int s = s_begin; s < s_end; ++s) {
      float gv[MV], d[VEC];
      ld<MV>(g + (int64_t)s * g_stride + mo, gv);
      if constexpr (EVEN) {
#pragma unroll
        for (int e = 0; e < MV; ++e) gv[e] = gv[e] / rc[e];
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) d[e] = hit[e] ? gv[ROW ? 0 : e] : 0.f;
      st<VEC>(dx + (int64_t)s * dx_stride + t * VEC, d);
    }
  }
}

// ---- host: the contract and the path of a shape ----------------------------------------------------------------------------------
struct MaxredPlan {
  int row;  // inner == 1
  int vec;
  int W;      // forward row path: lanes per row
  int s_per;  // VJP: seeds per grid.y slice
  int64_t lanes, blocks, groups;
};

// false: a shape outside the contract of the entry points
static bool maxred_shape_ok(int64_t S, int64_t outer, int64_t L, int64_t inner) {
  if (S < 1 || S >= (1ll << 31) || outer < 0 || outer >= (1ll << 31) || L < 1 || L >= (1ll << 30) || inner < 1 ||
      inner >= (1ll << 30))
    return false;
  const unsigned __int128 n = (unsigned __int128)outer * (unsigned __int128)L * (unsigned __int128)inner;
  return n < ((unsigned __int128)1 << 40) && n * (unsigned __int128)S < ((unsigned __int128)1 << 40) &&
         (unsigned __int128)outer * (unsigned __int128)inner < ((unsigned __int128)1 << 31);
}

static void maxred_plan_fwd(int64_t outer, int64_t L, int64_t inner, bool aligned, MaxredPlan* p) {
  p->row = inner == 1;
  p->s_per = 1;
  if (p->row) {
    p->vec = 0;
    p->W = pow2_ceil(L, 64);
    const int per = 256 / p->W;
    p->groups = (outer + per - 1) / per;
    p->lanes = p->groups * 256;
    p->blocks = p->groups < STREAM_MAX_BLOCKS ? p->groups : STREAM_MAX_BLOCKS;
  } else {
    p->vec = aligned && inner % 4 == 0;
    p->W = 1;
    p->groups = 0;
    p->lanes = outer * (p->vec ? inner / 4 : inner);
    p->blocks = grid_blocks(p->lanes);
  }
}

static void maxred_plan_vjp(int64_t S, int64_t outer, int64_t L, int64_t inner, bool aligned, MaxredPlan* p) {
  p->row = inner == 1;
  p->vec = aligned && (p->row ? L : inner) % 4 == 0;
  p->W = 1;
  p->groups = 0;
  p->lanes = outer * L * inner / (p->vec ? 4 : 1);
  p->blocks = grid_blocks(p->lanes);
  p->s_per = seeds_per_slice(S, p->blocks * 4);
}

static MaxredGeom maxred_geometry(const MaxredPlan& p, int64_t L, int64_t inner, bool vjp) {
  MaxredGeom q;
  q.lanes = p.lanes, q.L = (int)L, q.inner = (int)inner;
  q.IV = (int)((vjp && p.row ? L : inner) / (p.vec ? 4 : 1));
  q.big = p.lanes >= (1ll << 31);
  q.iv_div = make_fastdiv(q.IV);
  q.l_div = make_fastdiv(q.L);
  return q;
}

static int maxred_check_fwd(const float* x, int64_t outer, int64_t L, int64_t inner, const float* y, const int* idx,
                            const int* cnt, MaxredPlan* p) {
  LK_REQUIRE(x && y && idx && cnt, "lk_maxred_fwd_f32: bad arguments (null pointer)");
  LK_REQUIRE(maxred_shape_ok(1, outer, L, inner),
             "lk_maxred_fwd_f32: bad arguments (0 <= outer, 1 <= L < 2^30, 1 <= inner < 2^30, outer * inner < 2^31, "
             "outer * L * inner < 2^40)");
  const unsigned __int128 xb = (unsigned __int128)outer * L * inner * 4, ob = (unsigned __int128)outer * inner * 4;
  LK_REQUIRE(disjoint(y, ob, x, xb) && disjoint(idx, ob, x, xb) && disjoint(cnt, ob, x, xb) && disjoint(y, ob, idx, ob) &&
                 disjoint(y, ob, cnt, ob) && disjoint(idx, ob, cnt, ob),
             "lk_maxred_fwd_f32: bad arguments (y, idx and cnt overlap x or each other)");
  maxred_plan_fwd(outer, L, inner, (((uintptr_t)x | (uintptr_t)y | (uintptr_t)idx | (uintptr_t)cnt) & 15) == 0, p);
  return LK_OK;
}

static int maxred_check_vjp(const float* g, const int* idx, const float* x, const float* y, const int* cnt, int64_t S,
                            int64_t outer, int64_t L, int64_t inner, const float* dx, bool* even, MaxredPlan* p) {
  LK_REQUIRE(g && dx, "lk_maxred_vjp_f32: bad arguments (null pointer)");
  const bool ev = x && y && cnt, first = idx && !x && !y && !cnt;
  LK_REQUIRE(ev || first, "lk_maxred_vjp_f32: bad arguments (give idx alone - first maximum - or x, y and cnt - even split)");
  LK_REQUIRE(maxred_shape_ok(S, outer, L, inner),
             "lk_maxred_vjp_f32: bad arguments (1 <= S, 0 <= outer, 1 <= L < 2^30, 1 <= inner < 2^30, outer * inner < 2^31, "
             "S * outer * L * inner < 2^40)");
  const unsigned __int128 xb = (unsigned __int128)outer * L * inner * 4, ob = (unsigned __int128)outer * inner * 4;
  const unsigned __int128 db = xb * (unsigned __int128)S;
  bool clear = disjoint(dx, db, g, ob * (unsigned __int128)S);
  if (ev) clear = clear && disjoint(dx, db, x, xb) && disjoint(dx, db, y, ob) && disjoint(dx, db, cnt, ob);
  else clear = clear && disjoint(dx, db, idx, ob);
  LK_REQUIRE(clear, "lk_maxred_vjp_f32: bad arguments (dx overlaps an operand)");
  uintptr_t bits = (uintptr_t)g | (uintptr_t)dx;
  if (ev) bits |= (uintptr_t)x | (uintptr_t)y | (uintptr_t)cnt;
  else bits |= (uintptr_t)idx;
  *even = ev;
  maxred_plan_vjp(S, outer, L, inner, (bits & 15) == 0, p);
  return LK_OK;
}

}  // namespace lk

using namespace lk;

extern "C" int lk_maxred_fwd_f32(const float* x, int64_t outer, int64_t L, int64_t inner, float* y, int* idx, int* cnt,
                                 void* stream) {
  MaxredPlan p;
  const int rc = maxred_check_fwd(x, outer, L, inner, y, idx, cnt, &p);
  if (rc != LK_OK) return rc;
  if (outer == 0) return LK_OK;
  hipStream_t st = (hipStream_t)stream;
  if (p.row) {
    hipLaunchKernelGGL(maxred_fwd_row_kernel, dim3((unsigned)p.blocks), dim3(256), 0, st, x, outer, (int)L, p.W, p.groups, y,
                       idx, cnt);
    return check_launch("maxred_fwd_row_kernel");
  }
  const MaxredGeom q = maxred_geometry(p, L, inner, false);
  if (p.vec) hipLaunchKernelGGL((maxred_fwd_col_kernel<4>), dim3((unsigned)p.blocks), dim3(256), 0, st, x, q, y, idx, cnt);
  else hipLaunchKernelGGL((maxred_fwd_col_kernel<1>), dim3((unsigned)p.blocks), dim3(256), 0, st, x, q, y, idx, cnt);
  return check_launch("maxred_fwd_col_kernel");
}

extern "C" int lk_maxred_vjp_f32(const float* g, const int* idx, const float* x, const float* y, const int* cnt, int64_t S,
                                 int64_t outer, int64_t L, int64_t inner, float* dx, void* stream) {
  MaxredPlan p;
  bool even = false;
  const int rc = maxred_check_vjp(g, idx, x, y, cnt, S, outer, L, inner, dx, &even, &p);
  if (rc != LK_OK) return rc;
  if (outer == 0) return LK_OK;
  const MaxredGeom q = maxred_geometry(p, L, inner, true);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)p.blocks, (unsigned)((S + p.s_per - 1) / p.s_per));
  const int64_t gs = outer * inner, ds = outer * L * inner;
#define LK_MAXRED_VJP(V, ROW, EV) \
  hipLaunchKernelGGL((maxred_vjp_kernel<V, ROW, EV>), grid, dim3(256), 0, st, g, idx, x, y, cnt, (int)S, p.s_per, q, gs, ds, dx)
#define LK_MAXRED_VJP_E(V, ROW)            \
  do {                                     \
    if (even) LK_MAXRED_VJP(V, ROW, true); \
    else LK_MAXRED_VJP(V, ROW, false);     \
  } while (0)
  if (p.row && p.vec) LK_MAXRED_VJP_E(4, true);
  else if (p.row) LK_MAXRED_VJP_E(1, true);
  else if (p.vec) LK_MAXRED_VJP_E(4, false);
  else LK_MAXRED_VJP_E(1, false);
#undef LK_MAXRED_VJP_E
#undef LK_MAXRED_VJP
  return check_launch("maxred_vjp_kernel");
}

// row | vec << 1 | even << 2 | 64-bit lane index << 3 | log2(lanes per row) << 4 | seed-split << 7 | workgroups of grid.x << 8
extern "C" int lk_reduce_variant(int vjp, int64_t S, int64_t outer, int64_t L, int64_t inner, int even, int aligned) {
  MaxredPlan p;
  if (!maxred_shape_ok(vjp ? S : 1, outer, L, inner)) return -1;
  if (vjp) maxred_plan_vjp(S, outer, L, inner, aligned != 0, &p);
  else maxred_plan_fwd(outer, L, inner, aligned != 0, &p);
  int lg = 0;
  while ((1 << lg) < p.W) ++lg;
  return p.row | p.vec << 1 | ((vjp && even) ? 1 : 0) << 2 | (p.lanes >= (1ll << 31) ? 1 : 0) << 3 | lg << 4 |
         ((vjp && p.s_per < S) ? 1 : 0) << 7 | (int)p.blocks << 8;
}
