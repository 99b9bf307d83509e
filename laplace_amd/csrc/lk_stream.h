// What the streaming kernel families of the reverse sweep share (lk_cat, lk_slice, lk_mul, lk_gate, lk_softmax, lk_pool,
// lk_dwconv, lk_embed, lk_normtap, lk_rmsnorm, lk_normvjp, lk_norm ...): the access of VEC adjacent floats, the two-plane fp16
// read, the amax word, lane index -> coordinates, and on the host the overlap check and the grid cap.  A new family starts from
// this header, not from a copy of one of those files.  Internal.
#pragma once

#include "lk_common.h"
#include "lk_split16.h"  // f16x4

namespace lk {

// ---- VEC adjacent floats: 16-byte accesses (VEC == 4, p 16-byte aligned) or one 4-byte access (VEC == 1) ---------------------
// (the load also serves VEC == 8, as two 16-byte loads: lk_normtap.hip)
template <int VEC>
__device__ __forceinline__ void ld(const float* __restrict__ p, float (&v)[VEC]) {
  static_assert(VEC == 1 || VEC % 4 == 0, "one float or whole 16-byte vectors");
  if constexpr (VEC == 1) {
    v[0] = *p;
  } else {
#pragma unroll
    for (int q = 0; q < VEC / 4; ++q) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(p + 4 * q);
      v[4 * q] = t[0], v[4 * q + 1] = t[1], v[4 * q + 2] = t[2], v[4 * q + 3] = t[3];
    }
  }
}

template <int VEC>
__device__ __forceinline__ void st(float* __restrict__ p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    f32x4 t;
    t[0] = v[0]; t[1] = v[1]; t[2] = v[2]; t[3] = v[3];
    *reinterpret_cast<f32x4*>(p) = t;
  } else {
    *p = v[0];
  }
}

// ---- VEC adjacent elements of a split tensor's two fp16 planes (8-byte loads of four halves where VEC == 4) --------------------
// float(h) + float(l): the form of a kernel that applies the power-of-two scale once, to a sum of such values
template <int VEC>
__device__ __forceinline__ void ld_split(const _Float16* __restrict__ h, const _Float16* __restrict__ l, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const f16x4 a = *reinterpret_cast<const f16x4*>(h), b = *reinterpret_cast<const f16x4*>(l);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (float)a[e] + (float)b[e];
  } else {
    v[0] = (float)*h + (float)*l;
  }
}
// (float(h) + float(l)) * scale; scale is a power of two, so the product is exact
template <int VEC>
__device__ __forceinline__ void ld_split(const _Float16* __restrict__ h, const _Float16* __restrict__ l, float scale,
                                         float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const f16x4 a = *reinterpret_cast<const f16x4*>(h), b = *reinterpret_cast<const f16x4*>(l);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ((float)a[e] + (float)b[e]) * scale;
  } else {
    v[0] = ((float)*h + (float)*l) * scale;
  }
}

// ---- the amax word: max|.| as the bit pattern of a non-negative float (such floats order like their bit patterns) --------------
__device__ __forceinline__ unsigned wave_max_bits(float m) {  // the maximum over the wave, in every lane
  unsigned b = __float_as_uint(m);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) b = max(b, (unsigned)__shfl_xor((int)b, off, 64));
  return b;
}
// one atomic per wave, none where the wave's maximum is zero
__device__ __forceinline__ void wave_amax(float m, unsigned* __restrict__ amax) {
  const unsigned b = wave_max_bits(m);
  if (amax != nullptr && (threadIdx.x & 63) == 0 && b) atomicMax(amax, b);
}

// ---- lane index -> coordinates ---------------------------------------------------------------------------------------------------
// a column range [c0, c0 + Cs) of the rows of a [R][Ct] matrix (lk_cat.hip, lk_slice.hip)
struct ColSliceGeom {
  int64_t Ct, c0, Cs, lanes;
  int CV;   // lanes per row
  int big;  // the lane index does not fit 31 bits: 64-bit division
  FastDiv cv_div;
};
// -> (row, first column of the lane inside the range)
template <int VEC>
__device__ __forceinline__ void col_where(const ColSliceGeom& q, int64_t t, int64_t& r, int& c) {
  if (!q.big) {
    const int ri = fdiv((int)t, q.cv_div);
    r = ri;
    c = ((int)t - ri * q.CV) * VEC;
  } else {
    r = t / q.CV;
    c = (int)(t - r * q.CV) * VEC;
  }
}
// -> (channel vector, column, row, image) of a [.., rows, cols, CV] map; GEOM has CV, big, cv_div, w_div, h_div (lk_pool.hip,
// lk_dwconv.hip)
template <typename GEOM>
__device__ __forceinline__ void map_where(const GEOM& q, int64_t t, int rows, int cols, int& cv, int& col, int& row, int64_t& n) {
  if (!q.big) {
    const int ti = (int)t, pix = fdiv(ti, q.cv_div), r = fdiv(pix, q.w_div), ni = fdiv(r, q.h_div);
    cv = ti - pix * q.CV;
    col = pix - r * cols;
    row = r - ni * rows;
    n = ni;
  } else {
    const int64_t pix = t / q.CV, r = pix / cols;
    cv = (int)(t - pix * q.CV);
    col = (int)(pix - r * cols);
    n = r / rows;
    row = (int)(r - n * rows);
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
constexpr int64_t STREAM_MAX_BLOCKS = 256 * 8;  // 256 CUs x 8 workgroups of 256 threads

// workgroups of 256 lanes of a grid that strides over `lanes`
static inline int64_t grid_blocks(int64_t lanes) {
  const int64_t need = (lanes + 255) / 256;
  return need < STREAM_MAX_BLOCKS ? need : STREAM_MAX_BLOCKS;
}

// [p, p + p_bytes) and [q, q + q_bytes) do not meet
static inline bool disjoint(const void* p, unsigned __int128 p_bytes, const void* q, unsigned __int128 q_bytes) {
  const unsigned __int128 p0 = (uintptr_t)p, q0 = (uintptr_t)q;
  return p0 + p_bytes <= q0 || q0 + q_bytes <= p0;
}

}  // namespace lk
