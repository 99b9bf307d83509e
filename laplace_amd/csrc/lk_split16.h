// The split-fp16 fixed-point form, once: power-of-two scales, the two-piece split of an fp32 value, and the element-wise VJP
// arithmetic on eight channels that the convolution epilogues (lk_conv.hip) and vjp_nhwc_split_kernel (lk_sweep16.hip) share.
// (The form itself — why two fp16 planes, what is dropped — is described at the head of lk_conv.hip.)
#pragma once

#include "lk_common.h"

namespace lk {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// ---- power-of-two scaling -------------------------------------------------------------------------------------------
// exponent s such that amax * 2^s lies in [2^14, 2^15)  (clamped so that 2^s and every scaled element stay finite)
__device__ __forceinline__ int scale_exp_for(float amax) {
  int be = (int)((__float_as_uint(amax) >> 23) & 0xffu);
  if (be == 0) be = 1;  // zero / subnormal tensors: largest scale that is safe for anything below 2^-126
  int s = 14 - (be - 127);
  return s > 120 ? 120 : s;
}
__device__ __forceinline__ float exp2i(int s) {  // 2^s, -126 <= s <= 127 (the raw form: no clamp)
  return __uint_as_float((unsigned)(127 + s) << 23);
}
__device__ __forceinline__ float exp2i_sat(int s) {  // 2^s with s clamped to [-126, 127]
  return exp2i(s < -126 ? -126 : (s > 127 ? 127 : s));
}
// 2^-s, the factor that takes a scale exponent off again.  NOT exp2i_sat(-s): a scale exponent is at most 120, so only the
// clamp from below can bind, and that is all the sites that un-scale have ever computed (one operation less per site).
__device__ __forceinline__ float exp2i_neg(int s) { return exp2i(-s < -126 ? -126 : -s); }
// 2^(15 - s): what bounds a tensor that was split with exponent s (max|x| 2^s < 2^15).  The values of exp2i_sat(15 - s); spelled
// out on 15 - s because hipcc then keeps a uniform s in scalar registers (s_min + s_cselect) where the clamp of an argument
// becomes a v_med3_i32: the kernels that sit at their register limit keep the form they were tuned with.
__device__ __forceinline__ float bound_of_sexp(int s) { return exp2i(15 - s < -126 ? -126 : (15 - s > 127 ? 127 : 15 - s)); }

// ---- x = h + l, both fp16 (+ <= 2^-22 |x|, 2^-25 absolute) ---------------------------------------------------------------
// The value is made opaque before it is split: h and the residual must come from the SAME fp32 value.  Left to itself hipcc
// forms the stored h from the fp32-rounded product but the residual from a fused fp16(v * mult - h') with h' = fp16 of the
// EXACT product (v_fma_mix); the two h differ at rounding ties and the pair then misses the value by a whole fp16 ulp.
// Returns the opaque value (what max|.| is tracked on).
__device__ __forceinline__ float split2_scaled(float xs, _Float16& h, _Float16& l) {
  asm volatile("" : "+v"(xs));
  h = (_Float16)xs;
  l = (_Float16)(xs - (float)h);
  return xs;
}
__device__ __forceinline__ void split2(float x, float sc, _Float16& h, _Float16& l) { split2_scaled(x * sc, h, l); }
template <typename V>  // the same into element j of two fp16 vectors
__device__ __forceinline__ float split2_at(float xs, V& h, V& l, int j) {
  asm volatile("" : "+v"(xs));
  const _Float16 hh = (_Float16)xs;
  h[j] = hh;
  l[j] = (_Float16)(xs - (float)hh);
  return xs;
}

// ---- x = h + m + l exactly, three bf16 pieces kept as the high halves of fp32 words (truncation keeps the subtractions exact)
__device__ __forceinline__ void split3(float x, unsigned& h, unsigned& m, unsigned& l) {
  h = __float_as_uint(x) & 0xffff0000u;
  const float r1 = x - __uint_as_float(h);
  m = __float_as_uint(r1) & 0xffff0000u;
  l = __float_as_uint(r1 - __uint_as_float(m));  // at most 8 significant bits are left: exact in bf16
}
__device__ __forceinline__ unsigned pack_hi16(unsigned lo_elem, unsigned hi_elem) {
  return (lo_elem >> 16) | (hi_elem & 0xffff0000u);
}

// ---- element-wise VJP on eight channels:  o = (v + addend) * M * scale[channel], as a split tensor ------------------------
// Scale of the result from a GUARANTEED bound known before the launch (a loose bound only costs fixed-point range):
//   bound = (base + 2^(15 - add_sexp)) * max|M| * max|scale|
// Every optional factor comes as (is the tensor there — its pointer as the site holds it, or a flag —, its device word); max|M| counts for fp32 multipliers only.
// VALU_CLAMP: the strided kernel and vjp_nhwc_split_kernel clamp both powers of two of the addend as exp2i_sat does; the generic
// and window kernels use bound_of_sexp and exp2i_neg (the un-scale factor clamped from below only).  Equal for every exponent a
// producer here can emit (-114 .. 120); both are kept because they are different instructions.
struct VjpScale {
  int so;        // scale exponent of the result
  float sc_out;  // 2^so
  float inv2;    // 2^-add_sexp (0 without an addend)
};
template <bool VALU_CLAMP, typename ADD, typename MASK, typename SCALE>
__device__ __forceinline__ VjpScale vjp_bound_scale(float bound, ADD add, const int* add_sexp, MASK mask, int mask_float,
                                                    const unsigned* mult_amax, SCALE scale, const unsigned* scale_amax) {
  VjpScale r;
  r.inv2 = 0.f;
  if (add) {
    const int s2 = add_sexp[0];
    bound += VALU_CLAMP ? exp2i_sat(15 - s2) : bound_of_sexp(s2);
    r.inv2 = VALU_CLAMP ? exp2i_sat(-s2) : exp2i_neg(s2);
  }
  if (mask && mask_float && mult_amax) bound *= __uint_as_float(mult_amax[0]);
  if (scale) bound *= __uint_as_float(scale_amax[0]);
  r.so = scale_exp_for(bound);
  r.sc_out = exp2i(r.so);
  return r;
}
// The eight factors mult[j] = 2^so * M[j] * scale[channel j], built in steps on an array the site has filled with 2^so: which
// factors exist — and where their eight values lie — is the site's business and stays in its control flow, so that each one's
// address arithmetic and load sit inside the branch that uses them; the arithmetic is here.  (The fill is the site's own loop on
// purpose: as a helper it is optimised on its own into one eight-wide store before it is inlined, hipcc then keeps `mult` as a
// vector through the unrolled chunk loop, and every fused kernel grew by eight instructions per chunk and two registers.)
__device__ __forceinline__ void vjp_mult8_times(float (&mult)[8], const float* f8) {  // fp32 multipliers or channel scales (16-byte aligned)
  const f32x4 a = *reinterpret_cast<const f32x4*>(f8), b = *reinterpret_cast<const f32x4*>(f8 + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) mult[j] *= a[j], mult[4 + j] *= b[j];
}
__device__ __forceinline__ void vjp_mult8_mask(float (&mult)[8], uint2 bytes) {  // a zero mask byte zeroes the factor
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!((bytes.x >> (8 * j)) & 0xffu)) mult[j] = 0.f;
    if (!((bytes.y >> (8 * j)) & 0xffu)) mult[4 + j] = 0.f;
  }
}
// v += the split addend (un-scaled by inv2 = 2^-add_sexp).  Addend, factors and split are separate calls, made in the order each
// site has always made them (the window form builds its factors once per tile).
__device__ __forceinline__ void vjp_add8(float (&v)[8], const f16x8& add_h, const f16x8& add_l, float inv2) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] += ((float)add_h[j] + (float)add_l[j]) * inv2;
}
// v * mult, split, max|.| of the scaled values folded into vmax.  KEEP: the byte mask is applied HERE, as `byte ? v * mult : 0`
// (the window form), not as a zero factor in mult (the others): the same bits for finite v, but a zero factor turns an Inf or
// NaN accumulator into NaN where the select gives 0 — both behaviours are kept as they were.
template <bool KEEP = false>
__device__ __forceinline__ void vjp_chunk8(const float (&v)[8], const float (&mult)[8], unsigned& vmax, f16x8& h, f16x8& l,
                                           uint2 keep = make_uint2(0u, 0u)) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float xs = v[j] * mult[j];
    if constexpr (KEEP) {
      const bool kept = ((j < 4 ? keep.x >> (8 * j) : keep.y >> (8 * (j - 4))) & 0xffu) != 0;
      xs = kept ? xs : 0.f;
    }
    xs = split2_at(xs, h, l, j);
    vmax = max(vmax, __float_as_uint(xs) & 0x7fffffffu);
  }
}

}  // namespace lk
