// Vector access and the amax word of the row kernels that keep a statistics row on chip across the seeds (lk_normvjp.hip,
// lk_rmsnorm.hip).  Internal.
#pragma once

#include "lk_common.h"

namespace lk {

template <int VEC>
__device__ __forceinline__ void nv_ld(const float* __restrict__ p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  } else {
    v[0] = *p;
  }
}

template <int VEC>
__device__ __forceinline__ void nv_st(float* __restrict__ p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    f32x4 t;
    t[0] = v[0]; t[1] = v[1]; t[2] = v[2]; t[3] = v[3];
    *reinterpret_cast<f32x4*>(p) = t;
  } else {
    *p = v[0];
  }
}

// one atomic per wave: the lanes' maxima of |dx| (non-negative floats order like their bit patterns)
__device__ __forceinline__ void nv_wave_amax(float m, unsigned* __restrict__ amax) {
  unsigned b = __float_as_uint(m);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) b = max(b, (unsigned)__shfl_xor((int)b, off, 64));
  if (amax != nullptr && (threadIdx.x & 63) == 0 && b) atomicMax(amax, b);
}

}  // namespace lk
