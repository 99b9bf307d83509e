// The small device helpers the link kernels share (lk_link.hip, lk_linkwide.hip): the wave maximum, a lane's value as a scalar and
// the register Cholesky of a diagonal block, a lane per row.  Internal.
#pragma once

#include "lk_common.h"

#include <float.h>

namespace lk {

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// the value of lane `src` (a compile-time constant after unrolling) as a scalar
__device__ __forceinline__ float lane_bcast(float v, int src) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// Right-looking Cholesky of the leading n x n block, a lane per row: a[k] is column k of this lane's row (k > lane is never used;
// rows and columns >= n are identity).  Returns 0, or j + 1 for the first pivot that is <= 0 or not finite.  On success a[] is
// the row of L, zeros above the diagonal.  The subtractions of one element run in ascending column order.
template <int N>
__device__ __forceinline__ int chol_rows(float (&a)[N], int lane, int n) {
  int bad = 0;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    if (j < n && bad == 0) {  // (uniform)
      const float d = lane_bcast(a[j], j);
      if (!(d > 0.f) || d > FLT_MAX) {
        bad = j + 1;
      } else {
        const float piv = sqrtf(d);
        const float l = lane > j ? a[j] / piv : (lane == j ? piv : 0.f);
        a[j] = l;
#pragma unroll
        for (int k = j + 1; k < N; ++k) a[k] = fmaf(-l, lane_bcast(l, k), a[k]);
      }
    }
  }
  return bad;
}

}  // namespace lk
