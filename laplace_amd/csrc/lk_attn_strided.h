// The part of the contract that lk_attn_fwd_strided_f32 / lk_attn_vjp_strided_f32 (csrc/lk_attn.hip) add to that of the layout-1 entry
// points: q, k, v are read as [B][T][H][D] with a row stride of ldq floats (the slices of one packed [B][T][3 H D] projection:
// q = qkv, k = qkv + H D, v = qkv + 2 H D, ldq = 3 H D), dq, dk, dv are written as [S][B][T][H][D] with a row stride of ldd floats and
// may interleave in one [S][B][T][3 H D] buffer.  The shape, the pointers and the overlap of an output with an input are checked by
// the checkers of lk_attn.hip on the extents that `attn_strided_bytes` gives.
#pragma once
#include "lk_stream.h"

namespace lk {

// bytes from the first to one past the last element of `rows` rows of H D floats with a row stride of ld floats
static inline size_t attn_strided_bytes(int64_t rows, int64_t ld, int64_t HD) {
  return rows > 0 ? (size_t)((rows - 1) * ld + HD) * sizeof(float) : 0;
}

static int attn_check_strides(const char* fn, int64_t S, int64_t B, int64_t H, int64_t T, int64_t D, int64_t ldq, int64_t ldd) {
  const int64_t HD = H * D;
  LK_REQUIRE(ldq >= HD && ldd >= HD && ldq % 4 == 0 && ldd % 4 == 0 && ldq < (1ll << 40) && ldd < (1ll << 40),
             "%s: row stride out of range (ldq >= H * D, ldd >= H * D, both multiples of 4)", fn);
  LK_REQUIRE((unsigned __int128)(B * T) * ldq < ((unsigned __int128)1 << 40) &&
                 (unsigned __int128)(S * B) * T * ldd < ((unsigned __int128)1 << 40),
             "%s: too many elements (B * T * ldq < 2^40, S * B * T * ldd < 2^40)", fn);
  return LK_OK;
}

// two outputs of `rows` rows with the same row stride share no element: apart by the whole extent, or interleaved so that the
// H D floats of a row of one end before a row of the other begins
static int attn_check_interleave(const char* fn, const float* const* out, int n_out, int64_t rows, int64_t ld, int64_t HD) {
  const size_t extent = attn_strided_bytes(rows, ld, HD);
  for (int i = 0; i < n_out; ++i)
    for (int j = i + 1; j < n_out; ++j) {
      if (disjoint(out[i], extent, out[j], extent)) continue;
      const uintptr_t a = (uintptr_t)out[i], b = (uintptr_t)out[j];
      const uint64_t r = (uint64_t)((a > b ? a - b : b - a) % ((uint64_t)ld * sizeof(float)));
      LK_REQUIRE(r >= (uint64_t)HD * sizeof(float) && r + (uint64_t)HD * sizeof(float) <= (uint64_t)ld * sizeof(float),
                 "%s: the outputs overlap each other (they may interleave: rows of H * D floats, ldd apart)", fn);
    }
  return LK_OK;
}

}  // namespace lk
