// Tile products of the weight-sharing quadratic forms (lk_quadconv.hip, lk_grid.hip): the 32x32 tile (rows o, one column i
// per lane) of  sum_l u[c][:, l] v[:, l]^T  for CT outputs of one sample, held in MFMA accumulators.
#pragma once

#include "lk_common.h"
#include "lk_split16.h"

namespace lk {

constexpr int QC_KC = 16;  // positions per chunk

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct QcOperands {  // one tile's operands: sample base pointers, first row, this lane's column
  const float* un;   // u[n]: [C][Do][L] with the outputs `cs` elements apart (Do * L when u is sample-major)
  const float* vn;   // v[n]: [Dk][L]
  int o0, icol;
  unsigned cs;
};

// LDS arena of one workgroup, reinterpreted by the two tile products below
template <int CT>
struct QcLds {
  static constexpr int BYTES = CT * 6144;  // split-bf16: [2][3 pieces][CT][32 o][16 k] bf16; fp32: [2][CT][16 k][32 o] (4096 CT)
};

// ---- generic tile product (any L, any alignment): fp32 operands, v_mfma_f32_32x32x2_f32 --------------------------
// acc[c] = the 32x32 tile (rows o0.., this wave's columns icol) of  sum_l u[c][:, l] v[:, l]^T  for all CT outputs of
// one sample.  A operand (u, all outputs) through double-buffered LDS shared by the 4 waves, B operand straight from
// memory.  Used when the positions cannot be read four at a time.
template <int CT>
__device__ __forceinline__ void qc_tile_gemm(const QcOperands& t, int C, int Do, int Dk, int L, char* lds,
                                             f32x16 (&acc)[CT]) {
  constexpr int NA = 2 * CT;  // staged dwords per thread per chunk: CT * QC_KC * 32 / 256
  float(*sA)[CT][QC_KC][32] = reinterpret_cast<float(*)[CT][QC_KC][32]>(lds);
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
#pragma unroll
  for (int c = 0; c < CT; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

  float ra[NA], rb[QC_KC / 2];
  auto fetch = [&](int l0) {
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const int e = tid + 256 * j, o = e & 31, ll = (e >> 5) & (QC_KC - 1), c = e >> 9;
      const bool ok = c < C && l0 + ll < L && t.o0 + o < Do;
      // 32-bit offsets from the sample's (uniform) base pointer: the host checks C*L*Do and L*Dk < 2^29
      ra[j] = ok ? t.un[(unsigned)(c * t.cs + (t.o0 + o) * L + l0 + ll)] : 0.f;
    }
#pragma unroll
    for (int kk = 0; kk < QC_KC / 2; ++kk) {
      const int l = l0 + 2 * kk + hi;
      rb[kk] = (l < L && t.icol < Dk) ? t.vn[(unsigned)(t.icol * L + l)] : 0.f;
    }
  };
  fetch(0);
  int buf = 0;
  for (int l0 = 0; l0 < L; l0 += QC_KC) {
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const int e = tid + 256 * j;
      sA[buf][e >> 9][(e >> 5) & (QC_KC - 1)][e & 31] = ra[j];
    }
    float b[QC_KC / 2];
#pragma unroll
    for (int kk = 0; kk < QC_KC / 2; ++kk) b[kk] = rb[kk];
    __syncthreads();
    if (l0 + QC_KC < L) fetch(l0 + QC_KC);
    float a_cur[CT], a_nxt[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) a_cur[c] = sA[buf][c][hi][lo];
#pragma unroll
    for (int kk = 0; kk < QC_KC / 2; ++kk) {
      if (kk + 1 < QC_KC / 2) {
#pragma unroll
        for (int c = 0; c < CT; ++c) a_nxt[c] = sA[buf][c][2 * kk + 2 + hi][lo];
      }
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[c], b[kk], acc[c], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int c = 0; c < CT; ++c) a_cur[c] = a_nxt[c];
    }
    buf ^= 1;  // the other buffer was last read two chunks ago: one barrier per chunk suffices
  }
  __syncthreads();  // every wave is done with both LDS buffers before the caller's next tile refills them
}

// ---- the tile product on the bf16 matrix cores at fp32 accuracy (L % 4 == 0) --------------------------------------
// Every operand is split ONCE into three bf16 pieces, x = h + m + l exactly (truncation keeps the subtractions exact),
// and  x y ~= h h' + h m' + m h' + m m' + h l' + l h'  (dropped terms <= 3 * 2^-24 |x y|): six
// v_mfma_f32_32x32x16_bf16 (32 cycles, 16 positions) instead of eight v_mfma_f32_32x32x2_f32 (64 cycles, 2 positions)
// per chunk and output -- 192 matrix-pipe cycles where the fp32 form needs 512.  Both operands are position-contiguous
// in memory, which is what a lane of the bf16 MFMA wants (8 consecutive k): the A chunk is staged as float4s along
// the positions, split by the staging thread and kept in LDS as [piece][output][row o][16 k]; the B operand is this
// lane's own 8 positions of column icol, split in registers.  The pipeline runs across tiles: during a tile's last
// chunk the first chunk of the NEXT tile (other rows / columns, or the next sample) is fetched; loads are issued raw
// from a clamped address and zeroed where they are consumed.
// (split3 / pack_hi16: lk_split16.h)

template <int CT>
struct QcStage {  // raw operands in flight: this thread's float4 slots of the A chunk, this lane's 8 positions of B
  f32x4 ra[(CT + 1) / 2];
  f32x4 rb[2];
};

// staging coordinates of thread tid: float4 slot e4 = tid + 256 j  ->  k4 = 4 (tid & 3), row o = (tid >> 2) & 31,
// output c = (tid >> 7) + 2 j
template <int CT>
__device__ __forceinline__ void qc_fetch_b6(QcStage<CT>& st, int j_lo, int j_hi, int h_lo, int h_hi, const QcOperands& t,
                                            int l0, int C, int Do, int Dk, int L) {
  const int tid = threadIdx.x, hi = (tid & 63) >> 5;
  const int k4 = 4 * (tid & 3), o = (tid >> 2) & 31, c0 = tid >> 7;
#pragma unroll
  for (int j = j_lo; j < j_hi; ++j) {
    const bool ok = t.o0 + o < Do && c0 + 2 * j < C && l0 + k4 < L;
    const unsigned off = ok ? (unsigned)((c0 + 2 * j) * t.cs + (t.o0 + o) * L + l0 + k4) : 0u;
    st.ra[j] = *reinterpret_cast<const f32x4*>(t.un + off);
  }
#pragma unroll
  for (int h = h_lo; h < h_hi; ++h) {
    const int l = l0 + 8 * hi + 4 * h;
    const bool ok = t.icol < Dk && l < L;
    st.rb[h] = *reinterpret_cast<const f32x4*>(t.vn + (ok ? (unsigned)(t.icol * L + l) : 0u));
  }
}

// On entry `st` holds chunk 0 of `cur`; on exit chunk 0 of `nxt` (if has_next).
template <int CT>
__device__ __forceinline__ void qc_tile_gemm_b6(const QcOperands& cur, const QcOperands& nxt, bool has_next, int C,
                                                int Do, int Dk, int L, char* lds, f32x16 (&acc)[CT], QcStage<CT>& st) {
  constexpr int NA4 = (CT + 1) / 2;        // float4 slots per thread per chunk: CT * 32 * 4 / 256
  constexpr int PIECE = CT * 32 * 16 * 2;  // bytes of one piece of one buffer
  const int tid = threadIdx.x, lane = tid & 63, lo = lane & 31, hi = lane >> 5;
  const int k4 = 4 * (tid & 3), o = (tid >> 2) & 31, c0 = tid >> 7;
#pragma unroll
  for (int c = 0; c < CT; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
  const bool okO = cur.o0 + o < Do, okI = cur.icol < Dk;
  int buf = 0;
  for (int l0 = 0; l0 < L; l0 += QC_KC) {
    char* wr = lds + buf * 3 * PIECE;
#pragma unroll
    for (int j = 0; j < NA4; ++j)
      if (c0 + 2 * j < CT) {
        const bool ok = okO && c0 + 2 * j < C && l0 + k4 < L;
        const f32x4 x = ok ? st.ra[j] : f32x4{0.f, 0.f, 0.f, 0.f};
        unsigned h[4], m[4], l[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) split3(x[q], h[q], m[q], l[q]);
        char* dst = wr + (((c0 + 2 * j) * 32 + o) * 16 + k4) * 2;
        *reinterpret_cast<u32x2*>(dst) = u32x2{pack_hi16(h[0], h[1]), pack_hi16(h[2], h[3])};
        *reinterpret_cast<u32x2*>(dst + PIECE) = u32x2{pack_hi16(m[0], m[1]), pack_hi16(m[2], m[3])};
        *reinterpret_cast<u32x2*>(dst + 2 * PIECE) = u32x2{pack_hi16(l[0], l[1]), pack_hi16(l[2], l[3])};
      }
    // this lane's B operand: positions l0 + 8 hi .. + 7 of column icol, as three bf16x8
    u32x4 bp[3];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const bool ok = okI && l0 + 8 * hi + 4 * hh < L;
      const f32x4 x = ok ? st.rb[hh] : f32x4{0.f, 0.f, 0.f, 0.f};
      unsigned h[4], m[4], l[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) split3(x[q], h[q], m[q], l[q]);
      bp[0][2 * hh] = pack_hi16(h[0], h[1]);
      bp[0][2 * hh + 1] = pack_hi16(h[2], h[3]);
      bp[1][2 * hh] = pack_hi16(m[0], m[1]);
      bp[1][2 * hh + 1] = pack_hi16(m[2], m[3]);
      bp[2][2 * hh] = pack_hi16(l[0], l[1]);
      bp[2][2 * hh + 1] = pack_hi16(l[2], l[3]);
    }
    bf16x8 b[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) b[p] = __builtin_bit_cast(bf16x8, bp[p]);
    __syncthreads();
    // what travels during this chunk: the tile's next chunk, or chunk 0 of the next tile -- chosen with uniform
    // selects, not branches; the very last chunk of a workgroup re-reads its own chunk 0 for nothing
    const bool more = l0 + QC_KC < L;
    const QcOperands src = more ? cur : (has_next ? nxt : cur);
    const int lsrc = more ? l0 + QC_KC : 0;
    const char* rd = lds + buf * 3 * PIECE + (lo * 16 + 8 * hi) * 2;  // this lane's (row, k half) in output 0, piece 0
    bf16x8 a_cur[3], a_nxt[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) a_cur[p] = *reinterpret_cast<const bf16x8*>(rd + p * PIECE);
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      if (c + 1 < CT) {
#pragma unroll
        for (int p = 0; p < 3; ++p) a_nxt[p] = *reinterpret_cast<const bf16x8*>(rd + p * PIECE + (c + 1) * 32 * 16 * 2);
      }
      // the next chunk's loads go out one per output between the MFMA groups
      qc_fetch_b6<CT>(st, c, c < NA4 ? c + 1 : c, c < 2 ? c : 2, (c < 2 ? c + 1 : 2) + (CT == 1 ? 1 : 0), src, lsrc, C, Do,
                      Dk, L);
      f32x16 d = acc[c];
      d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_cur[2], b[0], d, 0, 0, 0);  // small terms first
      d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_cur[0], b[2], d, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_cur[1], b[1], d, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_cur[1], b[0], d, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_cur[0], b[1], d, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_cur[0], b[0], d, 0, 0, 0);
      acc[c] = d;
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int p = 0; p < 3; ++p) a_cur[p] = a_nxt[p];
    }
    buf ^= 1;  // the other buffer was last read two chunks ago: one barrier per chunk suffices
  }
  __syncthreads();
}

// ---- host side: which instantiation a shape launches ------------------------------------------------------------------
// The ONE copy of the selection rules: the launchers of lk_quadconv.hip / lk_grid.hip and lk_quadform_shared_variant (the
// query the tests read) all go through these.
inline int64_t qc_ntiles(int64_t Do, int64_t Dk) { return ((Do + 31) / 32) * ((Dk + 127) / 128); }

inline int qc_class_tile(int64_t C) {
  static const int tiles[] = {1, 2, 3, 4, 5, 6, 8, 10};  // 12 outputs would spill accumulators
  for (int t : tiles)
    if (C <= t) return t;
  return 0;
}

// workgroups per sample of the quadratic-form kernels (fp32 operands and planes)
inline int qc_split(int64_t B, int64_t Do, int64_t Dk) {
  const int64_t ntiles = qc_ntiles(Do, Dk);
  int64_t want = (2048 + B - 1) / B;
#ifdef LK_QC_MIN_SPLIT
  if (want < LK_QC_MIN_SPLIT) want = LK_QC_MIN_SPLIT;
#endif
  if (want < 1) want = 1;
  return (int)(want < ntiles ? want : ntiles);
}

// workgroups per tile of diag_ggn_shared_kernel (each walks the samples sp, sp + nsplit, ...)
inline int dg_split(int64_t B, int64_t Do, int64_t Dk) {
  const int64_t ntiles = qc_ntiles(Do, Dk);
  int64_t want = (1024 + ntiles - 1) / ntiles;
  if (want < 1) want = 1;
  return (int)(want < B ? want : (B < 1 ? 1 : B));
}

// output block of one launch of the weight-sharing grid kernel, and its workgroups per sample
inline int grid_class_tile(int64_t C) { return C <= 1 ? 1 : C <= 2 ? 2 : C <= 5 ? 5 : 10; }

inline int grid_split(int64_t B, int64_t Do, int64_t Dk) {
  const int64_t ntiles = qc_ntiles(Do, Dk);
  int64_t want = (2048 + B - 1) / B;
  if (want < 1) want = 1;
  return (int)(want < ntiles ? want : ntiles);
}

inline bool qc_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ARITH of the fp32-operand kernels: 1 (three-piece bf16, positions read four at a time) needs whole float4s
inline int qc_arith(int64_t L, bool aligned16) { return (L % 4 == 0) && aligned16 ? 1 : 0; }

// quadform_conv_planes_kernel<CT, OCC, SUB>, the eigenvalues in LDS or not, workgroups per sample
struct QpVariant {
  int ct, occ, sub, w_in_lds, split;
};

inline QpVariant qp_variant(int64_t B, int64_t C, int64_t Do, int64_t Dk, int64_t L) {
  QpVariant q;
  q.ct = qc_class_tile(C);
  const size_t w_bytes = (size_t)(Do + Dk) * sizeof(float);
  q.w_in_lds = w_bytes <= 40960 ? 1 : 0;  // (the eigenvalues behind the ring: ResNet-18's widest layer needs 20 KB)
  // two workgroups per CU only where the eigenvalues fit beside two rings (see lk_kron_quadform_shared_planes_f16x2)
  q.occ = w_bytes <= 24576 ? 2 : 1;
  // one-chunk tiles (4 x 4 maps): the sub-tile form with two-wide pair sums (see the kernel; -DLK_QC_NO_SUB: development build)
#ifdef LK_QC_NO_SUB
  q.sub = 0;
#else
  q.sub = q.occ == 2 && q.w_in_lds && L == 16 ? 1 : 0;
#endif
  q.split = qc_split(B, Do, Dk);
  return q;
}

}  // namespace lk
