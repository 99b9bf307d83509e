// Static, separable, linear resampling of the last two dims (nn.Upsample / F.interpolate in every 1-D and 2-D mode, F.pad and the
// padding modules in every mode) for the seed-batched reverse sweep.  Per image plane the operation is y = Mh x Mw^T + const with
// sparse static axis matrices Mh [OH][H] and Mw [OW][W]; its VJP for all seeds is
//   dx[p][h][w] = sum_{j in T_h(h)} sum_{i in T_w(w)} wh[j] * ww[i] * g[p][idx_h[j]][idx_w[i]],     p over the P = S B C planes
// with T_h, T_w the TRANSPOSED tap lists in CSR form (ptr [L + 1], idx ascending, w): the outputs that read an input.
// Replaces, in the reverse pass of laplace/curvature/curvlinops.py:87-100 and curvature.py:88-129 through such an operation as stock
// torch runs it once per seed, upsample_*_backward / reflection_pad*_backward / replication_pad*_backward (atomics: the order of
// the additions changes from run to run) or a zero fill and a strided copy (constant pad).
//
// A lane owns VEC adjacent pixels of a row of a [H][W] plane (lanes run along w).  It reads the taps of its pixels ONCE - into
// registers when every list has at most RS_REG entries (x2 nearest and bilinear, every pad; decided per lane), else it walks the
// tables, which the scalar / L1 caches hold - and then walks the planes of its slice of P, RS_PL planes per pass with their g loads
// in flight together.  The sum runs oh ascending, then ow, as  acc += wh * (sum_i ww * g): one owner per dx element, plain
// stores, no atomics, repeated runs give the same bits.  Every dx element is written; an input that no output reads receives
// +0.0f (the caller fills nothing).  16-byte stores where W % 4 == 0 and dx is aligned, 4-byte stores otherwise (g is read by
// 4-byte loads: adjacent pixels read different outputs).  One plane with few pixels: the planes are split into slices over
// grid.y, and where a plane has at most 128 lanes a workgroup takes 256 / lanes slices side by side, so that its waves are full.
// The reuse of g (up to taps_h * taps_w lanes read an element) is left to the caches: a workgroup reads a window of at most a
// few rows of one plane.  Minimal traffic: 4 P (OH OW + H W) bytes.
// The tables are not validated on the device; what is free is done: a list is cut at LK_RESAMPLE_MAX_TAPS entries and an index
// is clamped into the plane, so that no table can make the kernel read outside g or write outside dx.
#include "lk_stream.h"

namespace lk {

constexpr int RS_PL = 4;   // planes per pass (their g loads are in flight together)
constexpr int RS_REG = 4;  // taps per list that a lane keeps in registers

struct ResampleGeom {
  int H, W, OH, OW, WV;  // WV: lanes per row
  int big;               // the lane index does not fit 31 bits: 64-bit division
  int G;                 // slices of planes a workgroup takes side by side (> 1: one plane has at most 128 lanes)
  int64_t lanes;         // of one plane
  FastDiv wv_div, lanes_div;
};

struct ResampleTables {
  const int *ptr_h, *idx_h, *ptr_w, *idx_w;
  const float *w_h, *w_w;
};

__device__ __forceinline__ int rs_clamp(int i, int n) { return min(max(i, 0), n - 1); }

// the planes [p_begin, p_end) of the lane's pixels; REG: the taps are held in registers (every list <= RS_REG entries)
template <int VEC, bool REG>
__device__ __forceinline__ void resample_planes(const float* __restrict__ g, const ResampleGeom& q, const ResampleTables& t,
                                                int hb, int nh, const int (&wb)[VEC], const int (&nw)[VEC], int64_t p_begin,
                                                int64_t p_end, float* __restrict__ dp) {
  const int64_t gplane = (int64_t)q.OH * q.OW, dplane = (int64_t)q.H * q.W;
  int64_t ih[REG ? RS_REG : 1];  // (row offsets: OH * OW may pass 2^31)
  int iw[VEC][REG ? RS_REG : 1];
  float ah[REG ? RS_REG : 1], aw[VEC][REG ? RS_REG : 1];
  if constexpr (REG) {
#pragma unroll
    for (int j = 0; j < RS_REG; ++j) {
      const bool on = j < nh;
      ih[j] = on ? (int64_t)rs_clamp(t.idx_h[hb + j], q.OH) * q.OW : 0;
      ah[j] = on ? t.w_h[hb + j] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e)
#pragma unroll
      for (int i = 0; i < RS_REG; ++i) {
        const bool on = i < nw[e];
        iw[e][i] = on ? rs_clamp(t.idx_w[wb[e] + i], q.OW) : 0;
        aw[e][i] = on ? t.w_w[wb[e] + i] : 0.f;
      }
  }
  for (int64_t p0 = p_begin; p0 < p_end; p0 += RS_PL) {
    float acc[RS_PL][VEC];
#pragma unroll
    for (int k = 0; k < RS_PL; ++k)
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[k][e] = 0.f;
    const float* gp = g + p0 * gplane;
    if constexpr (REG) {
#pragma unroll
      for (int j = 0; j < RS_REG; ++j) {
        if (j < nh) {
          float row[RS_PL][VEC];
#pragma unroll
          for (int k = 0; k < RS_PL; ++k)
#pragma unroll
            for (int e = 0; e < VEC; ++e) row[k][e] = 0.f;
#pragma unroll
          for (int e = 0; e < VEC; ++e)
#pragma unroll
            for (int i = 0; i < RS_REG; ++i) {
              if (i < nw[e]) {
                float gv[RS_PL];
#pragma unroll
                for (int k = 0; k < RS_PL; ++k) gv[k] = p0 + k < p_end ? gp[k * gplane + ih[j] + iw[e][i]] : 0.f;
#pragma unroll
                for (int k = 0; k < RS_PL; ++k) row[k][e] += aw[e][i] * gv[k];
              }
            }
#pragma unroll
          for (int k = 0; k < RS_PL; ++k)
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[k][e] += ah[j] * row[k][e];
        }
      }
    } else {
      for (int j = 0; j < nh; ++j) {
        const int64_t oh = (int64_t)rs_clamp(t.idx_h[hb + j], q.OH) * q.OW;
        const float a = t.w_h[hb + j];
        float row[RS_PL][VEC];
#pragma unroll
        for (int k = 0; k < RS_PL; ++k)
#pragma unroll
          for (int e = 0; e < VEC; ++e) row[k][e] = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          for (int i = 0; i < nw[e]; ++i) {
            const int ow = rs_clamp(t.idx_w[wb[e] + i], q.OW);
            const float b = t.w_w[wb[e] + i];
            float gv[RS_PL];
#pragma unroll
            for (int k = 0; k < RS_PL; ++k) gv[k] = p0 + k < p_end ? gp[k * gplane + oh + ow] : 0.f;
#pragma unroll
            for (int k = 0; k < RS_PL; ++k) row[k][e] += b * gv[k];
          }
#pragma unroll
        for (int k = 0; k < RS_PL; ++k)
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc[k][e] += a * row[k][e];
      }
    }
#pragma unroll
    for (int k = 0; k < RS_PL; ++k)
      if (p0 + k < p_end) st<VEC>(dp + (p0 + k) * dplane, acc[k]);
  }
}

template <int VEC>
__global__ __launch_bounds__(256) void resample_vjp_kernel(const float* __restrict__ g, ResampleGeom q, ResampleTables t, int64_t P,
                                                           int64_t p_per, float* __restrict__ dx) {
  // G == 1: the workgroups of grid.x stride over the lanes of a plane, blockIdx.y is the slice of planes;
  // G > 1: thread = (slice of the workgroup, lane of the plane), one pass
  const int sub = q.G > 1 ? fdiv((int)threadIdx.x, q.lanes_div) : 0;
  if (sub >= q.G) return;  // (the threads that 256 % lanes leaves over)
  const int64_t p_begin = ((int64_t)blockIdx.y * q.G + sub) * p_per, p_end = min(P, p_begin + p_per);
  if (p_begin >= P) return;
  const int64_t l0 = q.G > 1 ? (int64_t)threadIdx.x - (int64_t)sub * q.lanes : (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t step = q.G > 1 ? q.lanes : (int64_t)gridDim.x * 256;
  for (int64_t l = l0; l < q.lanes; l += step) {
    int h, wv;
    if (!q.big) {
      h = fdiv((int)l, q.wv_div), wv = (int)l - h * q.WV;
    } else {
      const int64_t hh = l / q.WV;
      h = (int)hh, wv = (int)(l - hh * q.WV);
    }
    const int w0 = wv * VEC;
    const int hb = t.ptr_h[h], nh = min(max(t.ptr_h[h + 1] - hb, 0), LK_RESAMPLE_MAX_TAPS);
    int wb[VEC], nw[VEC];
    bool reg = nh <= RS_REG;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      wb[e] = t.ptr_w[w0 + e];
      nw[e] = min(max(t.ptr_w[w0 + e + 1] - wb[e], 0), LK_RESAMPLE_MAX_TAPS);
      reg = reg && nw[e] <= RS_REG;
    }
    float* dp = dx + (int64_t)h * q.W + w0;
    if (reg) resample_planes<VEC, true>(g, q, t, hb, nh, wb, nw, p_begin, p_end, dp);
    else resample_planes<VEC, false>(g, q, t, hb, nh, wb, nw, p_begin, p_end, dp);
  }
}

// ---- host: the contract and the path of a shape ----------------------------------------------------------------------------------
struct ResamplePlan {
  int vec, big, G;
  int64_t lanes, blocks, p_per, slices, grid_y;
};

// false: a shape outside the contract of the entry point
static bool resample_shape_ok(int64_t P, int64_t OH, int64_t OW, int64_t H, int64_t W) {
  const int64_t lim = 1ll << 30;
  if (P < 1 || OH < 1 || OH >= lim || OW < 1 || OW >= lim || H < 1 || H >= lim || W < 1 || W >= lim) return false;
  const unsigned __int128 go = (unsigned __int128)OH * (unsigned __int128)OW, di = (unsigned __int128)H * (unsigned __int128)W;
  return (unsigned __int128)P * (go > di ? go : di) < ((unsigned __int128)1 << 40);
}

static void resample_plan(int64_t P, int64_t H, int64_t W, bool aligned, ResamplePlan* p) {
  p->vec = aligned && W % 4 == 0;
  p->lanes = H * (W / (p->vec ? 4 : 1));
  p->big = p->lanes >= (1ll << 31);
  p->G = p->lanes <= 128 ? (int)(256 / p->lanes) : 1;
  p->blocks = grid_blocks(p->lanes);
  // planes per slice: all of them unless one plane leaves the device short of waves (256 CUs x 8 waves; a workgroup of 4 waves
  // takes G slices); whole passes of RS_PL planes
  const int64_t want = 2048, waves = p->blocks * 4;
  int64_t slices = waves >= want ? 1 : (want + waves - 1) / waves * p->G;
  if (slices > P) slices = P;
  if (slices > 65535ll * p->G) slices = 65535ll * p->G;
  p->p_per = ((P + slices - 1) / slices + RS_PL - 1) / RS_PL * RS_PL;
  p->slices = (P + p->p_per - 1) / p->p_per;
  p->grid_y = (p->slices + p->G - 1) / p->G;
}

static int resample_check_vjp(const float* g, int64_t P, int64_t OH, int64_t OW, int64_t H, int64_t W, const int* ptr_h,
                              const int* idx_h, const float* w_h, const int* ptr_w, const int* idx_w, const float* w_w,
                              const float* dx, ResamplePlan* p) {
  LK_REQUIRE(g && ptr_h && idx_h && w_h && ptr_w && idx_w && w_w && dx, "lk_resample_vjp_f32: bad arguments (null pointer)");
  LK_REQUIRE(resample_shape_ok(P, OH, OW, H, W),
             "lk_resample_vjp_f32: bad arguments (1 <= P, 1 <= OH, OW, H, W < 2^30, P * max(OH * OW, H * W) < 2^40)");
  const unsigned __int128 gb = (unsigned __int128)P * OH * OW * 4, db = (unsigned __int128)P * H * W * 4;
  // (the tables: the pointer arrays in full, the tap arrays by their first entry - their length lives on the device)
  LK_REQUIRE(disjoint(dx, db, g, gb) && disjoint(dx, db, ptr_h, (unsigned __int128)(H + 1) * 4) &&
                 disjoint(dx, db, ptr_w, (unsigned __int128)(W + 1) * 4) && disjoint(dx, db, idx_h, 4) && disjoint(dx, db, w_h, 4) &&
                 disjoint(dx, db, idx_w, 4) && disjoint(dx, db, w_w, 4),
             "lk_resample_vjp_f32: bad arguments (dx overlaps an operand)");
  resample_plan(P, H, W, ((uintptr_t)dx & 15) == 0, p);
  return LK_OK;
}

}  // namespace lk

using namespace lk;

extern "C" int lk_resample_vjp_f32(const float* g, int64_t P, int64_t OH, int64_t OW, int64_t H, int64_t W, const int* ptr_h,
                                   const int* idx_h, const float* w_h, const int* ptr_w, const int* idx_w, const float* w_w,
                                   float* dx, void* stream) {
  ResamplePlan p;
  const int rc = resample_check_vjp(g, P, OH, OW, H, W, ptr_h, idx_h, w_h, ptr_w, idx_w, w_w, dx, &p);
  if (rc != LK_OK) return rc;
  ResampleGeom q;
  q.H = (int)H, q.W = (int)W, q.OH = (int)OH, q.OW = (int)OW, q.WV = (int)(W / (p.vec ? 4 : 1));
  q.big = p.big, q.G = p.G, q.lanes = p.lanes, q.wv_div = make_fastdiv(q.WV);
  q.lanes_div = make_fastdiv(p.G > 1 ? (int)p.lanes : 1);
  ResampleTables t;
  t.ptr_h = ptr_h, t.idx_h = idx_h, t.w_h = w_h, t.ptr_w = ptr_w, t.idx_w = idx_w, t.w_w = w_w;
  const dim3 grid((unsigned)p.blocks, (unsigned)p.grid_y);
  hipStream_t st = (hipStream_t)stream;
  if (p.vec) hipLaunchKernelGGL((resample_vjp_kernel<4>), grid, dim3(256), 0, st, g, q, t, P, p.p_per, dx);
  else hipLaunchKernelGGL((resample_vjp_kernel<1>), grid, dim3(256), 0, st, g, q, t, P, p.p_per, dx);
  return check_launch("resample_vjp_kernel");
}

// vec | taps-in-registers << 1 | 64-bit lane index << 2 | plane-split << 3 | grid-stride << 4 | packed slices << 5 |
// workgroups of grid.x << 8
extern "C" int lk_resample_variant(int64_t P, int64_t OH, int64_t OW, int64_t H, int64_t W, int taps_h, int taps_w, int aligned) {
  if (!resample_shape_ok(P, OH, OW, H, W) || taps_h < 0 || taps_w < 0 || taps_h > LK_RESAMPLE_MAX_TAPS ||
      taps_w > LK_RESAMPLE_MAX_TAPS)
    return -1;
  ResamplePlan p;
  resample_plan(P, H, W, aligned != 0, &p);
  return p.vec | ((taps_h <= RS_REG && taps_w <= RS_REG) ? 1 : 0) << 1 | p.big << 2 | (p.slices > 1 ? 1 : 0) << 3 |
         (p.blocks * 256 < p.lanes ? 1 : 0) << 4 | (p.G > 1 ? 1 : 0) << 5 | (int)p.blocks << 8;
}
