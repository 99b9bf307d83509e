// The two reductions of KFAC-reduce (the weight-sharing Kronecker approximation that sums a layer's output gradients and averages
// its inputs over the shared positions BEFORE the outer products): the rows the Gram engine then sees have depth B or S B
// instead of B L.  They replace, in the fit with kfac_approx="reduce" (laplace/curvature/curvlinops.py:95-98 hands the argument
// to curvlinops' KFAC), the torch sequences  g.float().sum((1, 2)),  g.reshape(S * B, Do, L).sum(2),  a.reshape(B, L, Di).mean(1)
// and  F.unfold(a, ...).mean(2)  - the last of which writes and reads a [B, Ci kh kw, L] patch matrix to keep Ci kh kw numbers a
// sample.
//
// ---- position sum  y[r][d] = alpha * sum_l x[r][l][d]  (layout 0, D contiguous)  or  alpha * sum_l x[r][d][l]  (layout 1) ------
// x is an fp32 tensor or the two fp16 planes of a ONE-scale split tensor read as they lie, value = (float(h) + float(l)) * 2^-sexp
// (sexp read from its device word: the power of two is applied once, to the sum, together with alpha).
//   * layout 0: a workgroup of 256 threads is CL lanes across the channel vectors of a position (a power of two <= 64) times
//     PG = 256 / CL position groups and owns one (row, tile of CL channel vectors).  A thread adds positions pg, pg + PG, ... in
//     ascending order, the PG partial sums meet in a fixed tree over LDS, group 0 stores.  Many rows of modest length fill the
//     device with CL as wide as the row; FEW rows (a sequence batch) narrow CL - more tiles, more position groups a tile - until
//     there are POSSUM_UNITS units or a lane group would read less than 128 contiguous bytes.
//   * layout 1: LR lanes (a power of two <= 256) own a row of L contiguous elements, 256 / LR rows a workgroup; lane-strided
//     partial sums, the same LDS tree.  One wave a row at most while the rows fill the device, the whole workgroup otherwise.
// 16-byte fp32 loads (8-byte ones of four halves) where the contiguous extent is a multiple of 4 and the bases are aligned,
// 4-byte (2-byte) ones otherwise.  Minimal traffic: x once plus 4 R D bytes.
//
// ---- patch mean  out[b][col(kh, kw, ci)] = 1/L sum_{oh, ow} x[b][ci][oh sh + kh dh - ph][ow sw + kw dw - pw] ---------------------
// The sum over the output positions is separable: a tap (kh, kw) sees the rows {oh sh + kh dh - ph} x the columns {ow sw + kw dw
// - pw} of the map, so the sum over the column set can be formed once per (row, kw) and shared by every kh (or the other way
// round).  A workgroup owns (sample, block of CB channels) and keeps the one-axis sums T of its block in LDS:
//   * channels-last memory [B][H][W][C]: a thread owns (row r, channel vector) - lanes across the channels - walks w upwards, loads
//     each element ONCE and adds it to T[r][kw][c] of every kw whose column set holds w (its own LDS cells: no race); then a
//     thread per output sums T over the row set of its kh.
//   * NCHW memory [B][C][H][W]: the roles of the axes swap so that the lanes still run along memory: a thread owns (channel, vector
//     of w), walks r upwards and adds to T[c][kh][w]; then a thread per output sums T over the column set of its kw.
// Both are one kernel: a `lane' axis (contiguous), an `own' axis and a `walk' axis with the tap geometry of the walk axis in
// stage 1 and of the lane / own axis in stage 2.  Every x element is read from HBM once, every output has one owner, the orders
// are fixed (walk index ascending, then set index ascending): repeated runs give the same bits.  Out-of-image taps add nothing.
// Minimal traffic: 4 B H W C + 4 B kh kw C bytes.  CB is the largest block whose T fits half the 160 KiB of LDS (two workgroups a
// CU), else all of it; it is halved while that leaves the device short of workgroups and every thread still owns a walk.
#include "lk_stream.h"

namespace lk {

constexpr int64_t POSSUM_UNITS = 1024;       // workgroups that fill the device (256 CUs x 4)
constexpr int PM_LDS_MAX = 160 * 1024;       // LDS of a CU
constexpr int PM_MAX_K = 16;                 // widest kernel side
constexpr int64_t PM_UNITS = 512;            // workgroups the patch mean wants before it stops halving its channel block

struct PsSrc {  // the source: f32 non-null, or the planes with their scale word
  const float* f32;
  const _Float16* h;
  const _Float16* l;
  const int* sexp;
};

template <int VEC, bool SPLIT>
__device__ __forceinline__ void ps_ld(const PsSrc& X, int64_t at, float (&v)[VEC]) {
  if constexpr (!SPLIT) {
    ld<VEC>(X.f32 + at, v);
  } else {
    ld_split<VEC>(X.h + at, X.l + at, v);
  }
}

// the partial sums red[e * 256 + t] of the `groups` thread groups `step` threads apart: a fixed tree, the result in group 0
template <int VEC>
__device__ __forceinline__ void ps_tree(float* red, int group, int groups, int step) {
  __syncthreads();
  for (int half = groups >> 1; half > 0; half >>= 1) {
    if (group < half) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) red[e * 256 + threadIdx.x] += red[e * 256 + threadIdx.x + half * step];
    }
    __syncthreads();
  }
}

// ---- layout 0: [R][L][D] -------------------------------------------------------------------------------------------------------------
// `nvc`: channel vectors of a position; `tiles`: tiles of CL of them; `units` = R * tiles
template <int VEC, bool SPLIT>
__global__ __launch_bounds__(256) void possum_cols_kernel(PsSrc X, int L, int64_t D, int CL, int nvc, int tiles, int64_t units,
                                                          float alpha, float* __restrict__ y) {
  __shared__ float red[256 * VEC];
  const int PG = 256 / CL;
  const int cl = threadIdx.x & (CL - 1), pg = threadIdx.x / CL;
  const float scale = SPLIT ? alpha * ldexpf(1.f, -X.sexp[0]) : alpha;
  // (every trip count below is uniform over the workgroup: dead lanes stay in the barriers and touch no memory)
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t r = u / tiles;
    const int cvi = (int)(u - r * tiles) * CL + cl;
    const bool live = cvi < nvc;
    const int np = live ? L : 0;
    const int64_t base = r * L * D + (int64_t)cvi * VEC;
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
#pragma unroll 4
    for (int p = pg; p < np; p += PG) {  // (L < 2^30 and PG <= 256: no overflow)
      float v[VEC];
      ps_ld<VEC, SPLIT>(X, base + (int64_t)p * D, v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] += v[e];
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) red[e * 256 + threadIdx.x] = acc[e];
    ps_tree<VEC>(red, pg, PG, CL);
    if (pg == 0 && live) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] = red[e * 256 + threadIdx.x] * scale;
      st<VEC>(y + r * D + (int64_t)cvi * VEC, acc);
    }
    __syncthreads();  // (red is written again by the next unit)
  }
}

// ---- layout 1: `rows` = R * D rows of L contiguous elements --------------------------------------------------------------------------
// `nv`: vectors of a row; `units`: groups of 256 / LR rows
template <int VEC, bool SPLIT>
__global__ __launch_bounds__(256) void possum_rows_kernel(PsSrc X, int64_t rows, int L, int LR, int nv, int64_t units, float alpha,
                                                          float* __restrict__ y) {
  __shared__ float red[256];
  const int RPB = 256 / LR;
  const int lr = threadIdx.x & (LR - 1), rg = threadIdx.x / LR;
  const float scale = SPLIT ? alpha * ldexpf(1.f, -X.sexp[0]) : alpha;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t row = u * RPB + rg;
    const bool live = row < rows;
    const int n = live ? nv : 0;
    const int64_t base = row * L;
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
#pragma unroll 4
    for (int i = lr; i < n; i += LR) {
      float v[VEC];
      ps_ld<VEC, SPLIT>(X, base + (int64_t)i * VEC, v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] += v[e];
    }
    float s = acc[0];
#pragma unroll
    for (int e = 1; e < VEC; ++e) s += acc[e];
    red[threadIdx.x] = s;
    ps_tree<1>(red, lr, LR, 1);
    if (lr == 0 && live) y[row] = red[threadIdx.x] * scale;
    __syncthreads();
  }
}

// ---- patch mean ------------------------------------------------------------------------------------------------------------------------
struct PmAxis {  // one spatial axis of the convolution: out index o and tap t meet the input at o * s + t * d - p
  int n, k, s, d, p, o;  // input extent, kernel side, stride, dilation, padding, output extent
  FastDiv s_div;
};

struct PmGeom {
  int64_t C;
  int CB, nblk;             // channels of a block, blocks of a sample
  int lanes;                // threads along the lane axis (vectors of the contiguous extent a workgroup covers)
  int owners;               // extent of the own axis inside a workgroup (rows r / channels of the block)
  int64_t lane_stride_own;  // elements between two owners, and between two steps of the walk
  int64_t stride_walk;
  int64_t sample, blk;      // elements of a sample; elements between two channel blocks
  int q;                    // floats of T along the lane axis (CB / W)
  PmAxis walk, set;         // the axis stage 1 reduces, the axis stage 2 reduces
  int channels_last, unfold_order;
  float inv_l;
};

// T[(own * walk.k + t) * q + lane element]
template <int VEC>
__global__ __launch_bounds__(256) void patch_mean_kernel(const float* __restrict__ x, PmGeom g, float* __restrict__ out) {
  extern __shared__ float T[];
  const int64_t b = blockIdx.x / g.nblk;
  const int blk = (int)(blockIdx.x - b * g.nblk);
  const int c0 = blk * g.CB;
  const int cb = g.C - c0 < g.CB ? (int)(g.C - c0) : g.CB;  // channels of this block
  const float* xb = x + b * g.sample + (int64_t)blk * g.blk;
  // the live extents: channels-last (own = rows, lanes = the block's channels), NCHW (own = the block's channels, lanes = w)
  const int n_own = g.channels_last ? g.owners : cb;
  const int n_lane = (g.channels_last ? cb : g.q) / VEC;
  // ---- stage 1: every element once; T of the owner's cells --------------------------------------------------------------------
  const int KT = g.walk.k;
  for (int i = threadIdx.x; i < n_own * n_lane; i += 256) {
    const int own = i / n_lane, lane = i - own * n_lane;
    float* t0 = T + (int64_t)own * KT * g.q + lane * VEC;
    for (int t = 0; t < KT; ++t) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) t0[t * g.q + e] = 0.f;
    }
    const float* xp = xb + own * g.lane_stride_own + lane * VEC;
#pragma unroll 4
    for (int m = 0; m < g.walk.n; ++m) {
      float v[VEC];
      ld<VEC>(xp + m * g.stride_walk, v);
      for (int t = 0; t < KT; ++t) {
        const int a = m + g.walk.p - t * g.walk.d;
        if (a < 0) break;  // (a falls with t)
        const int o = g.walk.s == 1 ? a : fdiv(a, g.walk.s_div);
        if (o < g.walk.o && o * g.walk.s == a) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) t0[t * g.q + e] += v[e];
        }
      }
    }
  }
  __syncthreads();
  // ---- stage 2: a thread per output (tap of the set axis, tap of the walk axis, channel) -----------------------------------------
  const int KS = g.set.k;
  const int KK = KS * KT;
  for (int i = threadIdx.x; i < KK * cb; i += 256) {
    int ts, tw, c;
    if (g.channels_last) {  // channel fastest: neighbours read neighbouring LDS words
      const int tap = i / cb;
      c = i - tap * cb, ts = tap / KT, tw = tap - ts * KT;
    } else {
      c = i / KK;
      const int tap = i - c * KK;
      tw = tap / KS, ts = tap - tw * KS;
    }
    float acc = 0.f;
    for (int o = 0; o < g.set.o; ++o) {
      const int a = o * g.set.s + ts * g.set.d - g.set.p;
      if (a >= 0 && a < g.set.n) acc += g.channels_last ? T[((int64_t)a * KT + tw) * g.q + c] : T[((int64_t)c * KT + tw) * g.q + a];
    }
    // channels-last: set = rows (kh = ts), walk = columns (kw = tw); NCHW: set = columns (kw = ts), walk = rows (kh = tw)
    const int kh = g.channels_last ? ts : tw, kw = g.channels_last ? tw : ts;
    const int nkw = g.channels_last ? KT : KS;
    const int64_t col = g.unfold_order ? ((int64_t)(c0 + c) * KK + kh * nkw + kw) : ((int64_t)(kh * nkw + kw) * g.C + c0 + c);
    out[b * KK * g.C + col] = acc * g.inv_l;
  }
}

// ---- host: the contracts and the path of a shape ---------------------------------------------------------------------------------------
struct PsPlan {
  int vec;         // 16-byte fp32 accesses, 8-byte ones of the planes
  int lanes;       // layout 0: CL lanes across the channel vectors; layout 1: LR lanes of a row
  int nv, tiles;   // vectors of the contiguous extent; layout 0: tiles of CL of them
  int64_t units, blocks;
};

static int possum_check_shape(const char* fn, int64_t R, int64_t L, int64_t D, int layout, bool aligned, PsPlan* p) {
  LK_REQUIRE(layout == 0 || layout == 1, "%s: bad arguments (layout is 0, [R][L][D], or 1, [R][D][L])", fn);
  LK_REQUIRE(R >= 0 && L >= 1 && L < (1ll << 30) && D >= 1 && D < (1ll << 30),
             "%s: bad arguments (0 <= R, 1 <= L < 2^30, 1 <= D < 2^30)", fn);
  LK_REQUIRE((unsigned __int128)R * (unsigned __int128)L * (unsigned __int128)D < ((unsigned __int128)1 << 40),
             "%s: bad arguments (R * L * D < 2^40)", fn);
  const int64_t inner = layout == 0 ? D : L;
  p->vec = aligned && inner % 4 == 0;
  p->nv = (int)(p->vec ? inner / 4 : inner);
  if (layout == 0) {
    int CL = pow2_ceil(p->nv, 64);
    const int floor_cl = p->vec ? 8 : 32;  // a lane group reads at least 128 contiguous bytes
    while (CL > floor_cl && R * ((p->nv + CL - 1) / CL) < POSSUM_UNITS && 256 / CL < L) CL >>= 1;
    p->lanes = CL;
    p->tiles = (p->nv + CL - 1) / CL;
    p->units = R * p->tiles;
  } else {
    const int64_t rows = R * D;
    int LR = pow2_ceil(p->nv, 64);
    while (LR < 256 && LR < p->nv && (rows + 256 / LR - 1) / (256 / LR) < POSSUM_UNITS) LR <<= 1;
    p->lanes = LR;
    p->tiles = 1;
    p->units = (rows + 256 / LR - 1) / (256 / LR);
  }
  p->blocks = p->units < STREAM_MAX_BLOCKS ? p->units : STREAM_MAX_BLOCKS;
  return LK_OK;
}

static int possum_check_f32(const float* x, int64_t R, int64_t L, int64_t D, int layout, const float* y, PsPlan* p) {
  LK_REQUIRE(x && y, "lk_possum_f32: bad arguments (null pointer)");
  LK_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 3) == 0, "lk_possum_f32: bad arguments (x and y are 4-byte aligned)");
  const int rc = possum_check_shape("lk_possum_f32", R, L, D, layout, (((uintptr_t)x | (uintptr_t)y) & 15) == 0, p);
  if (rc != LK_OK) return rc;
  LK_REQUIRE(disjoint(y, (unsigned __int128)R * D * 4, x, (unsigned __int128)R * L * D * 4), "lk_possum_f32: bad arguments (y overlaps x)");
  return LK_OK;
}

static int possum_check_f16x2(const void* x_h, const void* x_l, const int* sexp, int64_t R, int64_t L, int64_t D, int layout,
                              const float* y, PsPlan* p) {
  LK_REQUIRE(x_h && x_l && sexp && y, "lk_possum_f16x2: bad arguments (null pointer)");
  LK_REQUIRE((((uintptr_t)x_h | (uintptr_t)x_l) & 1) == 0 && (((uintptr_t)sexp | (uintptr_t)y) & 3) == 0,
             "lk_possum_f16x2: bad arguments (the planes are 2-byte, sexp and y 4-byte aligned)");
  const bool aligned = (((uintptr_t)x_h | (uintptr_t)x_l) & 7) == 0 && ((uintptr_t)y & 15) == 0;
  const int rc = possum_check_shape("lk_possum_f16x2", R, L, D, layout, aligned, p);
  if (rc != LK_OK) return rc;
  const unsigned __int128 xb = (unsigned __int128)R * L * D * 2, yb = (unsigned __int128)R * D * 4;
  LK_REQUIRE(disjoint(y, yb, x_h, xb) && disjoint(y, yb, x_l, xb) && disjoint(y, yb, sexp, 4),
             "lk_possum_f16x2: bad arguments (y overlaps a plane or the scale word)");
  return LK_OK;
}

template <bool SPLIT>
static int launch_possum(const PsSrc& X, int64_t R, int64_t L, int64_t D, int layout, float alpha, float* y, const PsPlan& p,
                         hipStream_t st) {
  const dim3 grid((unsigned)p.blocks);
  if (layout == 0) {
    if (p.vec)
      hipLaunchKernelGGL((possum_cols_kernel<4, SPLIT>), grid, dim3(256), 0, st, X, (int)L, D, p.lanes, p.nv, p.tiles, p.units, alpha, y);
    else
      hipLaunchKernelGGL((possum_cols_kernel<1, SPLIT>), grid, dim3(256), 0, st, X, (int)L, D, p.lanes, p.nv, p.tiles, p.units, alpha, y);
    return check_launch("possum_cols_kernel");
  }
  if (p.vec)
    hipLaunchKernelGGL((possum_rows_kernel<4, SPLIT>), grid, dim3(256), 0, st, X, R * D, (int)L, p.lanes, p.nv, p.units, alpha, y);
  else
    hipLaunchKernelGGL((possum_rows_kernel<1, SPLIT>), grid, dim3(256), 0, st, X, R * D, (int)L, p.lanes, p.nv, p.units, alpha, y);
  return check_launch("possum_rows_kernel");
}

static int patch_mean_check_shape(const char* fn, int64_t B, int64_t C, int64_t H, int64_t W, int channels_last, int kh, int kw,
                                  int sh, int sw, int ph, int pw, int dh, int dw, int unfold_order, bool al16, PmGeom* g, int* vec,
                                  size_t* lds) {
  LK_REQUIRE((channels_last == 0 || channels_last == 1) && (unfold_order == 0 || unfold_order == 1),
             "%s: bad arguments (channels_last and unfold_order are 0 or 1)", fn);
  LK_REQUIRE(B >= 0 && C >= 1 && C < (1 << 20) && H >= 1 && H < (1 << 20) && W >= 1 && W < (1 << 20),
             "%s: bad arguments (0 <= B, 1 <= C, H, W < 2^20)", fn);
  LK_REQUIRE((unsigned __int128)B * (unsigned __int128)C * (unsigned __int128)H * (unsigned __int128)W < ((unsigned __int128)1 << 40),
             "%s: bad arguments (B * C * H * W < 2^40)", fn);
  LK_REQUIRE(kh >= 1 && kh <= PM_MAX_K && kw >= 1 && kw <= PM_MAX_K, "%s: bad arguments (1 <= kh, kw <= 16)", fn);
  LK_REQUIRE(sh >= 1 && sw >= 1 && dh >= 1 && dw >= 1 && ph >= 0 && pw >= 0 && sh < 65536 && sw < 65536 && dh < 65536 && dw < 65536 &&
                 ph < 65536 && pw < 65536,
             "%s: bad arguments (1 <= stride, dilation < 65536, 0 <= padding < 65536)", fn);
  const int64_t eh = H + 2 * ph - (int64_t)dh * (kh - 1) - 1, ew = W + 2 * pw - (int64_t)dw * (kw - 1) - 1;
  LK_REQUIRE(eh >= 0 && ew >= 0, "%s: bad arguments (the dilated kernel is larger than the padded map)", fn);
  const int OH = (int)(eh / sh) + 1, OW = (int)(ew / sw) + 1;
  const PmAxis rows = {(int)H, kh, sh, dh, ph, OH, make_fastdiv(sh)}, cols = {(int)W, kw, sw, dw, pw, OW, make_fastdiv(sw)};
  g->C = C, g->channels_last = channels_last, g->unfold_order = unfold_order;
  g->inv_l = 1.f / ((float)OH * (float)OW);
  g->sample = C * H * W;
  // floats of T per channel of a block, and the widest block that fits
  const int64_t per_c = channels_last ? H * kw : (int64_t)kh * W;
  int64_t cap = PM_LDS_MAX / 4 / per_c;
  if (cap > (PM_LDS_MAX / 8) / per_c && (PM_LDS_MAX / 8) / per_c >= (C < 16 ? C : 16)) cap = (PM_LDS_MAX / 8) / per_c;  // two a CU
  if (channels_last) {
    *vec = al16 && C % 4 == 0;
    const int V = *vec ? 4 : 1;
    LK_REQUIRE(cap >= V, "%s: bad arguments (the column sums of %d channels, H * kw * 4 bytes each, do not fit the LDS)", fn, V);
    int CB = (int)(C < 64 ? C : 64);
    while (CB > cap) CB = (CB / 2 + V - 1) / V * V;
    while (B * ((C + CB - 1) / CB) < PM_UNITS && CB % (2 * V) == 0 && CB / 2 >= 4 * V && H * (CB / 2 / V) >= 256) CB /= 2;
    g->CB = CB, g->q = CB, g->owners = (int)H, g->lanes = CB / V;
    g->lane_stride_own = W * C, g->stride_walk = C, g->blk = CB;
    g->walk = cols, g->set = rows;
  } else {
    *vec = al16 && W % 4 == 0;
    const int V = *vec ? 4 : 1;
    LK_REQUIRE(cap >= 1, "%s: bad arguments (the row sums of a channel, kh * W * 4 bytes, do not fit the LDS)", fn);
    int CB = (int)(C < 64 ? C : 64);
    if (CB > cap) CB = (int)cap;
    while (CB > 1 && B * ((C + CB - 1) / CB) < PM_UNITS && (CB / 2) * (W / V) >= 256) CB = (CB + 1) / 2;
    g->CB = CB, g->q = (int)W, g->owners = CB, g->lanes = (int)(W / V);
    g->lane_stride_own = H * W, g->stride_walk = W, g->blk = (int64_t)CB * H * W;
    g->walk = rows, g->set = cols;
  }
  g->nblk = (int)((C + g->CB - 1) / g->CB);
  LK_REQUIRE(B * g->nblk < (1ll << 31), "%s: bad arguments (B * channel blocks < 2^31)", fn);
  *lds = (size_t)per_c * g->CB * 4;
  return LK_OK;
}

static int patch_mean_check(const float* x, int64_t B, int64_t C, int64_t H, int64_t W, int channels_last, int kh, int kw, int sh,
                            int sw, int ph, int pw, int dh, int dw, int unfold_order, const float* out, PmGeom* g, int* vec,
                            size_t* lds) {
  const char* fn = "lk_patch_mean_f32";
  LK_REQUIRE(x && out, "%s: bad arguments (null pointer)", fn);
  LK_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 3) == 0, "%s: bad arguments (x and out are 4-byte aligned)", fn);
  const int rc = patch_mean_check_shape(fn, B, C, H, W, channels_last, kh, kw, sh, sw, ph, pw, dh, dw, unfold_order,
                                        ((uintptr_t)x & 15) == 0, g, vec, lds);
  if (rc != LK_OK) return rc;
  const unsigned __int128 xe = (unsigned __int128)B * C * H * W, oe = (unsigned __int128)B * C * kh * kw;
  LK_REQUIRE(disjoint(out, oe * 4, x, xe * 4), "%s: bad arguments (out overlaps x)", fn);
  return LK_OK;
}

}  // namespace lk

using namespace lk;

extern "C" int lk_possum_f32(const float* x, int64_t R, int64_t L, int64_t D, int layout, float alpha, float* y, void* stream) {
  PsPlan p;
  const int rc = possum_check_f32(x, R, L, D, layout, y, &p);
  if (rc != LK_OK) return rc;
  if (R == 0) return LK_OK;
  const PsSrc X = {x, nullptr, nullptr, nullptr};
  return launch_possum<false>(X, R, L, D, layout, alpha, y, p, (hipStream_t)stream);
}

extern "C" int lk_possum_f16x2(const void* x_h, const void* x_l, const int* sexp, int64_t R, int64_t L, int64_t D, int layout,
                               float alpha, float* y, void* stream) {
  PsPlan p;
  const int rc = possum_check_f16x2(x_h, x_l, sexp, R, L, D, layout, y, &p);
  if (rc != LK_OK) return rc;
  if (R == 0) return LK_OK;
  const PsSrc X = {nullptr, static_cast<const _Float16*>(x_h), static_cast<const _Float16*>(x_l), sexp};
  return launch_possum<true>(X, R, L, D, layout, alpha, y, p, (hipStream_t)stream);
}

// vec | layout << 1 | log2(lanes) << 2 | workgroups << 8, or a negative value for a shape the entry points refuse
extern "C" int lk_possum_variant(int64_t R, int64_t L, int64_t D, int layout, int aligned) {
  PsPlan p;
  if (possum_check_shape("lk_possum_variant", R, L, D, layout, aligned != 0, &p) != LK_OK) return -1;
  int lg = 0;
  while ((1 << lg) < p.lanes) ++lg;
  return p.vec | layout << 1 | lg << 2 | (int)p.blocks << 8;
}

extern "C" int lk_patch_mean_f32(const float* x, int64_t B, int64_t C, int64_t H, int64_t W, int channels_last, int kh, int kw,
                                 int sh, int sw, int ph, int pw, int dh, int dw, int unfold_order, float* out, void* stream) {
  PmGeom g;
  int vec;
  size_t lds;
  const int rc = patch_mean_check(x, B, C, H, W, channels_last, kh, kw, sh, sw, ph, pw, dh, dw, unfold_order, out, &g, &vec, &lds);
  if (rc != LK_OK) return rc;
  if (B == 0) return LK_OK;
  const void* fn = vec ? reinterpret_cast<const void*>(&patch_mean_kernel<4>) : reinterpret_cast<const void*>(&patch_mean_kernel<1>);
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      set_error("lk_patch_mean_f32: cannot raise dynamic LDS limit: %s", hipGetErrorString(e));
      return LK_ELAUNCH;
    }
  }
  const dim3 grid((unsigned)(B * g.nblk));
  if (vec)
    hipLaunchKernelGGL((patch_mean_kernel<4>), grid, dim3(256), lds, (hipStream_t)stream, x, g, out);
  else
    hipLaunchKernelGGL((patch_mean_kernel<1>), grid, dim3(256), lds, (hipStream_t)stream, x, g, out);
  return check_launch("patch_mean_kernel");
}

// vec | channels of a block << 1 | KiB of LDS (rounded up) << 12, or a negative value for a shape lk_patch_mean_f32 refuses
extern "C" int lk_patch_mean_variant(int64_t B, int64_t C, int64_t H, int64_t W, int channels_last, int kh, int kw, int sh, int sw,
                                     int ph, int pw, int dh, int dw, int aligned) {
  PmGeom g;
  int vec;
  size_t lds;
  if (patch_mean_check_shape("lk_patch_mean_variant", B, C, H, W, channels_last, kh, kw, sh, sw, ph, pw, dh, dw, 0, aligned != 0, &g,
                             &vec, &lds) != LK_OK)
    return -1;
  return vec | g.CB << 1 | (int)((lds + 1023) / 1024) << 12;
}
