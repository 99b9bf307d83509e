// Per-sample weight Jacobian of a GROUPED nn.Conv2d (groups > 1: depthwise, depthwise with a channel multiplier, ResNeXt-style
// narrow groups) for all seeds of a reverse sweep:
//   Js[n][c][col0 + o*Dkg + k] = sum_l g[c][n][o][l] * patch[n][l][grp(o)*Cig + ci][dy][dx]      Js[n][c][bcol0 + o] = sum_l g[c][n][o][l]
// Cig = Cin / groups, Dkg = Cig*kh*kw, k = (ci, dy, dx) in the order of weight[o].flatten(), grp(o) = o / (Do / groups).
// Replaces the grouped-convolution columns of the jacrev materialisation of CurvatureInterface.jacobians
// (laplace/curvature/curvature.py:88-129).  With groups = 1 it is the contract of lk_jac_conv_f32 (lk_diag.hip).
//
// Depthwise (Cig = 1, kh*kw <= 49) is the hot shape and has a kernel of its own: the 16 x 16 tile of jac_conv_kernel would hold
// Do/groups x kh*kw live entries (1 x 9 of 256).  The work is a reduction over L bound by the single read of g:
//   bytes that must move = 4 * (Cc*B*Do*L + B*Cin*H*W + B*Cc*Do*Dkg).
// A group of W lanes (a power of two <= 64) owns one row (n, o); a lane owns VEC consecutive output positions per tile, gathers
// their kh*kw input values ONCE (from the row's input plane, which the whole group re-reads through the vector L1) and keeps
// them in registers while it walks the seeds, so the plane is fetched once per pass of SC seeds; g is read once, 16 bytes
// per lane where OW is a multiple of 4 and g is 16-byte aligned.  Every lane holds kh*kw accumulators per seed, reduced over
// the group by a fixed xor-shuffle tree; the group then stores the row's kh*kw values as one contiguous run.  No atomics, one
// owner per output element, fixed order: two runs give the same bits.
//
// Everything else (Cig > 1, or more than 49 taps) goes through the tile scheme of jac_conv_kernel with the group's channel
// offset; 16-row output tiles do not straddle groups.
#include "lk_stream.h"

namespace lk {

struct GConvGeom {
  int Cin, H, W, OH, OW, kh, kw, sh, sw, ph, pw, dh, dw;
  int Cig, Dog;  // input / output channels per group
};

// Depthwise: g [Cc][rows][L] with rows = B * Do (n, o); x [B][Cin][H][W], row (n, o) reads plane n*Cin + o / Dog.
// KKT >= kh*kw: accumulators per seed; SC: seeds per pass; WL lanes per row; 256 / WL rows per workgroup.
template <int KKT, int SC, int VEC>
__global__ __launch_bounds__(256) void jac_dwconv_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                         int64_t rows, int Cc, int Do, GConvGeom cg, FastDiv div_ow, int WL,
                                                         float* __restrict__ Js, int64_t P, int64_t col0, int64_t bcol0) {
  const int64_t row = (int64_t)blockIdx.x * (256 / WL) + threadIdx.x / WL;
  const int lane = threadIdx.x & (WL - 1);
  const bool live = row < rows;  // (dead groups stay in the shuffles and touch no memory)
  const int KK = cg.kh * cg.kw, L = cg.OH * cg.OW;
  const int64_t n = live ? row / Do : 0;
  const int o = live ? (int)(row - n * Do) : 0;
  const float* xp = x + (n * cg.Cin + o / cg.Dog) * ((int64_t)cg.H * cg.W);
  const float* gr = g + row * L;
  const int64_t seed_stride = rows * L;
  const int tile = WL * VEC;
  for (int s0 = 0; s0 < Cc; s0 += SC) {
    float acc[SC][KKT], bs[SC];
#pragma unroll
    for (int s = 0; s < SC; ++s) {
      bs[s] = 0.f;
#pragma unroll
      for (int k = 0; k < KKT; ++k) acc[s][k] = 0.f;
    }
    for (int l0 = 0; l0 < L; l0 += tile) {
      const int l = l0 + lane * VEC;  // (VEC = 4: OW % 4 == 0, so the four positions share an output row and l + 3 < L)
      const bool on = live && l < L;
      float pv[VEC][KKT];
#pragma unroll
      for (int e = 0; e < VEC; ++e)
#pragma unroll
        for (int k = 0; k < KKT; ++k) pv[e][k] = 0.f;
      if (on) {
        const int oh = fdiv(l, div_ow), ow = l - oh * cg.OW;
        const int ih0 = oh * cg.sh - cg.ph, iw0 = ow * cg.sw - cg.pw;
        int dy = 0, dx = 0;  // (uniform)
#pragma unroll
        for (int k = 0; k < KKT; ++k) {
          if (k < KK) {
            const int ih = ih0 + dy * cg.dh;
            if (ih >= 0 && ih < cg.H) {
#pragma unroll
              for (int e = 0; e < VEC; ++e) {
                const int iw = iw0 + e * cg.sw + dx * cg.dw;
                if (iw >= 0 && iw < cg.W) pv[e][k] = xp[ih * cg.W + iw];
              }
            }
            if (++dx == cg.kw) {
              dx = 0;
              ++dy;
            }
          }
        }
      }
#pragma unroll
      for (int s = 0; s < SC; ++s) {
        if (s0 + s < Cc) {  // (wave-uniform)
          float gv[VEC];
#pragma unroll
          for (int e = 0; e < VEC; ++e) gv[e] = 0.f;
          if (on) ld<VEC>(gr + (int64_t)(s0 + s) * seed_stride + l, gv);
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            bs[s] += gv[e];
#pragma unroll
            for (int k = 0; k < KKT; ++k)
              if (k < KK) acc[s][k] += gv[e] * pv[e][k];
          }
        }
      }
    }
#pragma unroll
    for (int s = 0; s < SC; ++s) {
      if (s0 + s < Cc) {
        for (int off = WL >> 1; off > 0; off >>= 1) {
          bs[s] += __shfl_xor(bs[s], off, 64);
#pragma unroll
          for (int k = 0; k < KKT; ++k)
            if (k < KK) acc[s][k] += __shfl_xor(acc[s][k], off, 64);
        }
        // every lane of the group holds the sums: lane j stores element k with k % WL == j, a contiguous run per WL values
        float* out = Js + (n * Cc + (s0 + s)) * P;
        float* ow_ = out + col0 + (int64_t)o * KK;
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < KKT; ++k) {
          if (k < KK) {
            const int j = k & (WL - 1);
            if (lane == j) v = acc[s][k];
            if (j == WL - 1 || k == KK - 1) {
              if (live && lane <= j) ow_[k - j + lane] = v;
            }
          }
        }
        if (bcol0 >= 0 && live && lane == 0) out[bcol0 + o] = bs[s];
      }
    }
  }
}

// Any groups: the 16 x 16 tile scheme of jac_conv_kernel.  grid = (ceil(Dkg / 16), groups * ceil(Dog / 16), B * Cc).
__global__ __launch_bounds__(256) void jac_gconv_tile_kernel(const float* __restrict__ x, const float* __restrict__ g, int B,
                                                             int Cc, int Do, GConvGeom cg, int o_tiles,
                                                             float* __restrict__ Js, int64_t P, int64_t col0,
                                                             int64_t bcol0) {
  __shared__ float sg[16][17];  // [o][l]
  __shared__ float sp[16][17];  // [l][k]
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int n = blockIdx.z / Cc, c = blockIdx.z % Cc;
  const int KK = cg.kh * cg.kw, Dkg = cg.Cig * KK, L = cg.OH * cg.OW;
  const int grp = blockIdx.y / o_tiles, og0 = (blockIdx.y - grp * o_tiles) * 16;
  const int k0 = blockIdx.x * 16;
  const int og = og0 + ty;             // output channel within the group
  const int o = grp * cg.Dog + og;
  const bool o_ok = og < cg.Dog;
  const float* gn = g + ((int64_t)c * B + n) * Do * L;
  const float* xn = x + ((int64_t)n * cg.Cin + (int64_t)grp * cg.Cig) * cg.H * cg.W;
  const int kcol = k0 + tx;
  const int ci = kcol / KK;
  const int dd = kcol - ci * KK;
  const int dy = dd / cg.kw, dx = dd - dy * cg.kw;
  float acc = 0.f, bsum = 0.f;
  for (int l0 = 0; l0 < L; l0 += 16) {
    {
      const int l = l0 + tx;
      sg[ty][tx] = (o_ok && l < L) ? gn[(int64_t)o * L + l] : 0.f;
    }
    {
      const int l = l0 + ty;
      float v = 0.f;
      if (l < L && kcol < Dkg) {
        const int oh = l / cg.OW, ow = l - oh * cg.OW;
        const int ih = oh * cg.sh - cg.ph + dy * cg.dh, iw = ow * cg.sw - cg.pw + dx * cg.dw;
        if (ih >= 0 && ih < cg.H && iw >= 0 && iw < cg.W) v = xn[((int64_t)ci * cg.H + ih) * cg.W + iw];
      }
      sp[ty][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int l = 0; l < 16; ++l) {
      acc += sg[ty][l] * sp[l][tx];
      bsum += sg[ty][l];
    }
    __syncthreads();
  }
  float* out = Js + ((int64_t)n * Cc + c) * P;
  if (o_ok && kcol < Dkg) out[col0 + (int64_t)o * Dkg + kcol] = acc;
  if (bcol0 >= 0 && blockIdx.x == 0 && tx == 0 && o_ok) out[bcol0 + o] = bsum;
}

constexpr int GCONV_DW_MAX_TAPS = 49;  // the depthwise kernel's accumulators per seed (7 x 7)

struct GConvPlan {
  GConvGeom cg;
  bool depthwise, vec;
  int WL;          // lanes per row of the depthwise kernel
  int64_t blocks;  // its grid.x
  int o_tiles;     // 16-row output tiles per group of the tile kernel
};

// Every argument check of lk_jac_gconv_f32, before the first HIP call; fills the launch plan.
static int gconv_check_arguments(const float* x_nchw, const float* g, int64_t B, int64_t Cc, int64_t Cin, int64_t H,
                                 int64_t W, int64_t Do, int64_t groups, int kh, int kw, int sh, int sw, int ph, int pw,
                                 int dh, int dw, const float* Js, int64_t P, int64_t col0, int64_t bcol0,
                                 GConvPlan* plan) {
  LK_REQUIRE(x_nchw && g && Js && B >= 0 && Cc >= 1 && Cin >= 1 && Do >= 1 && groups >= 1,
             "lk_jac_gconv_f32: bad arguments");
  LK_REQUIRE(Cin % groups == 0 && Do % groups == 0, "lk_jac_gconv_f32: groups must divide Cin and Do");
  // the geometry travels as int; ih = oh*sh - ph + dy*dh and ih*W + iw are formed in int
  LK_REQUIRE(kh >= 1 && kw >= 1 && sh >= 1 && sw >= 1 && dh >= 1 && dw >= 1 && ph >= 0 && pw >= 0 && H >= 1 && W >= 1 &&
                 H < (1 << 15) && W < (1 << 15) && kh < (1 << 15) && kw < (1 << 15) && sh < (1 << 15) && sw < (1 << 15) &&
                 ph < (1 << 15) && pw < (1 << 15) && dh < (1 << 15) && dw < (1 << 15),
             "lk_jac_gconv_f32: bad geometry (kernel, stride, dilation >= 1; every extent < 32768)");
  const int64_t OH = (H + 2 * (int64_t)ph - (int64_t)dh * (kh - 1) - 1) / sh + 1;
  const int64_t OW = (W + 2 * (int64_t)pw - (int64_t)dw * (kw - 1) - 1) / sw + 1;
  LK_REQUIRE(H + 2 * (int64_t)ph >= (int64_t)dh * (kh - 1) + 1 && W + 2 * (int64_t)pw >= (int64_t)dw * (kw - 1) + 1,
             "lk_jac_gconv_f32: empty output");
  const int64_t Cig = Cin / groups, Dog = Do / groups, KK = (int64_t)kh * kw, Dkg = Cig * KK;
  LK_REQUIRE(B < (1ll << 31) && Cc < (1ll << 31) && Cin < (1ll << 31) && Do < (1ll << 31) && Dkg < (1ll << 31) - 16,
             "lk_jac_gconv_f32: extent too large (B, Cc, Cin, Do, Cig*kh*kw < 2^31)");
  LK_REQUIRE(col0 >= 0 && col0 + Do * Dkg <= P && (bcol0 < 0 || bcol0 + Do <= P),
             "lk_jac_gconv_f32: column range outside Js");
  LK_REQUIRE(bcol0 < 0 || bcol0 + Do <= col0 || col0 + Do * Dkg <= bcol0,
             "lk_jac_gconv_f32: weight and bias columns overlap");
  GConvGeom& cg = plan->cg;
  cg.Cin = (int)Cin; cg.H = (int)H; cg.W = (int)W; cg.OH = (int)OH; cg.OW = (int)OW; cg.kh = kh; cg.kw = kw;
  cg.sh = sh; cg.sw = sw; cg.ph = ph; cg.pw = pw; cg.dh = dh; cg.dw = dw; cg.Cig = (int)Cig; cg.Dog = (int)Dog;
  plan->depthwise = Cig == 1 && KK <= GCONV_DW_MAX_TAPS;
  if (plan->depthwise) {
    const int64_t L = OH * OW;
    plan->vec = OW % 4 == 0 && ((uintptr_t)g & 15) == 0;
    const int64_t units = plan->vec ? L / 4 : L;
    int wl = 1;
    while (wl < units && wl < 64) wl <<= 1;
    plan->WL = wl;
    const int64_t per_block = 256 / wl;  // rows (n, o) per workgroup; B*Do < 2^62
    plan->blocks = (B * Do + per_block - 1) / per_block;
    LK_REQUIRE(plan->blocks < (1ll << 31), "lk_jac_gconv_f32: too many rows for one launch (B*Do*lanes < 2^39)");
  } else {
    LK_REQUIRE(B * Cc <= 65535, "lk_jac_gconv_f32: B*C too large for grid.z (chunk the batch)");
    const int64_t o_tiles = (Dog + 15) / 16;
    LK_REQUIRE(groups * o_tiles <= 65535, "lk_jac_gconv_f32: too many output tiles for grid.y (groups * ceil(Do/groups/16) <= 65535)");
    plan->o_tiles = (int)o_tiles;
  }
  return LK_OK;
}

template <int KKT, int SC>
static void gconv_run_depthwise(const GConvPlan& p, const float* x, const float* g, int64_t rows, int Cc, int Do, float* Js,
                                int64_t P, int64_t col0, int64_t bcol0, hipStream_t st) {
  const FastDiv d = make_fastdiv(p.cg.OW);
  const dim3 grid((unsigned)p.blocks);
  if constexpr (KKT <= 9) {
    if (p.vec) {
      hipLaunchKernelGGL((jac_dwconv_kernel<KKT, SC, 4>), grid, dim3(256), 0, st, x, g, rows, Cc, Do, p.cg, d, p.WL, Js, P,
                         col0, bcol0);
      return;
    }
  }
  hipLaunchKernelGGL((jac_dwconv_kernel<KKT, SC, 1>), grid, dim3(256), 0, st, x, g, rows, Cc, Do, p.cg, d, p.WL, Js, P, col0,
                     bcol0);
}

}  // namespace lk

using namespace lk;

extern "C" int lk_jac_gconv_f32(const float* x_nchw, const float* g, int64_t B, int64_t Cc, int64_t Cin, int64_t H,
                                int64_t W, int64_t Do, int64_t groups, int kh, int kw, int sh, int sw, int ph, int pw,
                                int dh, int dw, float* Js, int64_t P, int64_t col0, int64_t bcol0, void* stream) {
  GConvPlan plan;
  const int rc = gconv_check_arguments(x_nchw, g, B, Cc, Cin, H, W, Do, groups, kh, kw, sh, sw, ph, pw, dh, dw, Js, P, col0,
                                       bcol0, &plan);
  if (rc != LK_OK) return rc;
  if (B == 0) return LK_OK;
  hipStream_t st = (hipStream_t)stream;
  if (plan.depthwise) {
    const int KK = kh * kw;
    const int64_t rows = B * Do;
    if (KK <= 9)
      gconv_run_depthwise<9, 10>(plan, x_nchw, g, rows, (int)Cc, (int)Do, Js, P, col0, bcol0, st);
    else if (KK <= 25)
      gconv_run_depthwise<25, 4>(plan, x_nchw, g, rows, (int)Cc, (int)Do, Js, P, col0, bcol0, st);
    else
      gconv_run_depthwise<49, 2>(plan, x_nchw, g, rows, (int)Cc, (int)Do, Js, P, col0, bcol0, st);
    return check_launch("jac_dwconv_kernel");
  }
  const int64_t Dkg = (int64_t)plan.cg.Cig * kh * kw;
  dim3 grid((unsigned)((Dkg + 15) / 16), (unsigned)(groups * plan.o_tiles), (unsigned)(B * Cc));
  hipLaunchKernelGGL(jac_gconv_tile_kernel, grid, dim3(256), 0, st, x_nchw, g, (int)B, (int)Cc, (int)Do, plan.cg,
                     plan.o_tiles, Js, P, col0, bcol0);
  return check_launch("jac_gconv_tile_kernel");
}
