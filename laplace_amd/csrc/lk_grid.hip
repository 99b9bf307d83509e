// Validation loss of the GLM predictive at G prior precisions in one pass (the grid search of
// laplace/baselaplace.py:487-561, which re-runs the whole predictive once per grid point).
//
// Under a Kronecker or diagonal posterior the variance of output c at prior precision delta is
//   f_var_delta[n][c] = sum_p R[n][c][p]^2 / (mu_p + delta)
// with R the sample's Jacobian in the posterior's eigenbasis (mu = outer(l1, l2), or h for a diagonal posterior): the
// forward pass, the reverse sweep, the rotations and the tile products R are the same for every grid point, and only the
// weighted reduction depends on delta.  The kernels here form R once and run that reduction G times.  Only the diagonal of
// the output covariance is produced ([G][B][C]) — the probit link needs nothing else — so the outputs are independent and
// any number of them is covered by launches over blocks of outputs.
//
// Weight forms (mode): 0 Kron 1 / (l1_o l2_i + delta);  1 damped Kron 1 / ((l1_o + sqrt delta)(l2_i + sqrt delta));
//                      2 diagonal 1 / (h_oi + delta).
// Every sum runs in a fixed order (no float atomics): two runs give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lk_common.h"
#include "lk_quadtile.h"

namespace lk {

enum { GRID_KRON = 0, GRID_KRON_DAMPED = 1, GRID_DIAG = 2 };

// ---- nn.Linear layers ------------------------------------------------------------------------------------------------
// var[g][n][c] += sum_o u[c][n][o]^2 S_g[n][o] (+ sum_o ub[c][n][o]^2 / (wb_o + delta_g)),  S_g[n][o] = sum_i v[n][i]^2 W_g(o,i)
// One workgroup per GRID_LIN_NB samples, which share every reciprocal; v^2 and the S_g of a chunk of GS grid points in LDS.
constexpr int GRID_LIN_NB = 4;

template <int MODE>
__global__ __launch_bounds__(256) void quadform_linear_grid_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                                   const float* __restrict__ w0, const float* __restrict__ w1,
                                                                   const float* __restrict__ deltas, int G, int GS, int B,
                                                                   int C, int Do, int Di, const float* __restrict__ ub,
                                                                   const float* __restrict__ wb, float* __restrict__ var) {
  constexpr int NB = GRID_LIN_NB;
  extern __shared__ float dyn[];  // [NB][Di] v^2, then [NB][GS][Do] S
  float* v2 = dyn;
  float* S = dyn + NB * Di;
  const int n0 = blockIdx.x * NB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int e = tid; e < NB * Di; e += 256) {
    const int nb = e / Di, i = e - nb * Di;
    const float t = n0 + nb < B ? v[(int64_t)(n0 + nb) * Di + i] : 0.f;
    v2[e] = t * t;
  }
  for (int g0 = 0; g0 < G; g0 += GS) {
    const int gl = G - g0 < GS ? G - g0 : GS;
    __syncthreads();  // v2 staged / the previous chunk's S consumed
    for (int pr = wave; pr < gl * Do; pr += 4) {
      const int gg = pr / Do, o = pr - gg * Do;
      const float d = deltas[g0 + gg];
      const float sd = MODE == GRID_KRON_DAMPED ? sqrtf(d) : 0.f;
      float s[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) s[nb] = 0.f;
      for (int i = lane; i < Di; i += 64) {
        float den;
        if (MODE == GRID_KRON)
          den = w0[o] * w1[i] + d;
        else if (MODE == GRID_KRON_DAMPED)
          den = (w0[o] + sd) * (w1[i] + sd);
        else
          den = w0[(int64_t)o * Di + i] + d;
        const float w = 1.f / den;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) s[nb] += v2[nb * Di + i] * w;
      }
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const float t = wave_sum(s[nb]);
        if (lane == 0) S[((size_t)nb * GS + gg) * Do + o] = t;
      }
    }
    __syncthreads();
    for (int e = tid; e < NB * gl * C; e += 256) {
      const int nb = e / (gl * C), r = e - nb * gl * C, gg = r / C, c = r - gg * C;
      const int n = n0 + nb;
      if (n >= B) continue;
      const float* uc = u + ((int64_t)c * B + n) * Do;
      const float* Sg = S + ((size_t)nb * GS + gg) * Do;
      float acc = 0.f, accb = 0.f;  // (the bias block in its own accumulator, as in quadform_linear_kernel)
      for (int o = 0; o < Do; ++o) acc += uc[o] * uc[o] * Sg[o];
      if (ub != nullptr) {
        const float d = deltas[g0 + gg];
        const float* bc = ub + ((int64_t)c * B + n) * Do;
        for (int o = 0; o < Do; ++o) accb += bc[o] * bc[o] / (wb[o] + d);
      }
      var[((int64_t)(g0 + gg) * B + n) * C + c] += acc + accb;
    }
  }
}

// ---- weight-sharing layers (Conv2d, Linear along a sequence) --------------------------------------------------------
// The tile products of quadform_conv_kernel (lk_quadtile.h), then, per tile, the delta-dependent epilogue: the grid is
// walked in chunks of GC points; for each of this lane's 16 (o, i) positions the GC reciprocals are shared by the CT outputs
// (GC x CT = V <= 64 running sums per lane).  The V sums of the 64 lanes are transposed through LDS (lane r then adds up
// row r, 64 values in a fixed order) into a per-wave accumulator [G][CT] that lives for the whole workgroup.
// grid = B * split workgroups (as quadform_conv_kernel); partial[n][sp][G][CT].
constexpr int GRID_GMAX = 128;  // grid points per launch (the host walks larger grids in pieces)

template <int CT>
struct GridCfg {
  // grid points per epilogue chunk (ten outputs: 160 accumulators leave room for 50 running sums without spilling)
  static constexpr int GC = CT == 10 ? 5 : 64 / CT;
  static constexpr int V = GC * CT;   // running sums per lane
  static constexpr int SCRATCH = 4 * 64 * 65 * 4;  // per wave [64 rows][65] floats (padded: conflict-free row reads)
  static constexpr int ARENA = QcLds<CT>::BYTES > SCRATCH ? QcLds<CT>::BYTES : SCRATCH;
};

template <int CT, int MODE, int ARITH>
__global__ __launch_bounds__(256) void quadform_shared_grid_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                                   const float* __restrict__ w0, const float* __restrict__ w1,
                                                                   const float* __restrict__ deltas, int G, int C, int Do,
                                                                   int Dk, int L, int split, float* __restrict__ partial,
                                                                   int64_t u_sample_stride, unsigned u_class_stride) {
  using Cfg = GridCfg<CT>;
  constexpr int GC = Cfg::GC, V = Cfg::V;
  // the tile product's LDS is idle during the epilogue (qc_tile_gemm* end on a barrier and refill it only in the next
  // tile): the transposition scratch shares it
  __shared__ __attribute__((aligned(16))) char lds[Cfg::ARENA];
  __shared__ float accw[4][GRID_GMAX * CT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5;
  int n = blockIdx.x / split, sp = blockIdx.x % split;
  if (gridDim.x % (8 * split) == 0) {  // the workgroups of one sample on one XCD (as quadform_conv_kernel)
    const int xcd = blockIdx.x % 8, j = blockIdx.x / 8;
    n = xcd + 8 * (j / split), sp = j % split;
  }
  const int nOt = (Do + 31) / 32, nIg = (Dk + 127) / 128, ntiles = nOt * nIg;
  const float* __restrict__ un = u + (size_t)n * u_sample_stride;
  const float* __restrict__ vn = v + (size_t)n * Dk * L;
  float* const sc = reinterpret_cast<float*>(lds) + wave * 64 * 65;
  for (int e = lane; e < G * CT; e += 64) accw[wave][e] = 0.f;  // each wave zeroes (and later updates) its own row

  auto operands = [&](int t) {
    return QcOperands{un, vn, (t % nOt) * 32, (t / nOt) * 128 + wave * 32 + (lane & 31), u_class_stride};
  };
  QcStage<CT> st;
  if (ARITH == 1 && sp < ntiles) qc_fetch_b6<CT>(st, 0, (CT + 1) / 2, 0, 2, operands(sp), 0, C, Do, Dk, L);
  for (int t = sp; t < ntiles; t += split) {
    const QcOperands cur = operands(t);
    const int o0 = cur.o0, icol = cur.icol;
    f32x16 acc[CT];
    if constexpr (ARITH == 1)
      qc_tile_gemm_b6<CT>(cur, operands(t + split), t + split < ntiles, C, Do, Dk, L, lds, acc, st);
    else
      qc_tile_gemm<CT>(cur, C, Do, Dk, L, lds, acc);

    // the delta-independent part of this lane's 16 weights: accumulator element r is row o0 + (r & 3) + 8 (r >> 2) + 4 hi
    float base0[16], base1[16];
    bool ok[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = o0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
      ok[r] = o < Do && icol < Dk;
      const int oc = ok[r] ? o : 0, ic = ok[r] ? icol : 0;
      if (MODE == GRID_DIAG) {
        base0[r] = w0[(unsigned)(oc * Dk + ic)];
        base1[r] = 0.f;
      } else {
        base0[r] = w0[oc];
        base1[r] = w1[ic];
      }
      if (MODE == GRID_KRON) base0[r] *= base1[r];
    }
    for (int g0 = 0; g0 < G; g0 += GC) {
      float dq[GC];
#pragma unroll
      for (int gc = 0; gc < GC; ++gc) {
        const float d = deltas[g0 + gc < G ? g0 + gc : G - 1];
        dq[gc] = MODE == GRID_KRON_DAMPED ? sqrtf(d) : d;
      }
      float part[V];
#pragma unroll
      for (int e = 0; e < V; ++e) part[e] = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float sq[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) sq[c] = acc[c][r] * acc[c][r];
#pragma unroll
        for (int gc = 0; gc < GC; ++gc) {
          const float den = MODE == GRID_KRON_DAMPED ? (base0[r] + dq[gc]) * (base1[r] + dq[gc]) : base0[r] + dq[gc];
          const float w = ok[r] ? __builtin_amdgcn_rcpf(den) : 0.f;
#pragma unroll
          for (int c = 0; c < CT; ++c) part[gc * CT + c] += w * sq[c];
        }
      }
      // transpose through LDS: lane r adds up row r (grid point g0 + r / CT, output r % CT) over the wave's 64 lanes
#pragma unroll
      for (int e = 0; e < V; ++e) sc[e * 65 + lane] = part[e];
      __syncthreads();
      if (lane < V && g0 + lane / CT < G) {
        float s = 0.f;
        for (int j = 0; j < 64; ++j) s += sc[lane * 65 + j];
        accw[wave][(g0 + lane / CT) * CT + lane % CT] += s;
      }
      __syncthreads();
    }
  }
  __syncthreads();
  float* pw = partial + ((size_t)n * split + sp) * G * CT;
  for (int e = tid; e < G * CT; e += 256) pw[e] = (accw[0][e] + accw[1][e]) + (accw[2][e] + accw[3][e]);
}

// var[g0 + g][n][c0 + c] += sum over the workgroups of sample n, in fixed order
__global__ __launch_bounds__(256) void quadform_shared_grid_reduce_kernel(const float* __restrict__ partial, int64_t B,
                                                                          int G, int CT, int Cl, int split, int64_t g0,
                                                                          int64_t Ctot, int64_t c0, float* __restrict__ var) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= B * G * Cl) return;
  const int64_t n = e / (G * Cl);
  const int r = (int)(e - n * G * Cl), g = r / Cl, c = r - g * Cl;
  float s = 0.f;
  for (int sp = 0; sp < split; ++sp) s += partial[(((size_t)n * split + sp) * G + g) * CT + c];
  var[((g0 + g) * B + n) * Ctot + c0 + c] += s;
}

// ---- probit link + NLL ------------------------------------------------------------------------------------------------
// loss_sum[g] += sum_n -log(max(softmax(kappa f_mu[n])[y_n], 1e-30)),  kappa = 1 / sqrt(1 + pi/8 var[g][n][c]).
// One workgroup per grid point; per-sample terms in fp32 (as the loop's softmax), the sum in fp64, fixed order.
__global__ __launch_bounds__(256) void probit_nll_grid_kernel(const float* __restrict__ f_mu, const float* __restrict__ var,
                                                              const int64_t* __restrict__ y, int B, int C,
                                                              double* __restrict__ loss_sum) {
  __shared__ double red[256];
  const int g = blockIdx.x, tid = threadIdx.x;
  const float* vg = var + (int64_t)g * B * C;
  double acc = 0.0;
  for (int n = tid; n < B; n += 256) {
    const float* f = f_mu + (int64_t)n * C;
    const float* vn = vg + (int64_t)n * C;
    // one pass (running max, rescaled sum): every kappa_c f_c is formed once, so the label's term is the same value as
    // the one in the sum (C = 1 gives p = 1 exactly, as the loop's softmax does)
    float m = -INFINITY, s = 0.f, zy = 0.f;
    const int64_t yn = y[n];
    for (int c = 0; c < C; ++c) {
      const float z = 1.f / sqrtf(1.f + 0.39269908169872414f * vn[c]) * f[c];  // kappa * f_mu, as the loop
      if (z > m) {
        s = s * expf(m - z) + 1.f;
        m = z;
      } else {
        s += expf(z - m);
      }
      if (c == yn) zy = z;
    }
    const float p = expf(zy - m) / s;
    acc += (double)(-logf(fmaxf(p, 1e-30f)));
  }
  red[tid] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) loss_sum[g] += red[0];
}

}  // namespace lk

using namespace lk;

// (grid_class_tile, grid_split, qc_arith: lk_quadtile.h — the rules the variant query reports)

extern "C" int lk_quadform_linear_grid_f32(const float* u, const float* v, const float* w0, const float* w1,
                                           const float* deltas, int64_t G, int mode, int64_t B, int64_t C, int64_t Do,
                                           int64_t Di, const float* ub, const float* wb, float* var, void* stream_) {
  LK_REQUIRE(u && v && w0 && deltas && var && G >= 1 && B >= 0 && C >= 1 && Do >= 1 && Di >= 1 && mode >= 0 && mode <= 2,
             "lk_quadform_linear_grid_f32: bad arguments");
  LK_REQUIRE(mode == GRID_DIAG || w1 != nullptr, "lk_quadform_linear_grid_f32: Kron modes need l2");
  LK_REQUIRE(ub == nullptr || wb != nullptr, "lk_quadform_linear_grid_f32: bias block needs its weights");
  LK_REQUIRE(G < (1ll << 24) && B < (1ll << 30) && C < (1ll << 24) && Do < (1ll << 24) && Di < (1ll << 24) &&
                 G * B * C < (1ll << 62),
             "lk_quadform_linear_grid_f32: sizes out of range");
  if (B == 0) return LK_OK;
  constexpr int NB = GRID_LIN_NB;
  constexpr size_t LDS_MAX = 150 * 1024;
  const size_t fixed = (size_t)NB * Di * sizeof(float), per_g = (size_t)NB * Do * sizeof(float);
  if (fixed + per_g > LDS_MAX) {
    set_error("lk_quadform_linear_grid_f32: layer too wide for the LDS-staged kernel (Di = %lld, Do = %lld)", (long long)Di,
              (long long)Do);
    return LK_EINVAL;
  }
  // as many grid points per LDS chunk as fit in 64 KiB (or the whole layer's minimum beyond that)
  int64_t GS = fixed < 64 * 1024 ? (int64_t)((64 * 1024 - fixed) / per_g) : 1;
  if (GS < 1) GS = 1;
  if (GS > G) GS = G;
  const size_t lds = fixed + (size_t)GS * per_g;
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid((unsigned)((B + NB - 1) / NB));
#define LK_LG_CASE(M)                                                                                                  \
  case M: {                                                                                                            \
    if (lds > 64 * 1024) {                                                                                             \
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&quadform_linear_grid_kernel<M>),               \
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                        \
      if (e != hipSuccess) {                                                                                           \
        set_error("lk_quadform_linear_grid_f32: cannot raise dynamic LDS limit: %s", hipGetErrorString(e));            \
        return LK_ELAUNCH;                                                                                             \
      }                                                                                                                \
    }                                                                                                                  \
    hipLaunchKernelGGL((quadform_linear_grid_kernel<M>), grid, dim3(256), lds, stream, u, v, w0, w1, deltas, (int)G,   \
                       (int)GS, (int)B, (int)C, (int)Do, (int)Di, ub, wb, var);                                         \
    break;                                                                                                             \
  }
  switch (mode) {
    LK_LG_CASE(GRID_KRON)
    LK_LG_CASE(GRID_KRON_DAMPED)
    LK_LG_CASE(GRID_DIAG)
  }
#undef LK_LG_CASE
  return check_launch("quadform_linear_grid_kernel");
}

extern "C" size_t lk_quadform_shared_grid_workspace_bytes(int64_t B, int64_t C, int64_t Do, int64_t Dk, int64_t G) {
  if (B < 1 || C < 1 || Do < 1 || Dk < 1 || G < 1) return 0;  // (B == 0: nothing to do, and grid_split divides by B)
  const int64_t gl = G < GRID_GMAX ? G : GRID_GMAX;
  return (size_t)B * grid_split(B, Do, Dk) * gl * grid_class_tile(C) * sizeof(float);
}

extern "C" int lk_quadform_shared_grid_f32(const float* u, const float* v, const float* w0, const float* w1,
                                           const float* deltas, int64_t G, int mode, int64_t B, int64_t C, int64_t Do,
                                           int64_t Dk, int64_t L, int seed_major, float* var, void* ws, size_t ws_bytes,
                                           void* stream_) {
  const char* what = "lk_quadform_shared_grid_f32";
  LK_REQUIRE(u && v && w0 && deltas && var && G >= 1 && B >= 0 && C >= 1 && Do >= 1 && Dk >= 1 && L >= 1 && mode >= 0 &&
                 mode <= 2,
             "lk_quadform_shared_grid_f32: bad arguments");
  LK_REQUIRE(mode == GRID_DIAG || w1 != nullptr, "lk_quadform_shared_grid_f32: Kron modes need l2");
  // the tile products index one sample's operands with 32 bits from its base pointer (as lk_kron_quadform_shared_*_f32)
  LK_REQUIRE(B * 64 < (1ll << 31) && L * Dk < (1ll << 29) &&
                 (seed_major ? C * B * L * Do < (1ll << 31) : C * L * Do < (1ll << 29)) && G * B * C < (1ll << 62),
             "lk_quadform_shared_grid_f32: sizes out of range");
  if (B == 0) return LK_OK;
  if (ws == nullptr || ws_bytes < lk_quadform_shared_grid_workspace_bytes(B, C, Do, Dk, G)) {
    set_error("%s: workspace too small", what);
    return LK_EWORKSPACE;
  }
  hipStream_t stream = (hipStream_t)stream_;
  const int ct = grid_class_tile(C);
  const int split = grid_split(B, Do, Dk);
  float* partial = static_cast<float*>(ws);
  const dim3 grid((unsigned)(B * split));
  const int64_t uss = seed_major ? Do * L : C * Do * L;
  const unsigned ucs = (unsigned)(seed_major ? B * Do * L : Do * L);
  // blocks of ct outputs (independent: only the diagonal is formed) x pieces of at most GRID_GMAX grid points
  for (int64_t c0 = 0; c0 < C; c0 += ct) {
    const int cl = (int)(C - c0 < ct ? C - c0 : ct);
    const float* uc = u + (size_t)c0 * ucs;
    const bool v4 = qc_arith(L, qc_aligned16(uc) && qc_aligned16(v)) == 1;
    for (int64_t g0 = 0; g0 < G; g0 += GRID_GMAX) {
      const int gl = (int)(G - g0 < GRID_GMAX ? G - g0 : GRID_GMAX);
      const float* dg = deltas + g0;
#define LK_SG_LAUNCH(CT, M)                                                                                             \
  do {                                                                                                                  \
    if (v4)                                                                                                             \
      hipLaunchKernelGGL((quadform_shared_grid_kernel<CT, M, 1>), grid, dim3(256), 0, stream, uc, v, w0, w1, dg, gl,    \
                         cl, (int)Do, (int)Dk, (int)L, split, partial, uss, ucs);                                        \
    else                                                                                                                \
      hipLaunchKernelGGL((quadform_shared_grid_kernel<CT, M, 0>), grid, dim3(256), 0, stream, uc, v, w0, w1, dg, gl,    \
                         cl, (int)Do, (int)Dk, (int)L, split, partial, uss, ucs);                                        \
  } while (0)
#define LK_SG_MODES(CT)                          \
  case CT:                                       \
    if (mode == GRID_KRON)                       \
      LK_SG_LAUNCH(CT, GRID_KRON);               \
    else if (mode == GRID_KRON_DAMPED)           \
      LK_SG_LAUNCH(CT, GRID_KRON_DAMPED);        \
    else                                         \
      LK_SG_LAUNCH(CT, GRID_DIAG);               \
    break;
      switch (ct) {
        LK_SG_MODES(1)
        LK_SG_MODES(2)
        LK_SG_MODES(5)
        LK_SG_MODES(10)
      }
#undef LK_SG_MODES
#undef LK_SG_LAUNCH
      const int64_t total = B * gl * cl;
      hipLaunchKernelGGL(quadform_shared_grid_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                         partial, B, gl, ct, cl, split, g0, C, c0, var);
    }
  }
  return check_launch(what);
}

extern "C" int lk_probit_nll_grid_f32(const float* f_mu, const float* var, const int64_t* labels, int64_t G, int64_t B,
                                      int64_t C, double* loss_sum, void* stream) {
  LK_REQUIRE(f_mu && var && labels && loss_sum && G >= 1 && B >= 0 && C >= 1 && G < (1ll << 31) && B < (1ll << 31) &&
                 C < (1ll << 24) && G * B * C < (1ll << 62),
             "lk_probit_nll_grid_f32: bad arguments");
  if (B == 0) return LK_OK;
  hipLaunchKernelGGL(probit_nll_grid_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, f_mu, var, labels,
                     (int)B, (int)C, loss_sum);
  return check_launch("probit_nll_grid_kernel");
}
