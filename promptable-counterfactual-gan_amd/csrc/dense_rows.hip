// dense_rows.hip — whole-batch nn.Linear (+ BatchNorm1d + activation) on v_mfma_f32_16x16x4_f32 for batches of at most 128 rows
// (simple_gan/mnist/mnist_gan.py:44-59,70-77: 100→128→256→512→1024→784 and 784→512→256→1 at batch 64).
//
// One workgroup (4 waves) owns ALL rows of a tile of 16 output columns, so it holds complete BatchNorm columns: the batch statistics,
// the normalisation, the running-statistics update and the activation are the forward GEMM's epilogue; the activation derivative and
// the whole BatchNorm backward of the layer below are the grad-input GEMM's epilogue.  The four waves split the contraction (k-steps
// of 16, interleaved), each requests the operands of 8 of its steps in one burst, and the partial tiles are added in wave order
// from LDS: a fixed summation order, bitwise repeatable.  The weight gradient contracts over the rows only (K <= 128): one
// workgroup per 64x64 tile of dW, no slab split and no tickets.
// No inter-workgroup hand-off of any kind (no fences in loops, no grid barrier).
// The *_post forms are the same tiles for a stage in the other order, Linear -> activation -> BatchNorm1d -> Dropout (the house-sales
// classifier in training mode, house_sales_kc_usa/models/nn_classifier.py:8-25): the statistics are taken of the
// activation's output, which is the one saved tensor, and the first layer's 17 columns take guarded scalar operand loads.
#include "pcg_common.h"

namespace pcg {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int DR_MAX_ROWS = 128;   // 8 m-tiles of 16 rows
constexpr int DR_MT = DR_MAX_ROWS / 16;
constexpr int DR_NT = 16;          // output columns per workgroup
constexpr int DR_LDP = 17;         // padded row of the partial-tile image in LDS

struct DrShared {
  float part[4][DR_MAX_ROWS][DR_LDP];   // per-wave partial tiles [row][column]
  float red[2][16][16];                 // column reductions: [which][row group][column]
};

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// B operand of the two GEMM forms.  ROWMAJOR_K (forward, y = x W^T): the 16 columns of the tile are rows of W, k runs along a row.
// else (grad-input, dx = dz W): k is the row of W, the tile's columns are contiguous in it.
// VEC (row-major K only): K % 4 == 0 and 16-byte aligned rows; the post-activation forward's first layer (17 columns) has neither.
template <bool ROWMAJOR_K, bool VEC = true>
__device__ __forceinline__ f32x4 dr_load_b(const float* __restrict__ W, int K, int N, int col, int k) {
  f32x4 b = {0.f, 0.f, 0.f, 0.f};
  if (col < N && k < K) {
    if (ROWMAJOR_K && VEC) {
      b = ld4(W + (size_t)col * K + k);
    } else if (ROWMAJOR_K) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (k + j < K) b[j] = W[(size_t)col * K + k + j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (k + j < K) b[j] = W[(size_t)(k + j) * N + col];
    }
  }
  return b;
}

// A operand: rows of the activation, 4 consecutive k per lane.  VEC: K % 4 == 0 and 16-byte aligned rows.
template <bool VEC>
__device__ __forceinline__ f32x4 dr_load_a(const float* __restrict__ A, int R, int K, int row, int k) {
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  if (row < R && k < K) {
    if (VEC) {
      a = ld4(A + (size_t)row * K + k);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (k + j < K) a[j] = A[(size_t)row * K + k + j];
    }
  }
  return a;
}

// part[wave] <- A[R][K] . B over this wave's k-steps, for the 16 columns from n0.  A k-step is 16 wide: the lane group g = lane >> 4
// holds k0 + 4g .. 4g+3 of its row (A) and of its column (B), and MFMA j contracts element j of every group: both operands see the
// same k per lane group, so the permutation inside a step only changes the (fixed) summation order.
// Wave w owns steps w, w + 4, w + 8, ...; it requests the operands of DR_CHUNK of its steps in ONE burst (what a
// short kernel costs is the number of dependent memory round trips), then issues their MFMAs: K <= 512 is one round trip per wave,
// K = 1024 two.  MT: m-tiles compiled in (4 for R <= 64, 8 above) -- the burst of 8 steps holds 8 * (MT + 1) * 4 VGPRs.
// A forward (B_ROWMAJOR_K) without A_VEC reads W with guarded scalar loads too: both operands have rows of K floats.  CHUNK: steps
// per burst (the scalar forward takes 2: its loads cost four address computations each, and its K is small).
constexpr int DR_CHUNK = 8;
template <bool B_ROWMAJOR_K, bool A_VEC, int MT, int CHUNK = DR_CHUNK>
__device__ __forceinline__ void dr_mainloop(DrShared& sh, const float* __restrict__ A, const float* __restrict__ W, int R, int K, int N,
                                            int n0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const int mt = (R + 15) >> 4;
  const int nsteps = (K + 15) >> 4;
  f32x4 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int s0 = wave; s0 < nsteps; s0 += 4 * CHUNK) {
    f32x4 b[CHUNK], a[CHUNK][MT];
#pragma unroll
    for (int c = 0; c < CHUNK; ++c) {
      const int s = s0 + 4 * c;
      const int k = s < nsteps ? s * 16 + 4 * g : K;   // k = K: nothing is loaded, the operands are 0
      b[c] = dr_load_b<B_ROWMAJOR_K, A_VEC>(W, K, N, n0 + r16, k);
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        a[c][m] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (m < mt) a[c][m] = dr_load_a<A_VEC>(A, R, K, m * 16 + r16, k);
      }
    }
#pragma unroll
    for (int c = 0; c < CHUNK; ++c) {
      if (s0 + 4 * c < nsteps) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int m = 0; m < MT; ++m)
            if (m < mt) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c][m][j], b[c][j], acc[m], 0, 0, 0);
        }
      }
    }
  }
  // C/D map of 16x16: column = lane & 15, row = 4 * (lane >> 4) + register
#pragma unroll
  for (int m = 0; m < MT; ++m)
    if (m < mt) {
#pragma unroll
      for (int j = 0; j < 4; ++j) sh.part[wave][m * 16 + 4 * g + j][r16] = acc[m][j];
    }
  __syncthreads();
}

// sum over the 16 row groups of one column, in row-group order: the same value in every thread of the column
__device__ __forceinline__ float dr_colsum(float (*red)[16], float mine, int rg, int c) {
  red[rg][c] = mine;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) s += red[q][c];
  return s;
}

struct DrFwd {
  const float *x, *W, *bias;
  int R, I, O;
  const float *gamma, *beta;
  float *running_mean, *running_var;
  long long* num_batches_tracked;
  float *save_mean, *save_invstd, *xhat;
  float eps, momentum;
  int training, act;
  float slope;
  float* y;
};

template <bool BN, int MT>
__global__ __launch_bounds__(256) void dense_rows_fwd_kernel(DrFwd a) {
  __shared__ DrShared sh;
  const int n0 = blockIdx.x * DR_NT;
  dr_mainloop<true, true, MT>(sh, a.x, a.W, a.R, a.I, a.O, n0);
  const int c = threadIdx.x & 15, rg = threadIdx.x >> 4, col = n0 + c;
  const bool cok = col < a.O;
  const float bias = (a.bias && cok) ? a.bias[col] : 0.f;
  float v[DR_MT];
#pragma unroll
  for (int i = 0; i < DR_MT; ++i) {
    const int r = rg + 16 * i;
    v[i] = r < a.R ? ((sh.part[0][r][c] + sh.part[1][r][c]) + (sh.part[2][r][c] + sh.part[3][r][c])) + bias : 0.f;
  }
  float gam = 1.f, bet = 0.f, mean = 0.f, invstd = 1.f;
  if (BN) {
    gam = cok ? a.gamma[col] : 1.f;
    bet = cok ? a.beta[col] : 0.f;
    if (a.training) {
      float s1 = 0.f;
#pragma unroll
      for (int i = 0; i < DR_MT; ++i) s1 += v[i];                       // rows >= R hold 0
      mean = dr_colsum(sh.red[0], s1, rg, c) / (float)a.R;
      float s2 = 0.f;
#pragma unroll
      for (int i = 0; i < DR_MT; ++i)
        if (rg + 16 * i < a.R) s2 += (v[i] - mean) * (v[i] - mean);
      const float var = dr_colsum(sh.red[1], s2, rg, c) / (float)a.R;    // biased: what normalises
      invstd = 1.f / sqrtf(var + a.eps);
      if (rg == 0 && cok) {
        a.save_mean[col] = mean;
        a.save_invstd[col] = invstd;
        if (a.running_mean) a.running_mean[col] = (1.f - a.momentum) * a.running_mean[col] + a.momentum * mean;
        if (a.running_var)
          a.running_var[col] = (1.f - a.momentum) * a.running_var[col] + a.momentum * (var * ((float)a.R / (float)(a.R - 1)));
      }
      if (blockIdx.x == 0 && threadIdx.x == 0 && a.num_batches_tracked) *a.num_batches_tracked += 1;
    } else {
      mean = cok ? a.running_mean[col] : 0.f;
      invstd = 1.f / sqrtf((cok ? a.running_var[col] : 1.f) + a.eps);
    }
  }
  if (!cok) return;
#pragma unroll
  for (int i = 0; i < DR_MT; ++i) {
    const int r = rg + 16 * i;
    if (r < a.R) {
      float t = v[i];
      if (BN) {
        const float xh = (t - mean) * invstd;
        if (a.xhat) a.xhat[(size_t)r * a.O + col] = xh;
        t = fmaf(xh, gam, bet);
      }
      a.y[(size_t)r * a.O + col] = act_apply(t, a.act, a.slope);
    }
  }
}

struct DrDgrad {
  const float *dz, *W;
  int R, O, I;
  int act;
  float slope;
  const float* y_below;
  const float *xhat, *gamma, *invstd;
  float *dgamma, *dbeta;
  int accumulate;
  float* dx;
};

template <bool A_VEC, bool BN, int MT>
__global__ __launch_bounds__(256) void dense_rows_dgrad_kernel(DrDgrad a) {
  __shared__ DrShared sh;
  const int n0 = blockIdx.x * DR_NT;
  dr_mainloop<false, A_VEC, MT>(sh, a.dz, a.W, a.R, a.O, a.I, n0);
  const int c = threadIdx.x & 15, rg = threadIdx.x >> 4, col = n0 + c;
  const bool cok = col < a.I;
  float gr[DR_MT], xh[DR_MT];
#pragma unroll
  for (int i = 0; i < DR_MT; ++i) {
    const int r = rg + 16 * i;
    gr[i] = 0.f;
    xh[i] = 0.f;
    if (r < a.R && cok) {
      float t = (sh.part[0][r][c] + sh.part[1][r][c]) + (sh.part[2][r][c] + sh.part[3][r][c]);
      if (a.act != PCG_ACT_NONE) t *= act_grad_from_out(a.y_below[(size_t)r * a.I + col], a.act, a.slope);
      gr[i] = t;
      if (BN) xh[i] = a.xhat[(size_t)r * a.I + col];
    }
  }
  float k0 = 1.f, m1 = 0.f, m2 = 0.f;
  if (BN) {
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < DR_MT; ++i) {
      s1 += gr[i];
      s2 = fmaf(gr[i], xh[i], s2);
    }
    s1 = dr_colsum(sh.red[0], s1, rg, c);   // dbeta
    s2 = dr_colsum(sh.red[1], s2, rg, c);   // dgamma
    if (cok) {
      if (rg == 0) {
        a.dbeta[col] = a.accumulate ? a.dbeta[col] + s1 : s1;
        a.dgamma[col] = a.accumulate ? a.dgamma[col] + s2 : s2;
      }
      k0 = a.gamma[col] * a.invstd[col];
      m1 = s1 / (float)a.R;
      m2 = s2 / (float)a.R;
    }
  }
  if (!cok) return;
#pragma unroll
  for (int i = 0; i < DR_MT; ++i) {
    const int r = rg + 16 * i;
    if (r < a.R) a.dx[(size_t)r * a.I + col] = BN ? k0 * ((gr[i] - m1) - xh[i] * m2) : gr[i];
  }
}

// ---- the post-activation stage: Linear -> activation -> BatchNorm1d (batch statistics) -> Dropout ---------------------------------
// (house_sales_kc_usa/models/nn_classifier.py:8-25 in training mode).  The forward's epilogue holds complete columns of a = act(z), so
// the statistics are taken of a; the only saved activation is a: the backward recomputes x-hat from (a, mean, invstd) with the
// forward's expression and takes act' from a's sign.
struct DrFwdPost {
  const float *x, *W, *bias;
  int R, I, O;
  int act;
  float slope;
  const float *gamma, *beta;
  float *running_mean, *running_var;
  long long* num_batches_tracked;
  float eps, momentum;
  const float* mask;
  float scale;
  float *a, *save_mean, *save_invstd, *y;
};

template <bool VEC, int MT>
__global__ __launch_bounds__(256) void dense_rows_fwd_post_kernel(DrFwdPost a) {
  __shared__ DrShared sh;
  const int n0 = blockIdx.x * DR_NT;
  dr_mainloop<true, VEC, MT, VEC ? DR_CHUNK : 2>(sh, a.x, a.W, a.R, a.I, a.O, n0);
  const int c = threadIdx.x & 15, rg = threadIdx.x >> 4, col = n0 + c;
  const bool cok = col < a.O;
  const float bias = (a.bias && cok) ? a.bias[col] : 0.f;
  float v[DR_MT];
#pragma unroll
  for (int i = 0; i < DR_MT; ++i) {
    const int r = rg + 16 * i;
    v[i] = r < a.R ? act_apply(((sh.part[0][r][c] + sh.part[1][r][c]) + (sh.part[2][r][c] + sh.part[3][r][c])) + bias, a.act, a.slope) : 0.f;
  }
  const float gam = cok ? a.gamma[col] : 1.f, bet = cok ? a.beta[col] : 0.f;
  float s1 = 0.f;
#pragma unroll
  for (int i = 0; i < DR_MT; ++i) s1 += v[i];                         // rows >= R hold 0
  const float mean = dr_colsum(sh.red[0], s1, rg, c) / (float)a.R;
  float s2 = 0.f;
#pragma unroll
  for (int i = 0; i < DR_MT; ++i)
    if (rg + 16 * i < a.R) s2 += (v[i] - mean) * (v[i] - mean);
  const float var = dr_colsum(sh.red[1], s2, rg, c) / (float)a.R;      // biased: what normalises
  const float invstd = 1.f / sqrtf(var + a.eps);
  if (rg == 0 && cok) {
    a.save_mean[col] = mean;
    a.save_invstd[col] = invstd;
    if (a.running_mean) a.running_mean[col] = (1.f - a.momentum) * a.running_mean[col] + a.momentum * mean;
    if (a.running_var)
      a.running_var[col] = (1.f - a.momentum) * a.running_var[col] + a.momentum * (var * ((float)a.R / (float)(a.R - 1)));
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && a.num_batches_tracked) *a.num_batches_tracked += 1;
  if (!cok) return;                                                    // (after the column-sum barriers)
#pragma unroll
  for (int i = 0; i < DR_MT; ++i) {
    const int r = rg + 16 * i;
    if (r < a.R) {
      const size_t at = (size_t)r * a.O + col;
      a.a[at] = v[i];
      const float xh = (v[i] - mean) * invstd;                         // dense_rows_dgrad_post_kernel repeats this expression
      float t = fmaf(xh, gam, bet);
      if (a.mask) t = t * a.mask[at] * a.scale;
      a.y[at] = t;
    }
  }
}

struct DrDgradPost {
  const float *dz, *W;
  int R, O, I;
  const float* mask;
  float scale;
  const float *a, *mean, *invstd, *gamma;
  int act;
  float slope;
  float *dgamma, *dbeta, *db;
  int accumulate;
  float* dx;
};

// g = dz W, then Dropout', BatchNorm' and act' of the stage below, in that order (dense_rows_dgrad_kernel: act' first, then BatchNorm')
template <bool A_VEC, int MT>
__global__ __launch_bounds__(256) void dense_rows_dgrad_post_kernel(DrDgradPost a) {
  __shared__ DrShared sh;
  const int n0 = blockIdx.x * DR_NT;
  dr_mainloop<false, A_VEC, MT>(sh, a.dz, a.W, a.R, a.O, a.I, n0);
  const int c = threadIdx.x & 15, rg = threadIdx.x >> 4, col = n0 + c;
  const bool cok = col < a.I;
  const float mean = cok ? a.mean[col] : 0.f, invstd = cok ? a.invstd[col] : 1.f;
  float dn[DR_MT], xh[DR_MT], der[DR_MT];
#pragma unroll
  for (int i = 0; i < DR_MT; ++i) {
    const int r = rg + 16 * i;
    dn[i] = 0.f;
    xh[i] = 0.f;
    der[i] = 1.f;
    if (r < a.R && cok) {
      const size_t at = (size_t)r * a.I + col;
      float t = (sh.part[0][r][c] + sh.part[1][r][c]) + (sh.part[2][r][c] + sh.part[3][r][c]);
      if (a.mask) t = t * a.mask[at] * a.scale;
      dn[i] = t;
      const float av = a.a[at];
      xh[i] = (av - mean) * invstd;
      der[i] = act_grad_from_out(av, a.act, a.slope);
    }
  }
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < DR_MT; ++i) {
    s1 += dn[i];
    s2 = fmaf(dn[i], xh[i], s2);
  }
  s1 = dr_colsum(sh.red[0], s1, rg, c);   // dbeta
  s2 = dr_colsum(sh.red[1], s2, rg, c);   // dgamma
  const float k0 = cok ? a.gamma[col] * invstd : 0.f, m1 = s1 / (float)a.R, m2 = s2 / (float)a.R;
  float s3 = 0.f;
#pragma unroll
  for (int i = 0; i < DR_MT; ++i) {
    const int r = rg + 16 * i;
    if (r < a.R && cok) {
      const float d = (k0 * ((dn[i] - m1) - xh[i] * m2)) * der[i];
      a.dx[(size_t)r * a.I + col] = d;
      s3 += d;
    }
  }
  // the bias gradient of the stage's Linear is the column sum of dx, and the column is complete here (red[0] is free again: every
  // thread has passed the barrier of the second sum)
  if (a.db) s3 = dr_colsum(sh.red[0], s3, rg, c);                // kernel-uniform
  if (!cok || rg != 0) return;                                   // (after the column-sum barriers)
  a.dbeta[col] = a.accumulate ? a.dbeta[col] + s1 : s1;
  a.dgamma[col] = a.accumulate ? a.dgamma[col] + s2 : s2;
  if (a.db) a.db[col] = a.accumulate ? a.db[col] + s3 : s3;
}

// dW[O][I] (+)= dz^T x over all R rows; db[O] (+)= column sums of dz.  Workgroup: 64 (o) x 64 (i); wave w: rows of dW o0 + 16w .. +15.
__global__ __launch_bounds__(256) void dense_rows_wgrad_kernel(const float* __restrict__ dz, const float* __restrict__ x, int R, int O, int I,
                                                               float* __restrict__ dW, float* __restrict__ db, int accumulate) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c16 = lane & 15, g = lane >> 4;
  const int o = blockIdx.y * 64 + wave * 16 + c16;   // A operand: M index
  const int i0 = blockIdx.x * 64 + c16;              // B operand: N index of n-tile 0
  f32x4 acc[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int r0 = 0; r0 < R; r0 += 64) {   // 16 k-steps of 4 rows: 80 loads requested in one burst, then 64 MFMAs
    float av[16], bv[16][4];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int r = r0 + 4 * q + g;
      const bool rok = r < R;
      av[q] = (rok && o < O) ? dz[(size_t)r * O + o] : 0.f;
#pragma unroll
      for (int n = 0; n < 4; ++n) bv[q][n] = (rok && i0 + 16 * n < I) ? x[(size_t)r * I + i0 + 16 * n] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      if (r0 + 4 * q < R) {
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q], bv[q][n], acc[n], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int ic = i0 + 16 * n;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int orow = blockIdx.y * 64 + wave * 16 + 4 * g + j;
      if (orow < O && ic < I) {
        float* p = dW + (size_t)orow * I + ic;
        *p = accumulate ? *p + acc[n][j] : acc[n][j];
      }
    }
  }
  if (db && blockIdx.x == 0 && threadIdx.x < 64) {
    const int oc = blockIdx.y * 64 + threadIdx.x;
    if (oc < O) {
      float s = 0.f;
      for (int r = 0; r < R; ++r) s += dz[(size_t)r * O + oc];
      db[oc] = accumulate ? db[oc] + s : s;
    }
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace
}  // namespace pcg

using namespace pcg;

extern "C" int pcg_dense_rows_fwd(const float* x, const float* W, const float* bias, int32_t R, int32_t I, int32_t O,
                                  const pcg_dense_bn* bn, int act, float slope, float* y, pcg_stream_t stream) {
  PCG_REQUIRE(x && W && y && I > 0 && O > 0, "pcg_dense_rows_fwd: bad arguments");
  PCG_REQUIRE(R >= 1 && R <= DR_MAX_ROWS, "pcg_dense_rows_fwd: %d rows; one workgroup holds the whole batch, 1 <= R <= %d", R, DR_MAX_ROWS);
  PCG_REQUIRE(I % 4 == 0, "pcg_dense_rows_fwd: in_features %d is not a multiple of 4 (16-byte operand loads)", I);
  PCG_REQUIRE(al16(x) && al16(W), "pcg_dense_rows_fwd: x and W must be 16-byte aligned");
  PCG_REQUIRE(act >= PCG_ACT_NONE && act <= PCG_ACT_SIGMOID, "pcg_dense_rows_fwd: unknown activation %d", act);
  DrFwd a{};
  a.x = x; a.W = W; a.bias = bias; a.R = R; a.I = I; a.O = O; a.act = act; a.slope = slope; a.y = y;
  if (bn) {
    PCG_REQUIRE(bn->gamma && bn->beta, "pcg_dense_rows_fwd: BatchNorm needs gamma and beta");
    if (bn->training) {
      PCG_REQUIRE(R >= 2, "pcg_dense_rows_fwd: training-mode BatchNorm needs more than 1 row (got %d)", R);
      PCG_REQUIRE(bn->save_mean && bn->save_invstd, "pcg_dense_rows_fwd: training-mode BatchNorm needs save_mean and save_invstd");
    } else {
      PCG_REQUIRE(bn->running_mean && bn->running_var, "pcg_dense_rows_fwd: evaluation-mode BatchNorm needs the running statistics");
    }
    a.gamma = bn->gamma; a.beta = bn->beta; a.running_mean = bn->running_mean; a.running_var = bn->running_var;
    a.num_batches_tracked = (long long*)bn->num_batches_tracked;
    a.save_mean = bn->save_mean; a.save_invstd = bn->save_invstd; a.xhat = bn->xhat;
    a.eps = bn->eps; a.momentum = bn->momentum; a.training = bn->training;
  }
  const dim3 grid(ceil_div(O, DR_NT));
  hipStream_t s = (hipStream_t)stream;
  const bool small = R <= 64;     // 4 m-tiles compiled in: half the operand registers of the burst
  if (bn && small) hipLaunchKernelGGL((dense_rows_fwd_kernel<true, 4>), grid, dim3(256), 0, s, a);
  else if (bn) hipLaunchKernelGGL((dense_rows_fwd_kernel<true, 8>), grid, dim3(256), 0, s, a);
  else if (small) hipLaunchKernelGGL((dense_rows_fwd_kernel<false, 4>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((dense_rows_fwd_kernel<false, 8>), grid, dim3(256), 0, s, a);
  return launch_status("dense_rows_fwd_kernel");
}

extern "C" int pcg_dense_rows_dgrad(const float* dz, const float* W, int32_t R, int32_t O, int32_t I, int below_act, float below_slope,
                                    const float* y_below, const pcg_dense_bn_bwd* bn, float* dx, pcg_stream_t stream) {
  PCG_REQUIRE(dz && W && dx && I > 0 && O > 0, "pcg_dense_rows_dgrad: bad arguments");
  PCG_REQUIRE(R >= 1 && R <= DR_MAX_ROWS, "pcg_dense_rows_dgrad: %d rows; one workgroup holds the whole batch, 1 <= R <= %d", R, DR_MAX_ROWS);
  PCG_REQUIRE(below_act >= PCG_ACT_NONE && below_act <= PCG_ACT_SIGMOID, "pcg_dense_rows_dgrad: unknown activation %d", below_act);
  PCG_REQUIRE(below_act == PCG_ACT_NONE || y_below, "pcg_dense_rows_dgrad: the activation derivative needs the layer's output y_below");
  DrDgrad a{};
  a.dz = dz; a.W = W; a.R = R; a.O = O; a.I = I; a.act = below_act; a.slope = below_slope; a.y_below = y_below; a.dx = dx;
  if (bn) {
    PCG_REQUIRE(R >= 2, "pcg_dense_rows_dgrad: BatchNorm backward needs more than 1 row (got %d)", R);
    PCG_REQUIRE(bn->xhat && bn->gamma && bn->invstd && bn->dgamma && bn->dbeta,
                "pcg_dense_rows_dgrad: BatchNorm backward needs xhat, gamma, invstd, dgamma and dbeta");
    a.xhat = bn->xhat; a.gamma = bn->gamma; a.invstd = bn->invstd; a.dgamma = bn->dgamma; a.dbeta = bn->dbeta;
    a.accumulate = bn->accumulate;
  }
  const bool vec = O % 4 == 0 && al16(dz);
  const dim3 grid(ceil_div(I, DR_NT));
  hipStream_t s = (hipStream_t)stream;
#define DR_DGRAD(V, B, M) hipLaunchKernelGGL((dense_rows_dgrad_kernel<V, B, M>), grid, dim3(256), 0, s, a)
  if (R <= 64) {     // 4 m-tiles compiled in
    if (vec && bn) DR_DGRAD(true, true, 4); else if (vec) DR_DGRAD(true, false, 4); else if (bn) DR_DGRAD(false, true, 4); else DR_DGRAD(false, false, 4);
  } else {
    if (vec && bn) DR_DGRAD(true, true, 8); else if (vec) DR_DGRAD(true, false, 8); else if (bn) DR_DGRAD(false, true, 8); else DR_DGRAD(false, false, 8);
  }
#undef DR_DGRAD
  return launch_status("dense_rows_dgrad_kernel");
}

extern "C" int pcg_dense_rows_fwd_post(const float* x, const float* W, const float* bias, int32_t R, int32_t I, int32_t O, int act, float slope,
                                       const float* gamma, const float* beta, float* running_mean, float* running_var,
                                       int64_t* num_batches_tracked, float eps, float momentum, const float* mask, float scale, float* a,
                                       float* save_mean, float* save_invstd, float* y, pcg_stream_t stream) {
  PCG_REQUIRE(x && W && y && gamma && beta && I > 0 && O > 0, "pcg_dense_rows_fwd_post: bad arguments");
  PCG_REQUIRE(R >= 2 && R <= DR_MAX_ROWS,
              "pcg_dense_rows_fwd_post: %d rows; one workgroup holds the whole batch and its BatchNorm statistics, 2 <= R <= %d", R, DR_MAX_ROWS);
  PCG_REQUIRE(act == PCG_ACT_NONE || act == PCG_ACT_LRELU, "pcg_dense_rows_fwd_post: unknown activation %d (none or LeakyReLU)", act);
  PCG_REQUIRE(a && save_mean && save_invstd, "pcg_dense_rows_fwd_post: the backward needs a, save_mean and save_invstd");
  DrFwdPost p{};
  p.x = x; p.W = W; p.bias = bias; p.R = R; p.I = I; p.O = O; p.act = act; p.slope = slope; p.gamma = gamma; p.beta = beta;
  p.running_mean = running_mean; p.running_var = running_var; p.num_batches_tracked = (long long*)num_batches_tracked;
  p.eps = eps; p.momentum = momentum; p.mask = mask; p.scale = scale; p.a = a; p.save_mean = save_mean; p.save_invstd = save_invstd; p.y = y;
  const bool vec = I % 4 == 0 && al16(x) && al16(W);
  const dim3 grid(ceil_div(O, DR_NT));
  hipStream_t s = (hipStream_t)stream;
#define DR_FWD_POST(V, M) hipLaunchKernelGGL((dense_rows_fwd_post_kernel<V, M>), grid, dim3(256), 0, s, p)
  if (R <= 64) {     // 4 m-tiles compiled in
    if (vec) DR_FWD_POST(true, 4); else DR_FWD_POST(false, 4);
  } else {
    if (vec) DR_FWD_POST(true, 8); else DR_FWD_POST(false, 8);
  }
#undef DR_FWD_POST
  return launch_status("dense_rows_fwd_post_kernel");
}

extern "C" int pcg_dense_rows_dgrad_post(const float* dz, const float* W, int32_t R, int32_t O, int32_t I, const float* mask, float scale,
                                         const float* a, const float* mean, const float* invstd, const float* gamma, int act, float slope,
                                         float* dgamma, float* dbeta, float* db, int accumulate, float* dx, pcg_stream_t stream) {
  PCG_REQUIRE(dz && W && dx && I > 0 && O > 0, "pcg_dense_rows_dgrad_post: bad arguments");
  PCG_REQUIRE(R >= 2 && R <= DR_MAX_ROWS,
              "pcg_dense_rows_dgrad_post: %d rows; one workgroup holds the whole batch and its BatchNorm sums, 2 <= R <= %d", R, DR_MAX_ROWS);
  PCG_REQUIRE(act == PCG_ACT_NONE || act == PCG_ACT_LRELU, "pcg_dense_rows_dgrad_post: unknown activation %d (none or LeakyReLU)", act);
  PCG_REQUIRE(a && mean && invstd && gamma && dgamma && dbeta,
              "pcg_dense_rows_dgrad_post: the stage's backward needs a, mean, invstd, gamma, dgamma and dbeta");
  DrDgradPost p{};
  p.dz = dz; p.W = W; p.R = R; p.O = O; p.I = I; p.mask = mask; p.scale = scale; p.a = a; p.mean = mean; p.invstd = invstd; p.gamma = gamma;
  p.act = act; p.slope = slope; p.dgamma = dgamma; p.dbeta = dbeta; p.db = db; p.accumulate = accumulate; p.dx = dx;
  const bool vec = O % 4 == 0 && al16(dz);
  const dim3 grid(ceil_div(I, DR_NT));
  hipStream_t s = (hipStream_t)stream;
#define DR_DGRAD_POST(V, M) hipLaunchKernelGGL((dense_rows_dgrad_post_kernel<V, M>), grid, dim3(256), 0, s, p)
  if (R <= 64) {     // 4 m-tiles compiled in
    if (vec) DR_DGRAD_POST(true, 4); else DR_DGRAD_POST(false, 4);
  } else {
    if (vec) DR_DGRAD_POST(true, 8); else DR_DGRAD_POST(false, 8);
  }
#undef DR_DGRAD_POST
  return launch_status("dense_rows_dgrad_post_kernel");
}

extern "C" int pcg_dense_rows_wgrad(const float* dz, const float* x, int32_t R, int32_t O, int32_t I, float* dW, float* db, int accumulate,
                                    pcg_stream_t stream) {
  PCG_REQUIRE(dz && x && dW && I > 0 && O > 0, "pcg_dense_rows_wgrad: bad arguments");
  PCG_REQUIRE(R >= 1 && R <= DR_MAX_ROWS, "pcg_dense_rows_wgrad: %d rows; one workgroup reduces over the whole batch, 1 <= R <= %d", R, DR_MAX_ROWS);
  const dim3 grid(ceil_div(I, 64), ceil_div(O, 64));
  PCG_REQUIRE(grid.y <= 65535, "pcg_dense_rows_wgrad: out_features %d is too wide for the launch grid", O);
  hipLaunchKernelGGL(dense_rows_wgrad_kernel, grid, dim3(256), 0, (hipStream_t)stream, dz, x, R, O, I, dW, db, accumulate);
  return launch_status("dense_rows_wgrad_kernel");
}
