// mnist_clf.hip — the launches around the convolutions of the MNIST classifier's pre-training step
// (conditional_counteRGAN/mnist/trainer.py:16-21 on models/classifier.py:7-22).  All fp32, every sum in a fixed
// order, no floating-point atomics, no grid barrier and no fence; every entry takes a stream and can be captured.
//
//   pcg_drop2d_flatten_fwd   nn.Dropout2d(0.25) + nn.Flatten of the NCHW tensor (classifier.py:14,17) from the NHWC activation
//   pcg_drop2d_flatten_bwd   their backward and the derivative of the ReLU in front of them (classifier.py:13)
//   pcg_mnist_clf_head       nn.Dropout(0.5), Linear(256, K), CrossEntropyLoss (classifier.py:20-21, trainer.py:10,19) and their
//                            backward down to fc1's pre-activation gradient and bias gradient (trainer.py:20), one workgroup
//
// The batch entry pcg_mnist_clf_batch(_counter) is in rng.hip, next to the Philox draws it shares with pcg_house_clf_batch.
#include "pcg_common.h"

namespace pcg {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
__device__ __forceinline__ f32x4 mc_ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// ---- Dropout2d + Flatten: a transposition of every row's [HW][C] image to [C][HW] through a 32 x 32 LDS tile -------------------
// Reads and writes are 128-byte runs on both sides.  The products are those of dropout_apply_kernel ((x * mask) * scale) and of
// act_bwd_kernel (dy * act'(y)), in their order, so the outputs carry the bits of the launch chains they replace.
template <bool BWD>
__global__ void __launch_bounds__(256) drop2d_flatten_kernel(const float* __restrict__ src, const float* __restrict__ mask, float scale,
                                                             const float* __restrict__ y, int act, float slope, int HW, int C, int tiles_c,
                                                             float* __restrict__ out) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int tp = (int)blockIdx.x / tiles_c, tc = (int)blockIdx.x - tp * tiles_c;
  const int p0 = tp * 32, c0 = tc * 32;
  const size_t row = (size_t)blockIdx.y * HW * C;            // both sides hold HW * C floats per batch row
  const float* __restrict__ mrow = mask + (size_t)blockIdx.y * C;
  if (!BWD) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p = p0 + ty + 8 * q, c = c0 + tx;
      if (p < HW && c < C) tile[ty + 8 * q][tx] = src[row + (size_t)p * C + c] * mrow[c] * scale;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = c0 + ty + 8 * q, p = p0 + tx;
      if (p < HW && c < C) out[row + (size_t)c * HW + p] = tile[tx][ty + 8 * q];
    }
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = c0 + ty + 8 * q, p = p0 + tx;
      if (p < HW && c < C) tile[ty + 8 * q][tx] = src[row + (size_t)c * HW + p];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p = p0 + ty + 8 * q, c = c0 + tx;
      if (p < HW && c < C) {
        const size_t i = row + (size_t)p * C + c;
        const float d = tile[tx][ty + 8 * q] * mrow[c] * scale;
        out[i] = d * act_grad_from_out(y[i], act, slope);
      }
    }
  }
}

// ---- the head: everything above fc1's output in one workgroup of 16 waves ---------------------------------------------------------
constexpr int MH_ROWS = 128;       // 8 m-tiles of 16 rows
constexpr int MH_I = 256;          // fc1's width: 16 n-tiles, one per wave
constexpr int MH_K = 16;           // classes, padded to one MFMA tile
constexpr int MH_LDW = MH_I + 4;   // padded row of W2 in LDS (16-byte aligned)
constexpr int MH_LDK = 17;         // padded row of the logits image

struct MhShared {
  alignas(16) float w2[MH_K][MH_LDW];   // W2, rows >= K zero
  alignas(16) float dl[MH_ROWS][MH_K];  // dlogits, rows >= R and columns >= K zero; a row is one 16-byte-aligned A operand of (5)
  float lg[MH_ROWS][MH_LDK];       // logits
  float b2[MH_K];
  float red[256];
  int hits[256];
};

struct MhArgs {
  const float *h, *m1;
  float scale;
  const float *W2, *b2;
  const int64_t* y;
  int R, K;
  float *logits, *loss;
  double* tally;
  float *dW2, *db2, *dh, *db1;
};

__global__ void __launch_bounds__(1024) mnist_clf_head_kernel(MhArgs a) {
  __shared__ MhShared sh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const int R = a.R, K = a.K;
  const int mt = (R + 15) >> 4;
  const float* __restrict__ h = a.h;
  const float* __restrict__ m1 = a.m1;
  const float scale = a.scale;

  // (1) logits = (h * m1 * scale) W2^T: wave w < ceil(R / 16) owns the 16 rows of m-tile w and the whole contraction, 8 k-steps of 16
  // per burst.  The first burst is requested before W2 is staged, so the two round trips overlap.
  const int row = wave * 16 + r16;
  auto a_burst = [&](int s0, f32x4 (&av)[8]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int k = (s0 + c) * 16 + 4 * g;
      av[c] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (wave < mt && row < R) av[c] = mc_ld4(h + (size_t)row * MH_I + k) * mc_ld4(m1 + (size_t)row * MH_I + k) * scale;
    }
  };
  f32x4 av[8];
  a_burst(0, av);
  for (int i = tid; i < MH_K * MH_I; i += 1024) {
    const int k = i >> 8, c = i & (MH_I - 1);
    sh.w2[k][c] = k < K ? a.W2[(size_t)k * MH_I + c] : 0.f;
  }
  for (int i = tid; i < MH_ROWS * MH_K; i += 1024) (&sh.dl[0][0])[i] = 0.f;
  if (tid < MH_K) sh.b2[tid] = tid < K ? a.b2[tid] : 0.f;
  __syncthreads();
  if (wave < mt) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s0 = 0; s0 < MH_I / 16; s0 += 8) {
      if (s0) a_burst(s0, av);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const f32x4 bv = mc_ld4(&sh.w2[r16][(s0 + c) * 16 + 4 * g]);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c][j], bv[j], acc, 0, 0, 0);
      }
    }
    // C/D map of 16x16: column = lane & 15, row = 4 * (lane >> 4) + register
#pragma unroll
    for (int j = 0; j < 4; ++j) sh.lg[wave * 16 + 4 * g + j][r16] = acc[j];
  }
  // the operands of (4) and (5) -- column `col` of h and m1 in every row this lane meets there -- are requested now, in one burst,
  // and arrive while (2) runs
  const int col = wave * 16 + r16;
  float hv[MH_ROWS / 16][4], mv[MH_ROWS / 16][4];
#pragma unroll
  for (int m = 0; m < MH_ROWS / 16; ++m)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = m * 16 + 4 * g + j;
      hv[m][j] = 0.f;
      mv[m][j] = 0.f;
      if (r < R) {
        hv[m][j] = h[(size_t)r * MH_I + col];
        mv[m][j] = m1[(size_t)r * MH_I + col];
      }
    }
  __syncthreads();

  // (2) bias, softmax, loss and dlogits: thread b < R owns row b; the two reductions fold 256 partials in halves
  if (tid < 256) {
    float acc = 0.f;
    int hit = 0;
    if (tid < R) {
      float* z = sh.lg[tid];
      for (int k = 0; k < K; ++k) {
        z[k] += sh.b2[k];
        a.logits[(size_t)tid * K + k] = z[k];
      }
      float mx = z[0];
      int arg = 0;
      for (int k = 1; k < K; ++k)
        if (z[k] > mx) { mx = z[k]; arg = k; }                   // first maximum, as torch.argmax: a tie counts for the lower index
      float se = 0.f;
      for (int k = 0; k < K; ++k) se += expf(z[k] - mx);
      const float lse = mx + logf(se);
      int64_t t = a.y[tid];
      t = t < 0 ? 0 : (t >= K ? K - 1 : t);
      acc = lse - z[(int)t];
      hit = arg == (int)t ? 1 : 0;
      const float inv = 1.f / (float)R;
      for (int k = 0; k < K; ++k) sh.dl[tid][k] = (expf(z[k] - lse) - (k == (int)t ? 1.f : 0.f)) * inv;
    }
    sh.red[tid] = acc;
    sh.hits[tid] = hit;
  }
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) { sh.red[tid] += sh.red[tid + s]; sh.hits[tid] += sh.hits[tid + s]; }
    __syncthreads();
  }
  if (tid == 0) {
    const float loss = sh.red[0] / (float)R;
    a.loss[0] = loss;
    a.tally[0] += (double)loss * (double)R;
    a.tally[1] += (double)sh.hits[0];
    a.tally[2] += (double)R;
  }

  // (3) db2: column sums of dlogits on the last wave: lane (column, g) adds rows g, g + 4, ... (rows >= R hold 0), then the four lane
  // groups fold by two butterfly steps
  if (wave == 15) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < MH_ROWS; r += 4) s += sh.dl[r + g][r16];
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (g == 0 && r16 < K) a.db2[r16] = s;
  }

  // (4) dW2 = dlogits^T (h * m1 * scale): wave w owns the 16 columns of n-tile w; the contraction runs over the rows
  {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < MH_ROWS / 16; ++m)
      if (m < mt) {                                              // wave-uniform; rows >= R of dl and of the operands are zero
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(sh.dl[m * 16 + 4 * g + j][r16], hv[m][j] * mv[m][j] * scale, acc, 0, 0, 0);
      }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * g + j < K) a.dW2[(size_t)(4 * g + j) * MH_I + col] = acc[j];
  }

  // (5) dh = (dlogits W2) * m1 * scale * [h > 0] and its column sums: wave w owns the 16 columns of n-tile w over every m-tile, the
  // K-long contraction (padded to 16) is four MFMAs per tile, and a column's sum is complete inside the wave: rows in m-tile and
  // register order per lane, then the four lane groups by two butterfly steps.
  {
    float bw[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) bw[q] = sh.w2[4 * g + q][col];
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < MH_ROWS / 16; ++m) {
      if (m < mt) {                                              // wave-uniform
        const f32x4 dv = mc_ld4(&sh.dl[m * 16 + r16][4 * g]);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[q], bw[q], acc, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = m * 16 + 4 * g + j;
          if (r < R) {
            const float v = acc[j] * mv[m][j] * scale * act_grad_from_out(hv[m][j], PCG_ACT_RELU, 0.f);
            a.dh[(size_t)r * MH_I + col] = v;
            s += v;
          }
        }
      }
    }
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (g == 0) a.db1[col] = s;
  }
}

}  // namespace
}  // namespace pcg

using namespace pcg;

// Dropout2d + nn.Flatten of the NCHW tensor in one launch (classifier.py:14,17): out[b][c * HW + p] = a[b][p][c] * mask[b][c] * scale.
extern "C" int pcg_drop2d_flatten_fwd(const float* a, const float* mask, float scale, int32_t R, int32_t HW, int32_t C, float* out,
                                      pcg_stream_t stream) {
  PCG_REQUIRE(a && mask && out && a != out && R > 0 && R <= 65535 && HW > 0 && C > 0, "pcg_drop2d_flatten_fwd: bad arguments");
  const int tiles_c = (C + 31) / 32, tiles_p = (HW + 31) / 32;
  hipLaunchKernelGGL(drop2d_flatten_kernel<false>, dim3(tiles_c * tiles_p, R), dim3(256), 0, (hipStream_t)stream, a, mask, scale,
                     (const float*)nullptr, PCG_ACT_NONE, 0.f, HW, C, tiles_c, out);
  return launch_status("drop2d_flatten_kernel<fwd>");
}

// The backward of the above and of the activation in front of it (classifier.py:13-17 under trainer.py:20):
// out[b][p][c] = dflat[b][c * HW + p] * mask[b][c] * scale * act'(y[b][p][c]).
extern "C" int pcg_drop2d_flatten_bwd(const float* dflat, const float* mask, float scale, const float* y, int act, float slope, int32_t R,
                                      int32_t HW, int32_t C, float* out, pcg_stream_t stream) {
  PCG_REQUIRE(dflat && mask && y && out && dflat != out && R > 0 && R <= 65535 && HW > 0 && C > 0, "pcg_drop2d_flatten_bwd: bad arguments");
  const int tiles_c = (C + 31) / 32, tiles_p = (HW + 31) / 32;
  hipLaunchKernelGGL(drop2d_flatten_kernel<true>, dim3(tiles_c * tiles_p, R), dim3(256), 0, (hipStream_t)stream, dflat, mask, scale, y, act,
                     slope, HW, C, tiles_c, out);
  return launch_status("drop2d_flatten_kernel<bwd>");
}

// Dropout(0.5), fc2, CrossEntropyLoss and their backward down to fc1's pre-activation (classifier.py:19-21, trainer.py:10,19-20) in one
// launch of one workgroup; tally (float64[3]) += (loss * R, rows whose argmax is the label, R).
extern "C" int pcg_mnist_clf_head(const float* h, const float* m1, float scale, const float* W2, const float* b2, const int64_t* y, int32_t R,
                                  int32_t I, int32_t K, float* logits, float* loss, double* tally, float* dW2, float* db2, float* dh, float* db1,
                                  pcg_stream_t stream) {
  PCG_REQUIRE(h && m1 && W2 && b2 && y && logits && loss && tally && dW2 && db2 && dh && db1, "pcg_mnist_clf_head: null argument");
  PCG_REQUIRE(R >= 1 && R <= MH_ROWS, "pcg_mnist_clf_head: %d rows; one workgroup holds 1..%d", R, MH_ROWS);
  PCG_REQUIRE(I == MH_I, "pcg_mnist_clf_head: %d inputs; the kernel is built for %d", I, MH_I);
  PCG_REQUIRE(K >= 1 && K <= MH_K, "pcg_mnist_clf_head: %d classes; one MFMA tile holds 1..%d", K, MH_K);
  PCG_REQUIRE((((uintptr_t)h | (uintptr_t)m1) & 15) == 0, "pcg_mnist_clf_head: h and m1 must be 16-byte aligned");
  const MhArgs args{h, m1, scale, W2, b2, y, R, K, logits, loss, tally, dW2, db2, dh, db1};
  hipLaunchKernelGGL(mnist_clf_head_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, args);
  return launch_status("mnist_clf_head_kernel");
}
