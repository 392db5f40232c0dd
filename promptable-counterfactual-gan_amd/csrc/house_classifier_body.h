// house_classifier_body.h — the device body of the frozen tabular classifier that more than one translation unit runs: the tile
// constants, the dense forward layer on v_mfma_f32_16x16x4_f32 and the LDS image.  house_classifier_fused.hip (whose header comment
// describes the layout) builds the training step's launches from it, house_cf_eval.hip the evaluation launch.
#pragma once
#include <cstdint>
#include "pcg_common.h"

namespace pcg {
namespace {

constexpr int CL_R = 16;                 // rows per block: 4096 rows are 256 blocks, one per CU (32-row tiles left half the chip idle
                                         // and each CU MFMA-bound: 128 blocks x 1024 MFMAs for the 256 -> 256 layer alone)
constexpr int CL_P = CL_R + 1;           // LDS pitch of a k-row
constexpr int CL_W = 256;                // widest layer
constexpr int CL_IN = 17, CL_INP = 20;   // input width, padded to a multiple of the MFMA's reduction depth (4)
constexpr int CL_H1 = 256, CL_H2 = 256, CL_H3 = 128, CL_H4 = 64, CL_OUT = 4;
constexpr float CL_SLOPE = 0.1f;
constexpr int CL_NW = 8, CL_NT = CL_NW * 64;     // waves / threads per block
typedef float cl_acc_t __attribute__((ext_vector_type(4)));

struct ClsFwdW { const float* wt[5]; const float* b[5]; };   // wt[l]: [K_l (padded)][N_l] k-major; layer 4 (64 -> 4): as stored [4][64]

// v_mfma_f32_16x16x4_f32: lane (li = lane % 16, lq = lane / 16) supplies A[m = li][k = lq] and B[k = lq][n = li]; accumulator
// register r holds D[m = 4 lq + r][n = li].
//
// One dense layer: Y[16 rows][N] = act(X[16][K] Wt[K][N] + bias), X / Y k-major in LDS.  The eight waves take the N / 16 column
// tiles; a layer with fewer tiles than waves splits its reduction instead (KS waves per tile, a contiguous share of K each) and the
// partial tiles are added in share order through LDS.  G MFMA steps (4 G reduction indices) form a group whose B operands are
// prefetched two groups ahead.  Contains block barriers in the split form: all waves call it.
template <int K, int N, bool LEAKY>
__device__ __forceinline__ void cl_dense_fwd(const float* __restrict__ Xin, float* __restrict__ Xout, const float* __restrict__ Wt,
                                             const float* __restrict__ bias, float* __restrict__ gsave, float* part, size_t row0, int rows,
                                             int wave, int li, int lq) {
  constexpr int NT = N / 16, TPW = NT >= CL_NW ? NT / CL_NW : 1, KS = NT >= CL_NW ? 1 : CL_NW / NT;
  constexpr int KW = K / KS, STEPS = KW / 4, G = STEPS % 16 == 0 ? 16 : STEPS, NG = STEPS / G;
  static_assert(N % 16 == 0 && K % (4 * KS) == 0 && STEPS % G == 0 && (NT >= CL_NW ? NT % CL_NW == 0 : CL_NW % NT == 0), "tile shapes");
  const int tile0 = KS == 1 ? wave * TPW : wave % NT, ks = KS == 1 ? 0 : wave / NT;
  const int n0 = tile0 * 16, kb = ks * KW;
  cl_acc_t acc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const float bv = KS == 1 ? bias[n0 + t * 16 + li] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[t][r] = bv;
  }
  float bcur[TPW][G], bnxt[TPW][G], bnx2[TPW][G];
  const float* wp = Wt + (size_t)(kb + lq) * N + n0 + li;
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int g = 0; g < G; ++g) {
      bcur[t][g] = wp[(size_t)(4 * g) * N + t * 16];
      bnxt[t][g] = NG > 1 ? wp[(size_t)(4 * G + 4 * g) * N + t * 16] : 0.f;
    }
#pragma unroll 1
  for (int grp = 0; grp < NG; ++grp) {
    const int k0 = grp * 4 * G;
    if (grp + 2 < NG) {
#pragma unroll
      for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int g = 0; g < G; ++g) bnx2[t][g] = wp[(size_t)(k0 + 8 * G + 4 * g) * N + t * 16];
    }
    float a[G];
#pragma unroll
    for (int g = 0; g < G; ++g) a[g] = Xin[(kb + k0 + 4 * g + lq) * CL_P + li];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int t = 0; t < TPW; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g], bcur[t][g], acc[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
      for (int g = 0; g < G; ++g) { bcur[t][g] = bnxt[t][g]; bnxt[t][g] = bnx2[t][g]; }
  }
  if (KS == 1) {
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 4 * lq + r, n = n0 + t * 16 + li;
        float v = acc[t][r];
        if (LEAKY) v = v > 0.f ? v : v * CL_SLOPE;
        Xout[n * CL_P + m] = v;
        if (gsave && m < rows) gsave[(row0 + m) * N + n] = v;
      }
    return;
  }
  // split reduction: partial tiles [wave][column in tile][row] -> LDS, then every thread finishes N * 16 / 512 outputs (column
  // fastest: coalesced global rows, conflict-free LDS)
#pragma unroll
  for (int r = 0; r < 4; ++r) part[wave * (16 * CL_P) + li * CL_P + 4 * lq + r] = acc[0][r];
  __syncthreads();
#pragma unroll
  for (int tt = 0; tt < N * CL_R / CL_NT; ++tt) {
    const int e = threadIdx.x + tt * CL_NT;
    const int m = e / N, n = e - m * N, t = n >> 4, nl = n & 15;
    float v = bias[n];
#pragma unroll
    for (int q = 0; q < KS; ++q) v += part[(q * NT + t) * (16 * CL_P) + nl * CL_P + m];
    if (LEAKY) v = v > 0.f ? v : v * CL_SLOPE;
    Xout[n * CL_P + m] = v;
    if (gsave && m < rows) gsave[(row0 + m) * N + n] = v;
  }
}

struct alignas(16) ClsSmem {
  float X[2][CL_W * CL_P];                 // activation ping-pong, k-major
  float part[CL_NW * CL_R * CL_P];         // partial tiles of the split reductions, [wave][column][row]
};

}  // namespace
}  // namespace pcg
