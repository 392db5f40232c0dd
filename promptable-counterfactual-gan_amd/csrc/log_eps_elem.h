// log_eps_elem.h — the per-row element and the row sum of the log-eps GAN losses of conditional_counteRGAN/mnist/countergan2.py:188,198.
// ONE definition for pcg_prob_head_fwd's finishing workgroup and for pcg_log_eps_loss_fwd_bwd (csrc/prob_head.hip): fed the same
// probabilities, both form the same loss bits.
#pragma once
#include "pcg_common.h"

namespace pcg {

// One row's loss term and its derivative with respect to the probability d:
//   real (:188 d_real, :198 d_fake):  term = log(d + eps),         dterm = 1 / (d + eps)
//   fake (:188 d_fake):               term = log((1 - d) + eps),   dterm = -1 / ((1 - d) + eps)     left to right, as `1 - d_fake + 1e-6`
__device__ __forceinline__ void log_eps_elem(float d, bool fake, float eps, float& term, float& dterm) {
#pragma clang fp contract(off)
  const float u = fake ? (1.f - d) + eps : d + eps;
  term = logf(u);
  dterm = fake ? -1.f / u : 1.f / u;
}

// d loss / d d of one row: the loss is -(1/n) * sum of terms
__device__ __forceinline__ float log_eps_dp(float d, bool fake, float eps, float inv_n) {
#pragma clang fp contract(off)
  float term, dterm;
  log_eps_elem(d, fake, eps, term, dterm);
  return -inv_n * dterm;
}

// The sum of the terms over the rows, in the order both kernels share: thread t takes b = t, t + 256, ... below n (mode D: n = R/2 and
// the term of b is log(p[b] + eps) + log((1 - p[n + b]) + eps), the reference's own pairing; mode G: n = R), then the 256-wide tree.
// Called by all 256 threads of one workgroup; red: 256 floats of LDS.  Returns -(1/n) * sum in every thread.
__device__ __forceinline__ float log_eps_loss_rows(const float* p, int R, bool mode_d, float eps, float* red) {
#pragma clang fp contract(off)
  const int n = mode_d ? R / 2 : R;
  float acc = 0.f;
  for (int b = threadIdx.x; b < n; b += 256) {
    float t0, t1, unused;
    log_eps_elem(p[b], false, eps, t0, unused);
    if (mode_d) {
      log_eps_elem(p[n + b], true, eps, t1, unused);
      t0 = t0 + t1;
    }
    acc += t0;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  const float s = red[0];
  __syncthreads();
  return -(1.f / (float)n) * s;
}

}  // namespace pcg
