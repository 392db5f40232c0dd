// softmax_label.h — the probability softmax(lg[0..K))[y] of ONE class of a row of logits, fp32, max-subtracted: the running maximum,
// then e_k = expf(lg[k] - max) added in class order, then e_y / sum.  ONE definition for the score kernel of the prompted MNIST queries
// (mnist_cf_eval.hip: the classifier's probability of a row's own label) and for the per-class source pick (cf_report.hip): both must give
// the same bits for the same row, because the pick is tested against the score kernel's p_true exactly.  A y outside [0, K) gives 0.
#pragma once
#include <hip/hip_runtime.h>

namespace pcg {

__device__ __forceinline__ float softmax_prob_at(const float* lg, int K, int y) {
  float mx = lg[0];
  for (int k = 1; k < K; ++k) mx = fmaxf(mx, lg[k]);
  float den = 0.f, e_y = 0.f;
  for (int k = 0; k < K; ++k) {
    const float e = expf(lg[k] - mx);
    den += e;
    if (k == y) e_y = e;
  }
  return e_y / den;
}

}  // namespace pcg
