// launch_plan.h — what pcg_launch_plan_describe (tabular.hip) shares with the launchers of tabular.hip, cf_ops.hip, pointwise.hip,
// batchnorm.hip and instnorm.hip:
// the grid of an element-wise launch, and each file's describe piece.  A launcher and the describe entry call the SAME host predicate
// for every decision (rowdot_takes, skinny_takes, abs_mean_one_block, ce_threads, embed_bwd_splits_batch, ...), so the text cannot
// drift from what is launched.  Decisions a kernel takes itself are shared too: the float4 rows of cross_entropy_kernel are a macro both
// expand, the LDS-image / one-burst forms of the spectral-norm bodies are constexpr predicates (spectral_norm_body.h).  The normalisation
// layer's pieces: plan_cols / plan_apply / plan_presum / fin_threads (batchnorm.hip) and instnorm_plan (instnorm.hip).
#pragma once
#include <cstdio>
#include "pcg_common.h"

namespace pcg {

// grid of a grid-stride element-wise launch: one thread per work item in blocks of 256, at most max_blocks blocks
inline unsigned ew_grid(size_t n, unsigned max_blocks) {
  size_t b = (n + 255) / 256;
  if (b > max_blocks) b = max_blocks;
  if (b < 1) b = 1;
  return (unsigned)b;
}
inline void describe_ew_grid(char* buf, size_t bytes, size_t n, unsigned blocks) {
  const size_t per_pass = (size_t)blocks * 256;
  const size_t passes = (n + per_pass - 1) / per_pass;
  snprintf(buf, bytes, "%u %s of 256: %zu %s", blocks, blocks == 1 ? "block" : "blocks", passes, passes == 1 ? "pass" : "passes");
}

// a describe piece returns PCG_PLAN_NOT_MINE for an op (or element-wise family) of another file
constexpr int PCG_PLAN_NOT_MINE = 1;
int describe_cf_ops_plan(int32_t op, const int64_t* args, int32_t n_args, char* buf, size_t bytes);
int describe_pointwise_plan(int32_t op, const int64_t* args, int32_t n_args, char* buf, size_t bytes);
int describe_batchnorm_plan(int32_t op, const int64_t* args, int32_t n_args, char* buf, size_t bytes);
int describe_instnorm_plan(int32_t op, const int64_t* args, int32_t n_args, char* buf, size_t bytes);

}  // namespace pcg
