// prob_head.hip — the head of the full-resolution discriminator of conditional_counteRGAN/mnist/countergan2.py:76-93 and the log-eps
// losses of its training loop (:188, :198); DESIGN.md §3.21.  All fp32, every sum in an order fixed by the data and the arguments, no
// floating-point atomics, no grid barrier; every entry takes a stream and can be captured.
//
//   pcg_prob_head_fwd          Flatten + Linear(F -> 1) + Sigmoid, both log-eps losses, their gradient with respect to the logit and the
//                              bias gradient; one workgroup per (row, column slab)
//   pcg_log_eps_loss_fwd_bwd   the same loss on given probabilities, for the op chain (one workgroup)
//
// The head's backward is pcg_logit_head_bwd (delta_gan.hip) as it is.  The arrival protocol is logit_head_fwd_kernel's (delta_gan.hip):
// thread 0 publishes the workgroup's value with an agent-scope store, waits for it, takes a ticket; the workgroup that draws the last
// ticket re-arms the counter and reads every value back with agent-scope loads.  Those few helpers are restated here so that
// delta_gan.hip's code object stays what it was.
#include "log_eps_elem.h"

namespace pcg {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int NT = 256;
constexpr int WS_HEAD = 16;                     // bytes in front of the partials: the ticket
constexpr int MAX_SLABS = PCG_PROB_HEAD_MAX_SLABS;

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

__device__ __forceinline__ void publish(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float collect(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ bool last_ticket(int* ticket, int n) {
  __builtin_amdgcn_s_waitcnt(0);
  const int t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (t != n - 1) return false;
  __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

__device__ __forceinline__ float block_tree_256(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int k = NT / 2; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  const float s = red[0];
  __syncthreads();
  return s;
}

__device__ __forceinline__ float fold4(f32x4 av, f32x4 wv, float acc) {
#pragma unroll
  for (int j = 0; j < 4; ++j) acc = fmaf(av[j], wv[j], acc);
  return acc;
}

// ---- head forward: workgroup (r, s) folds slab s of row r; the last workgroup to arrive finishes every row -------------------------------
__global__ void __launch_bounds__(NT) prob_head_fwd_kernel(pcg_prob_head_fwd_args a, int slabs, int per) {
  __shared__ float redf[NT];
  __shared__ int s_last;
  const int r = blockIdx.x / slabs, s = blockIdx.x - r * slabs;
  const int R = a.R, F4 = a.F >> 2;
  const int q0 = min(s * per, F4), q1 = min(q0 + per, F4);              // an empty slab: q0 == q1, the tree of zeros is +0
  const f32x4* __restrict__ row = reinterpret_cast<const f32x4*>(a.a + (size_t)r * a.F);
  const f32x4* __restrict__ w4 = reinterpret_cast<const f32x4*>(a.w);
  int* ticket = reinterpret_cast<int*>(a.workspace);
  float* partial = reinterpret_cast<float*>(reinterpret_cast<char*>(a.workspace) + WS_HEAD);
  float acc = 0.f;
  int q = q0 + (int)threadIdx.x;
  for (; q + 3 * NT < q1; q += 4 * NT) {                                 // four groups in flight; folded in index order all the same
    const f32x4 a0 = row[q], a1 = row[q + NT], a2 = row[q + 2 * NT], a3 = row[q + 3 * NT];
    const f32x4 w0 = w4[q], w1 = w4[q + NT], w2 = w4[q + 2 * NT], w3 = w4[q + 3 * NT];
    acc = fold4(a3, w3, fold4(a2, w2, fold4(a1, w1, fold4(a0, w0, acc))));
  }
  for (; q < q1; q += NT) acc = fold4(row[q], w4[q], acc);
  const float dot = block_tree_256(acc, redf);
  if (threadIdx.x == 0) {
    publish(partial + blockIdx.x, dot);
    s_last = last_ticket(ticket, (int)gridDim.x) ? 1 : 0;
  }
  __syncthreads();
  if (!s_last) return;
  const bool mode_d = a.mode == PCG_PROB_HEAD_D;
  const int half = mode_d ? R / 2 : R;                                   // rows of the real kind
  const float inv = 1.f / (float)half, bias = a.bias[0];
  float sb = 0.f;
  for (int i = threadIdx.x; i < R; i += NT) {
#pragma clang fp contract(off)
    float* pr = partial + (size_t)i * slabs;
    float z = collect(pr);
    publish(pr, 0.f);                                                    // the workspace is left zero
    for (int k = 1; k < slabs; ++k) {
      z += collect(pr + k);
      publish(pr + k, 0.f);
    }
    z += bias;
    const float d = act_apply(z, PCG_ACT_SIGMOID, 0.f);                  // pcg_act_fwd's expression
    const float dl = log_eps_dp(d, i >= half, a.eps, inv) * act_grad_from_out(d, PCG_ACT_SIGMOID, 0.f);
    a.logits[i] = z;
    a.prob[i] = d;
    a.dlogit[i] = dl;
    sb += dl;
  }
  const float sd = block_tree_256(sb, redf);                             // its barriers also make prob visible to the whole workgroup
  const float loss = log_eps_loss_rows(a.prob, R, mode_d, a.eps, redf);
  if (threadIdx.x == 0) {
    a.loss[0] = loss;
    a.db[0] = sd;
  }
}

// ---- the loss alone: one workgroup ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NT) log_eps_loss_kernel(pcg_log_eps_loss_args a) {
  __shared__ float redf[NT];
  const bool mode_d = a.mode == PCG_PROB_HEAD_D;
  const float loss = log_eps_loss_rows(a.p, a.R, mode_d, a.eps, redf);
  if (threadIdx.x == 0 && a.loss) a.loss[0] = loss;
  if (!a.dp) return;
  const int half = mode_d ? a.R / 2 : a.R;
  const float inv = 1.f / (float)half, g = a.grad_out ? a.grad_out[0] : 1.f;
  for (int i = threadIdx.x; i < a.R; i += NT) {
    const float dp = log_eps_dp(a.p[i], i >= half, a.eps, inv);
    a.dp[i] = a.grad_out ? dp * g : dp;
  }
}

// the library's slab count for R rows (pcgan_hip.h states the rule and where it was measured)
int default_slabs(int R) { return R <= 128 ? 2 : 1; }

bool rows_ok(int R, int slabs) { return R >= 1 && R <= 65535 && slabs >= 0 && slabs <= MAX_SLABS; }

}  // namespace
}  // namespace pcg

using namespace pcg;

extern "C" size_t pcg_prob_head_workspace_bytes(int32_t R, int32_t slabs) {
  if (!rows_ok(R, slabs)) return 0;
  return WS_HEAD + (size_t)R * (slabs ? slabs : default_slabs(R)) * sizeof(float);
}

extern "C" int pcg_prob_head_fwd(const pcg_prob_head_fwd_args* args, pcg_stream_t stream) {
  PCG_REQUIRE(args, "pcg_prob_head_fwd: null arguments");
  const pcg_prob_head_fwd_args& a = *args;
  PCG_REQUIRE(a.mode == PCG_PROB_HEAD_D || a.mode == PCG_PROB_HEAD_G, "pcg_prob_head_fwd: mode %d", a.mode);
  PCG_REQUIRE(a.R >= 1 && a.R <= 65535, "pcg_prob_head_fwd: %d rows (1..65535)", a.R);
  PCG_REQUIRE(a.mode != PCG_PROB_HEAD_D || a.R % 2 == 0, "pcg_prob_head_fwd: mode D takes real and fake halves; %d rows are odd", a.R);
  PCG_REQUIRE(a.F >= 4 && a.F % 4 == 0, "pcg_prob_head_fwd: F %d (a multiple of 4)", a.F);
  PCG_REQUIRE(a.slabs >= 0 && a.slabs <= MAX_SLABS, "pcg_prob_head_fwd: slabs %d (0: the library's choice, or 1..%d)", a.slabs, MAX_SLABS);
  PCG_REQUIRE(a.eps > 0.f && a.eps < 1.f, "pcg_prob_head_fwd: eps %g (0 < eps < 1)", (double)a.eps);
  PCG_REQUIRE(a.a && a.w && a.bias && a.logits && a.prob && a.loss && a.dlogit && a.db && a.workspace,
              "pcg_prob_head_fwd: null a, w, bias, logits, prob, loss, dlogit, db or workspace");
  PCG_REQUIRE(aligned(a.a, 16) && aligned(a.w, 16) && aligned(a.workspace, 4),
              "pcg_prob_head_fwd: a and w are read 16 bytes at a time; a pointer is not aligned");
  const int slabs = a.slabs ? a.slabs : default_slabs(a.R);
  const size_t need = WS_HEAD + (size_t)a.R * slabs * sizeof(float);
  if (a.workspace_bytes < need) {
    set_error("pcg_prob_head_fwd: workspace of %zu bytes, %zu needed", a.workspace_bytes, need);
    return PCG_ERR_WORKSPACE;
  }
  const int per = ceil_div(a.F / 4, slabs);
  hipLaunchKernelGGL(prob_head_fwd_kernel, dim3((unsigned)(a.R * slabs)), dim3(NT), 0, (hipStream_t)stream, a, slabs, per);
  return launch_status("prob_head_fwd_kernel");
}

extern "C" int pcg_log_eps_loss_fwd_bwd(const pcg_log_eps_loss_args* args, pcg_stream_t stream) {
  PCG_REQUIRE(args, "pcg_log_eps_loss_fwd_bwd: null arguments");
  const pcg_log_eps_loss_args& a = *args;
  PCG_REQUIRE(a.mode == PCG_PROB_HEAD_D || a.mode == PCG_PROB_HEAD_G, "pcg_log_eps_loss_fwd_bwd: mode %d", a.mode);
  PCG_REQUIRE(a.R >= 1 && a.R <= 65535, "pcg_log_eps_loss_fwd_bwd: %d rows (1..65535)", a.R);
  PCG_REQUIRE(a.mode != PCG_PROB_HEAD_D || a.R % 2 == 0, "pcg_log_eps_loss_fwd_bwd: mode D takes real and fake halves; %d rows are odd", a.R);
  PCG_REQUIRE(a.eps > 0.f && a.eps < 1.f, "pcg_log_eps_loss_fwd_bwd: eps %g (0 < eps < 1)", (double)a.eps);
  PCG_REQUIRE(a.p && (a.loss || a.dp), "pcg_log_eps_loss_fwd_bwd: null p, or neither loss nor dp asked for");
  PCG_REQUIRE(a.p != a.dp, "pcg_log_eps_loss_fwd_bwd: dp is written out of place");
  hipLaunchKernelGGL(log_eps_loss_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, a);
  return launch_status("log_eps_loss_kernel");
}
