// delta_cf_eval.hip — the prompted half of the additive-delta MNIST CounteRGAN (conditional_counteRGAN/mnist/gan_train_copy.py on
// modules/generator.py): the launches around the generator's convolutions when ONE pass carries a window of
// (target class, row) queries, and the per-iteration class draw of the random-target training loop.
//   pcg_delta_cf_entry          the generator's 2-channel NHWC input (x[b], table[target(q)]) with the broadcast done by indexing
//                               (modules/generator.py:19-20 at gan_train_copy.py:165)
//   pcg_delta_cf_tail           delta -> the clamped counterfactual (:165-166) and three continuous per-query sums
//   pcg_delta_gan_target_draw   ONE class for the whole batch (:119-120), its Philox offset by value or from a device counter that the
//                               launch advances (a replayed graph then draws the next class of the stream)
// A query is q = t * B + b (target-major), as in mnist_cf_eval.hip; entry and tail work on a window [q0, q0 + nq) and index their
// per-query tensors relative to q0.  x is never replicated.  Scoring is pcg_mnist_cf_score, unchanged: the tail's sums have its
// tail_sums layout.  fp32, wave64, no atomics; every sum has one order fixed by the shapes alone.
#include <cstdint>
#include "pcg_common.h"
#include "philox.h"

namespace pcg {
namespace {

using f32x2 = __attribute__((ext_vector_type(2))) float;
constexpr int NT = 256, WAVE = 64;

unsigned blocks_for(size_t n) {
  size_t b = (n + NT - 1) / NT;
  if (b > 16384) b = 16384;
  if (b < 1) b = 1;
  return (unsigned)b;
}

// ---- generator input: out[q - q0][p] = (x[b][p], table[target(q)][p]), one 8-byte store per (query, pixel) ------------------------------
__global__ void __launch_bounds__(NT) delta_cf_entry_kernel(const pcg_delta_cf_entry_args a) {
  const int HW = a.HW;
  const size_t n = (size_t)a.nq * HW;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
    const int r = (int)(i / HW), p = (int)(i - (size_t)r * HW);
    const int q = a.q0 + r, t = q / a.B, b = q - t * a.B;
    int64_t k = a.target ? a.target[b] : (int64_t)t;
    k = k < 0 ? 0 : (k >= a.K ? a.K - 1 : k);               // as embed_concat_fwd_kernel: never read outside the table
    *reinterpret_cast<f32x2*>(a.out + i * 2) = f32x2{a.x[(size_t)b * HW + p], a.table[(size_t)k * HW + p]};
  }
}

// ---- tail: one wave per query, float4 per lane, the three sums reduced across the wave by a fixed butterfly -----------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}

// torch.clamp(v, -1, 1): a NaN fails both comparisons and is returned as it is
__device__ __forceinline__ float clamp1(float v) { return v < -1.f ? -1.f : (v > 1.f ? 1.f : v); }

__global__ void __launch_bounds__(NT) delta_cf_tail_kernel(const pcg_delta_cf_tail_args a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int r = blockIdx.x * (NT / WAVE) + (threadIdx.x >> 6);
  if (r >= a.nq) return;                                     // whole waves leave: there is no block-wide barrier below
  const int q = a.q0 + r, t = q / a.B, b = q - t * a.B, n4 = a.HW >> 2;
  const float4* d4 = reinterpret_cast<const float4*>(a.delta + (size_t)r * a.HW);
  const float4* x4 = reinterpret_cast<const float4*>(a.x + (size_t)b * a.HW);
  float4* o4 = reinterpret_cast<float4*>(a.x_cf + (size_t)r * a.HW);
  float s_act = 0.f, s_abs = 0.f, s_sq = 0.f;
  for (int i = lane; i < n4; i += WAVE) {
    const float4 d = d4[i], x = x4[i];
    float4 y;
    // the sum is rounded, then clamped, as the reference's two statements (gan_train_copy.py:165-166); every term rounded on its own
#define PCG_TAIL(e)                                                                  \
    {                                                                                \
      y.e = clamp1(__fadd_rn(x.e, d.e));                                             \
      const float c = __fsub_rn(y.e, x.e);                                           \
      s_act = __fadd_rn(s_act, fabsf(c));                                            \
      s_abs = __fadd_rn(s_abs, fabsf(d.e));                                          \
      s_sq = __fadd_rn(s_sq, __fmul_rn(c, c));                                       \
    }
    PCG_TAIL(x) PCG_TAIL(y) PCG_TAIL(z) PCG_TAIL(w)
#undef PCG_TAIL
    o4[i] = y;
  }
  s_act = wave_sum(s_act); s_abs = wave_sum(s_abs); s_sq = wave_sum(s_sq);
  if (lane == 0) {
    float* s = a.sums + (size_t)r * 3;
    s[0] = s_act; s[1] = s_abs; s[2] = s_sq;
  }
}

// ---- the iteration's one class: every thread reads the offset, a barrier, thread 0 writes the increment --------------------------------
__global__ void __launch_bounds__(NT) delta_gan_target_draw_kernel(const pcg_delta_gan_target_draw_args a) {
  unsigned long long* ctr = reinterpret_cast<unsigned long long*>(a.counter);
  const uint64_t off = ctr ? (uint64_t)ctr[0] : a.offset;   // kernel-uniform
  const U4 r = draw(a.seed, off, 0);                         // randint_quad's element 0 of quad 0 with lo = 0, hi = K
  const int64_t k = (int64_t)(((uint64_t)r.x * (uint64_t)(uint32_t)a.K) >> 32);
  for (int b = threadIdx.x; b < a.B; b += NT) a.target[b] = k;
  if (ctr) {
    __syncthreads();                                         // every thread of the one workgroup has read the counter
    if (threadIdx.x == 0) ctr[0] = off + 1ull;               // (1 + 3) / 4 counter values: DeviceRNG.randint(.., n = 1)'s span
  }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
bool window_ok(int B, int T, int q0, int nq) { return B >= 1 && T >= 1 && q0 >= 0 && nq >= 1 && (int64_t)q0 + nq <= (int64_t)T * B; }

}  // namespace
}  // namespace pcg

using namespace pcg;

extern "C" int pcg_delta_cf_entry(const pcg_delta_cf_entry_args* args, pcg_stream_t stream) {
  PCG_REQUIRE(args, "pcg_delta_cf_entry: null arguments");
  const pcg_delta_cf_entry_args& a = *args;
  PCG_REQUIRE(a.x && a.table && a.out, "pcg_delta_cf_entry: null x, table or out");
  PCG_REQUIRE(a.HW >= 4 && a.HW % 4 == 0 && a.K >= 1 && window_ok(a.B, a.T, a.q0, a.nq),
              "pcg_delta_cf_entry: HW %d (a multiple of 4), K %d, window [%d, +%d) of %d x %d queries", a.HW, a.K, a.q0, a.nq, a.T, a.B);
  PCG_REQUIRE((int64_t)a.B * a.HW <= (int64_t)INT32_MAX && (int64_t)a.nq * a.HW * 2 <= (int64_t)INT32_MAX,
              "pcg_delta_cf_entry: %d rows or %d queries of %d pixels exceed the index range", a.B, a.nq, a.HW);
  PCG_REQUIRE(a.target ? a.T == 1 : a.T <= a.K, "pcg_delta_cf_entry: the per-row form (target [B]) takes T = 1, the sweep T <= K (T %d, K %d)", a.T,
              a.K);
  PCG_REQUIRE(!a.target_host || a.target, "pcg_delta_cf_entry: target_host is the host copy of target; target is null");
  PCG_REQUIRE(aligned(a.out, 8), "pcg_delta_cf_entry: out is written 8 bytes at a time; the pointer is not aligned");
  if (a.target_host)
    for (int b = 0; b < a.B; ++b)
      PCG_REQUIRE(a.target_host[b] >= 0 && a.target_host[b] < a.K, "pcg_delta_cf_entry: label %lld of row %d (target) is outside 0..%d",
                  (long long)a.target_host[b], b, a.K - 1);
  hipLaunchKernelGGL(delta_cf_entry_kernel, dim3(blocks_for((size_t)a.nq * a.HW)), dim3(NT), 0, (hipStream_t)stream, a);
  return launch_status("delta_cf_entry_kernel");
}

extern "C" int pcg_delta_cf_tail(const pcg_delta_cf_tail_args* args, pcg_stream_t stream) {
  PCG_REQUIRE(args, "pcg_delta_cf_tail: null arguments");
  const pcg_delta_cf_tail_args& a = *args;
  PCG_REQUIRE(a.delta && a.x && a.x_cf && a.sums, "pcg_delta_cf_tail: null delta, x, x_cf or sums");
  PCG_REQUIRE(a.HW >= 4 && a.HW % 4 == 0 && window_ok(a.B, a.T, a.q0, a.nq),
              "pcg_delta_cf_tail: HW %d (a multiple of 4), window [%d, +%d) of %d x %d queries", a.HW, a.q0, a.nq, a.T, a.B);
  PCG_REQUIRE((int64_t)a.B * a.HW <= (int64_t)INT32_MAX && (int64_t)a.nq * a.HW <= (int64_t)INT32_MAX,
              "pcg_delta_cf_tail: %d rows or %d queries of %d pixels exceed the index range", a.B, a.nq, a.HW);
  PCG_REQUIRE(aligned(a.delta, 16) && aligned(a.x, 16) && aligned(a.x_cf, 16),
              "pcg_delta_cf_tail: rows are read and written 16 bytes at a time; a pointer is not aligned");
  const int per = NT / WAVE;
  hipLaunchKernelGGL(delta_cf_tail_kernel, dim3((unsigned)((a.nq + per - 1) / per)), dim3(NT), 0, (hipStream_t)stream, a);
  return launch_status("delta_cf_tail_kernel");
}

extern "C" int pcg_delta_gan_target_draw(const pcg_delta_gan_target_draw_args* args, pcg_stream_t stream) {
  PCG_REQUIRE(args, "pcg_delta_gan_target_draw: null arguments");
  const pcg_delta_gan_target_draw_args& a = *args;
  PCG_REQUIRE(a.target, "pcg_delta_gan_target_draw: null target");
  PCG_REQUIRE(a.B >= 1 && a.K >= 1, "pcg_delta_gan_target_draw: batch of %d rows, %d classes", a.B, a.K);
  PCG_REQUIRE(aligned(a.counter, 8), "pcg_delta_gan_target_draw: the counter is read 8 bytes at a time; the pointer is not aligned");
  hipLaunchKernelGGL(delta_gan_target_draw_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, a);
  return launch_status("delta_gan_target_draw_kernel");
}
