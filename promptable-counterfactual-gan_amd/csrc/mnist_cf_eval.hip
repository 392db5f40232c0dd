// mnist_cf_eval.hip — the glue of the MNIST CounteRGAN's prompted queries and per-target evaluation:
// conditional_counteRGAN/mnist eval_utils.py:46-110 (evaluate_counterfactuals, evaluate_generator_per_target), :204-288
// (build_patch_mask_for_batch), :292-344 (compute_masked_metrics) and gradio_app.py:234-259 (one image, that digit, only these patches).
// The convolutions stay the library's (pcg_conv2d); these four kernels are what surrounds them when ONE generator pass carries
// every (target class, row) query of a loader batch:
//   patch_mask_bits   one 64-bit word per mask -> a dense [H][W] mask of whole patches
//   entry             the generator's NHWC input (x[b], table[target(q)], mask[row(q)]) with the broadcast done by indexing
//   tail              conv_out's result -> raw / masked residual, the clamped counterfactual and three per-query L1 sums
//   score             softmax / argmax of the classifier's logits per query and the per-(target, loader batch) group sums
// A query is q = t * B + b (target-major); every kernel works on a window [q0, q0 + nq) of the T * B queries and indexes its per-query
// inputs and outputs relative to q0.  x and the mask are never replicated.  fp32, wave64, no atomics; every sum has one fixed order.
#include <cstdint>
#include "pcg_common.h"
#include "softmax_label.h"

namespace pcg {
namespace {

constexpr int NT = 256, WAVE = 64;
constexpr int SCORE_KMAX = 16;            // classes the score kernel keeps in registers
constexpr int NSUM = PCG_MNIST_CF_GROUP_SUMS;

unsigned blocks_for(size_t n) {
  size_t b = (n + NT - 1) / NT;
  if (b > 16384) b = 16384;
  if (b < 1) b = 1;
  return (unsigned)b;
}

__device__ __forceinline__ size_t mask_row(int mode, int b, int q) { return mode == PCG_MASK_SHARED ? 0 : mode == PCG_MASK_PER_ROW ? b : q; }

// ---- patch bits -> dense masks (create_mask_from_indices, eval_utils.py:247-256) ------------------------------------------------
__global__ void __launch_bounds__(NT) patch_mask_bits_kernel(const pcg_patch_mask_bits_args a) {
  const int HW = a.H * a.W, nph = a.H / a.ps, npw = a.W / a.ps;
  const size_t n = (size_t)a.n * HW;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
    const int m = (int)(i / HW), p = (int)(i - (size_t)m * HW);
    const int y = p / a.W, x = p - y * a.W, pi = y / a.ps, pj = x / a.ps;
    float v = 0.f;
    if (pi < nph && pj < npw) v = (float)((a.bits[m] >> (pi * npw + pj)) & 1ull);   // outside the patch grid: the border stays 0
    a.mask[i] = v;
  }
}

// ---- generator input: out[q - q0][p][0..2] = x[b][p], table[target(q)][p], mask[row(q)][p] ------------------------------------
__global__ void __launch_bounds__(NT) mnist_cf_entry_kernel(const pcg_mnist_cf_entry_args a) {
  const int HW = a.HW;
  const size_t n = (size_t)a.nq * HW;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
    const int r = (int)(i / HW), p = (int)(i - (size_t)r * HW);
    const int q = a.q0 + r, t = q / a.B, b = q - t * a.B;
    int64_t k = a.target ? a.target[b] : (int64_t)t;
    k = k < 0 ? 0 : (k >= a.K ? a.K - 1 : k);               // the host checks the range; never read outside the table
    float* o = a.out + i * 3;
    o[0] = a.x[(size_t)b * HW + p];
    o[1] = a.table[(size_t)k * HW + p];
    o[2] = a.mask[mask_row(a.mask_mode, b, q) * HW + p];
  }
}

// ---- tail: one wave per query, float4 per lane, the three sums reduced across the wave by a fixed butterfly ---------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}

__device__ __forceinline__ float clamp1(float v) { return fminf(fmaxf(v, -1.f), 1.f); }

__global__ void __launch_bounds__(NT) mnist_cf_tail_kernel(const pcg_mnist_cf_tail_args a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int r = blockIdx.x * (NT / WAVE) + (threadIdx.x >> 6);
  if (r >= a.nq) return;                                     // whole waves leave: no block-wide barrier below
  const int q = a.q0 + r, t = q / a.B, b = q - t * a.B, n4 = a.HW >> 2;
  const float4* c4 = reinterpret_cast<const float4*>(a.c + (size_t)r * a.HW);
  const float4* x4 = reinterpret_cast<const float4*>(a.x + (size_t)b * a.HW);
  const float4* m4 = reinterpret_cast<const float4*>(a.mask + mask_row(a.mask_mode, b, q) * a.HW);
  float4* o4 = reinterpret_cast<float4*>(a.x_cf + (size_t)r * a.HW);
  float4* raw4 = a.raw ? reinterpret_cast<float4*>(a.raw + (size_t)r * a.HW) : nullptr;
  float4* msk4 = a.masked ? reinterpret_cast<float4*>(a.masked + (size_t)r * a.HW) : nullptr;
  float s_act = 0.f, s_in = 0.f, s_out = 0.f;
  for (int i = lane; i < n4; i += WAVE) {
    const float4 c = c4[i], x = x4[i], m = m4[i];
    float4 raw, mk, y;
    // separately rounded products and sums, as the reference's three tensor expressions (generator.py:80,82, eval_utils.py:57)
#define PCG_TAIL(e)                                                                  \
    raw.e = __fmul_rn(c.e, a.scale);                                                 \
    mk.e = __fmul_rn(raw.e, m.e);                                                    \
    y.e = clamp1(__fadd_rn(x.e, mk.e));                                              \
    s_act += fabsf(__fsub_rn(y.e, x.e));                                             \
    s_in += fabsf(mk.e);                                                             \
    s_out += fabsf(__fmul_rn(raw.e, __fsub_rn(1.f, m.e)));
    PCG_TAIL(x) PCG_TAIL(y) PCG_TAIL(z) PCG_TAIL(w)
#undef PCG_TAIL
    o4[i] = y;
    if (raw4) raw4[i] = raw;
    if (msk4) msk4[i] = mk;
  }
  s_act = wave_sum(s_act); s_in = wave_sum(s_in); s_out = wave_sum(s_out);
  if (lane == 0) {
    float* s = a.sums + (size_t)r * 3;
    s[0] = s_act; s[1] = s_in; s[2] = s_out;
  }
}

// ---- score: one workgroup per (target slot t, loader batch j); a thread scores a row, threads 0..7 add the rows in index order ----
__global__ void __launch_bounds__(NT) mnist_cf_score_kernel(const pcg_mnist_cf_score_args a, int n_groups) {
  __shared__ float st[NSUM][NT];
  const int tid = threadIdx.x;
  const int t = blockIdx.x / n_groups, j = blockIdx.x - t * n_groups;
  int b0 = j * a.group_rows, b1 = b0 + a.group_rows < a.B ? b0 + a.group_rows : a.B;
  // the group's rows inside the window [q0, q0 + nq)
  const int lo = a.q0 - t * a.B, hi = a.q0 + a.nq - t * a.B;
  if (b0 < lo) b0 = lo;
  if (b1 > hi) b1 = hi;
  float acc = 0.f;                                           // thread k < NSUM: the running sum (k == 1: maximum) of statistic k
  for (int base = b0; base < b1; base += NT) {               // uniform trip count: the barriers are block-wide
    const int b = base + tid;
    float v[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; ++k) v[k] = 0.f;
    if (b < b1) {
      const int q = t * a.B + b, r = q - a.q0;
      const float* lg = a.logits_cf + (size_t)r * a.ld;
      float z[SCORE_KMAX];
      float mx = lg[0];
      int arg = 0;
#pragma unroll
      for (int k = 0; k < SCORE_KMAX; ++k) {
        z[k] = k < a.K ? lg[k] : 0.f;
        if (k > 0 && k < a.K && z[k] > mx) { mx = z[k]; arg = k; }   // strict: the first maximum, as torch.argmax
      }
      float den = 0.f;
#pragma unroll
      for (int k = 0; k < SCORE_KMAX; ++k)
        if (k < a.K) { z[k] = expf(z[k] - mx); den += z[k]; }
      int64_t tg = a.target ? a.target[b] : (int64_t)t;
      tg = tg < 0 ? 0 : (tg >= a.K ? a.K - 1 : tg);
      int64_t yt = a.y_true ? a.y_true[b] : -1;
      yt = yt >= a.K ? a.K - 1 : yt;
      float p_t = 0.f, p_y = 0.f;
#pragma unroll
      for (int k = 0; k < SCORE_KMAX; ++k) {                 // selects, not a dynamic register index
        if (k == (int)tg) p_t = z[k] / den;
        if (k == (int)yt) p_y = z[k] / den;
      }
      const float conf = 1.f / den;                          // exp(mx - mx) / den
      float p_o = 0.f;
      if (a.logits_orig && yt >= 0) p_o = softmax_prob_at(a.logits_orig + (size_t)b * a.ld, a.K, (int)yt);
      const float flip = arg == (int)tg ? 1.f : 0.f;
      if (a.pred) a.pred[r] = arg;
      if (a.conf) a.conf[r] = conf;
      if (a.p_target) a.p_target[r] = p_t;
      if (a.p_true) a.p_true[r] = p_y;
      if (a.p_orig_true) a.p_orig_true[r] = p_o;
      if (a.flip) a.flip[r] = flip;
      v[0] = flip; v[1] = flip;
      if (yt >= 0) { v[2] = p_t - p_y; v[3] = a.logits_orig ? p_t - p_o : 0.f; }
      if (a.tail_sums) { v[4] = a.tail_sums[(size_t)r * 3]; v[5] = a.tail_sums[(size_t)r * 3 + 1]; v[6] = a.tail_sums[(size_t)r * 3 + 2]; }
      v[7] = 1.f;
    }
    if (a.group_sums) {
#pragma unroll
      for (int k = 0; k < NSUM; ++k) st[k][tid] = v[k];
      __syncthreads();
      if (tid < NSUM) {
        const int n = b1 - base < NT ? b1 - base : NT;
        if (tid == 1) for (int i = 0; i < n; ++i) acc = fmaxf(acc, st[1][i]);
        else for (int i = 0; i < n; ++i) acc += st[tid][i];
      }
      __syncthreads();
    }
  }
  if (a.group_sums && tid < NSUM) a.group_sums[((size_t)t * n_groups + j) * NSUM + tid] = acc;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
bool window_ok(int B, int T, int q0, int nq) { return B >= 1 && T >= 1 && q0 >= 0 && nq >= 1 && (int64_t)q0 + nq <= (int64_t)T * B; }
bool mode_ok(int m) { return m == PCG_MASK_SHARED || m == PCG_MASK_PER_ROW || m == PCG_MASK_PER_QUERY; }

}  // namespace
}  // namespace pcg

using namespace pcg;

extern "C" int pcg_patch_mask_bits(const pcg_patch_mask_bits_args* args, pcg_stream_t stream) {
  PCG_REQUIRE(args, "pcg_patch_mask_bits: null arguments");
  const pcg_patch_mask_bits_args& a = *args;
  PCG_REQUIRE(a.bits && a.mask && a.n >= 1 && a.H >= 1 && a.W >= 1, "pcg_patch_mask_bits: null bits or mask, or n %d, H %d, W %d", a.n, a.H, a.W);
  PCG_REQUIRE(a.ps >= 1 && a.ps <= a.H && a.ps <= a.W, "pcg_patch_mask_bits: patch size %d gives no patch on %d x %d", a.ps, a.H, a.W);
  PCG_REQUIRE((int64_t)(a.H / a.ps) * (a.W / a.ps) <= 64, "pcg_patch_mask_bits: %d x %d patches exceed the 64 bits of a word", a.H / a.ps,
              a.W / a.ps);
  PCG_REQUIRE((int64_t)a.n * a.H * a.W <= INT32_MAX, "pcg_patch_mask_bits: %d masks of %d x %d exceed the index range", a.n, a.H, a.W);
  hipLaunchKernelGGL(patch_mask_bits_kernel, dim3(blocks_for((size_t)a.n * a.H * a.W)), dim3(NT), 0, (hipStream_t)stream, a);
  return launch_status("patch_mask_bits_kernel");
}

extern "C" int pcg_mnist_cf_entry(const pcg_mnist_cf_entry_args* args, pcg_stream_t stream) {
  PCG_REQUIRE(args, "pcg_mnist_cf_entry: null arguments");
  const pcg_mnist_cf_entry_args& a = *args;
  PCG_REQUIRE(a.x && a.table && a.mask && a.out, "pcg_mnist_cf_entry: null x, table, mask or out");
  PCG_REQUIRE(a.HW >= 1 && a.K >= 1 && window_ok(a.B, a.T, a.q0, a.nq), "pcg_mnist_cf_entry: HW %d, K %d, window [%d, +%d) of %d x %d queries",
              a.HW, a.K, a.q0, a.nq, a.T, a.B);
  PCG_REQUIRE(mode_ok(a.mask_mode), "pcg_mnist_cf_entry: mask mode %d", a.mask_mode);
  PCG_REQUIRE(a.target ? a.T == 1 : a.T <= a.K, "pcg_mnist_cf_entry: the per-row form (target [B]) takes T = 1, the sweep T <= K (T %d, K %d)", a.T,
              a.K);
  hipLaunchKernelGGL(mnist_cf_entry_kernel, dim3(blocks_for((size_t)a.nq * a.HW)), dim3(NT), 0, (hipStream_t)stream, a);
  return launch_status("mnist_cf_entry_kernel");
}

extern "C" int pcg_mnist_cf_tail(const pcg_mnist_cf_tail_args* args, pcg_stream_t stream) {
  PCG_REQUIRE(args, "pcg_mnist_cf_tail: null arguments");
  const pcg_mnist_cf_tail_args& a = *args;
  PCG_REQUIRE(a.c && a.x && a.mask && a.x_cf && a.sums, "pcg_mnist_cf_tail: null c, x, mask, x_cf or sums");
  PCG_REQUIRE(a.HW >= 4 && a.HW % 4 == 0 && window_ok(a.B, a.T, a.q0, a.nq),
              "pcg_mnist_cf_tail: HW %d (a multiple of 4), window [%d, +%d) of %d x %d queries", a.HW, a.q0, a.nq, a.T, a.B);
  PCG_REQUIRE(mode_ok(a.mask_mode), "pcg_mnist_cf_tail: mask mode %d", a.mask_mode);
  PCG_REQUIRE(aligned16(a.c) && aligned16(a.x) && aligned16(a.mask) && aligned16(a.x_cf) && aligned16(a.raw) && aligned16(a.masked),
              "pcg_mnist_cf_tail: rows are read and written 16 bytes at a time; a pointer is not 16-byte aligned");
  const int per = NT / WAVE;
  hipLaunchKernelGGL(mnist_cf_tail_kernel, dim3((unsigned)((a.nq + per - 1) / per)), dim3(NT), 0, (hipStream_t)stream, a);
  return launch_status("mnist_cf_tail_kernel");
}

extern "C" int pcg_mnist_cf_score(const pcg_mnist_cf_score_args* args, pcg_stream_t stream) {
  PCG_REQUIRE(args, "pcg_mnist_cf_score: null arguments");
  const pcg_mnist_cf_score_args& a = *args;
  PCG_REQUIRE(a.logits_cf, "pcg_mnist_cf_score: null logits_cf");
  PCG_REQUIRE(a.K >= 1 && a.K <= SCORE_KMAX && a.ld >= a.K && a.group_rows >= 1 && window_ok(a.B, a.T, a.q0, a.nq),
              "pcg_mnist_cf_score: K %d (<= %d), ld %d, group_rows %d, window [%d, +%d) of %d x %d queries", a.K, SCORE_KMAX, a.ld, a.group_rows,
              a.q0, a.nq, a.T, a.B);
  PCG_REQUIRE(a.target ? a.T == 1 : a.T <= a.K, "pcg_mnist_cf_score: the per-row form (target [B]) takes T = 1, the sweep T <= K (T %d, K %d)", a.T,
              a.K);
  PCG_REQUIRE(!a.logits_orig || a.y_true, "pcg_mnist_cf_score: logits_orig needs y_true");
  PCG_REQUIRE(a.pred || a.conf || a.p_target || a.p_true || a.p_orig_true || a.flip || a.group_sums, "pcg_mnist_cf_score: no output");
  const int64_t n_groups = ceil_div64(a.B, a.group_rows);
  PCG_REQUIRE(n_groups * a.T <= INT32_MAX, "pcg_mnist_cf_score: %lld groups exceed the grid", (long long)(n_groups * a.T));
  hipLaunchKernelGGL(mnist_cf_score_kernel, dim3((unsigned)(n_groups * a.T)), dim3(NT), 0, (hipStream_t)stream, a, (int)n_groups);
  return launch_status("mnist_cf_score_kernel");
}
