// cf_report.hip — the numbers and pixels of the MNIST CounteRGAN's report figures:
// conditional_counteRGAN/mnist eval_utils.py:113-201 (visualize_counterfactual_grid: one source row per class, the source-by-target grid),
// gr.py / gradio_app.py:346-441 (make_and_save_heatmaps) and :498-568 (save_user_modification_example): four panels per sample.
//   class_pick          one key per row, the maximum key per class: the first row of a class, or its most confident one
//   class_pick_gather   the K winning keys -> row indices, confidences and the source images
//   cf_panels           the [K*H, T*W] grid image (float and uint8), or the [n, 4, H, W] panels with their colour-scale maximum
// Streaming kernels, fp32, wave64.  The only atomics are integer maxima (64-bit keys, float bits of values >= 0): a maximum does not
// depend on the order of its operands, so every result is the same for any order of blocks, waves and chunks.
//
// Every pixel operation is ONE fp32 rounding, so the output is bit-identical to NumPy's fp32 expressions.  hipcc's default is
// -ffp-contract=fast, and the __f*_rn intrinsics do not stop it (this toolchain's headers define them as plain operators that carry
// the header's own contraction setting into the kernel), so the pixel arithmetic is written with plain operators under
// `#pragma clang fp contract(off)` below: no multiply is fused with an add that follows it (v * 255 + 0.5 would otherwise become one
// v_fma_f32; the device assembly of the two pixel kernels holds no v_fma / v_fmac).  The pragma stands after the includes:
// softmax_label.h is compiled here as it is in mnist_cf_eval.hip.
#include <cstdint>
#include "pcg_common.h"
#include "softmax_label.h"

#pragma clang fp contract(off)

namespace pcg {
namespace {

constexpr int NT = 256, WAVE = 64;
constexpr int PICK_KMAX = PCG_CLASS_PICK_KMAX;
constexpr unsigned MAX_BLOCKS = 8192;

unsigned blocks_for(size_t n) {
  size_t b = (n + NT - 1) / NT;
  if (b > MAX_BLOCKS) b = MAX_BLOCKS;
  if (b < 1) b = 1;
  return (unsigned)b;
}

// ---- pick: one thread per row; K keys per block in LDS, then at most K global atomics per block ------------------------------------
__global__ void __launch_bounds__(NT) class_pick_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                        unsigned long long* __restrict__ state, int n, int kp, int K, uint32_t row0,
                                                        int mode) {
  __shared__ unsigned long long best[PICK_KMAX];
  const int tid = threadIdx.x;
  if (tid < PICK_KMAX) best[tid] = 0ull;
  __syncthreads();
  const int i = blockIdx.x * NT + tid;                       // the launch has ceil(n / NT) blocks
  if (i < n) {
    const int64_t y = labels[i];
    if (y >= 0 && y < K) {                                   // a label outside [0, K) names no class: the row is skipped
      uint32_t hi = 1u;
      bool ok = true;
      if (mode == PCG_CLASS_PICK_BEST) {
        const float c = softmax_prob_at(logits + (size_t)i * kp, K, (int)y);
        ok = c == c && fabsf(c) <= 3.402823466e38f;          // a NaN never wins the reference's `>` either
        hi = __float_as_uint(c);                             // c >= 0: floats order as their bit patterns
      }
      if (ok) atomicMax(&best[y], ((unsigned long long)hi << 32) | (unsigned long long)(0xFFFFFFFFu - (row0 + (uint32_t)i)));
    }
  }
  __syncthreads();
  if (tid < K && best[tid] != 0ull) atomicMax(&state[tid], best[tid]);
}

// ---- gather: one block per class -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NT) class_pick_gather_kernel(const unsigned long long* __restrict__ state, const float* __restrict__ X,
                                                               int64_t* __restrict__ rows, float* __restrict__ conf,
                                                               float* __restrict__ sources, int64_t N, int HW, int mode) {
  const int k = blockIdx.x;
  const unsigned long long w = state[k];
  const int64_t row = w ? (int64_t)(0xFFFFFFFFu - (uint32_t)(w & 0xFFFFFFFFull)) : -1;
  if (threadIdx.x == 0) {
    rows[k] = row;
    conf[k] = (w && mode == PCG_CLASS_PICK_BEST) ? __uint_as_float((uint32_t)(w >> 32)) : 0.f;
  }
  if (X && sources) {
    const bool live = row >= 0 && row < N;                   // a row beyond the resident data set is never read
    for (int p = threadIdx.x; p < HW; p += NT) sources[(size_t)k * HW + p] = live ? X[(size_t)row * HW + p] : 0.f;
  }
}

// ---- pixels ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float to_unit(float v) { return (v + 1.f) / 2.f; }                        // (v + 1.0) / 2.0

__device__ __forceinline__ uint8_t to_u8(float v) {          // min(255, max(0, floor(v * 255 + 0.5)))
  const float q = floorf(v * 255.f + 0.5f);                  // two roundings: contraction is off in this file
  return (uint8_t)fminf(255.f, fmaxf(0.f, q));               // a NaN becomes 0
}

__global__ void __launch_bounds__(NT) cf_grid_kernel(const float* __restrict__ sources, const float* __restrict__ x_cf,
                                                     float* __restrict__ image, uint8_t* __restrict__ image_u8, int K, int T, int H, int W) {
  const uint32_t HW = (uint32_t)H * W, row_len = (uint32_t)T * W, total = (uint32_t)K * H * row_len;
  for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < total; i += gridDim.x * NT) {
    const uint32_t gy = i / row_len, gx = i - gy * row_len;
    const uint32_t r = gy / H, y = gy - r * H, c = gx / W, x = gx - c * W;
    const uint32_t p = y * W + x;
    const float v = to_unit(r == c ? sources[(size_t)r * HW + p] : x_cf[((size_t)c * K + r) * HW + p]);
    if (image) image[i] = v;
    if (image_u8) image_u8[i] = to_u8(v);
  }
}

__global__ void __launch_bounds__(NT) cf_panels_kernel(const float* __restrict__ x, const float* __restrict__ x_cf,
                                                       const float* __restrict__ mask, float* __restrict__ panels,
                                                       float* __restrict__ vmax, int n, int HW, int mask_mode) {
  const uint32_t total = (uint32_t)n * HW;
  float mx = 0.f;
  for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < total; i += gridDim.x * NT) {
    const uint32_t b = i / HW, p = i - b * HW;
    const float xv = to_unit(x[i]), cv = to_unit(x_cf[i]);
    const float d = fabsf(cv - xv);
    float* o = panels + (size_t)b * 4 * HW + p;
    o[0] = xv;
    o[HW] = cv;
    o[2 * (size_t)HW] = d;
    o[3 * (size_t)HW] = mask[mask_mode == PCG_MASK_SHARED ? p : i];
    mx = fmaxf(mx, d);
  }
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, WAVE));
  // d >= 0: the float maximum is the maximum of the bit patterns; one atomic per wave that saw a positive value
  if ((threadIdx.x & (WAVE - 1)) == 0 && mx > 0.f) atomicMax(reinterpret_cast<unsigned int*>(vmax), __float_as_uint(mx));
}

}  // namespace
}  // namespace pcg

using namespace pcg;

extern "C" int pcg_class_pick(const float* logits, const int64_t* labels, uint64_t* state, int32_t n, int32_t kp, int32_t K, int64_t row0,
                              int32_t mode, pcg_stream_t stream) {
  PCG_REQUIRE(labels && state, "pcg_class_pick: null labels or state");
  PCG_REQUIRE(mode == PCG_CLASS_PICK_FIRST || mode == PCG_CLASS_PICK_BEST, "pcg_class_pick: mode %d", mode);
  PCG_REQUIRE(K >= 1 && K <= PICK_KMAX, "pcg_class_pick: K %d is outside [1, %d]", K, PICK_KMAX);
  PCG_REQUIRE(n >= 1 && (int64_t)n <= (int64_t)INT32_MAX - NT, "pcg_class_pick: n %d", n);
  PCG_REQUIRE(row0 >= 0 && row0 + (int64_t)n <= (int64_t)0xFFFFFFFFll,
              "pcg_class_pick: rows [%lld, +%d) do not stay below 2^32 - 1 (the key holds 0xFFFFFFFF - row)", (long long)row0, n);
  PCG_REQUIRE(((uintptr_t)state & 7) == 0, "pcg_class_pick: state is not 8-byte aligned");
  if (mode == PCG_CLASS_PICK_BEST)
    PCG_REQUIRE(logits && kp >= K && kp % 4 == 0, "pcg_class_pick: best mode reads logits [n, kp] with kp >= K a multiple of 4 (kp %d, K %d)", kp, K);
  hipLaunchKernelGGL(class_pick_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, logits, labels,
                     reinterpret_cast<unsigned long long*>(state), n, kp, K, (uint32_t)row0, mode);
  return launch_status("class_pick_kernel");
}

extern "C" int pcg_class_pick_gather(const uint64_t* state, const float* X, int64_t* rows, float* conf, float* sources, int32_t K, int64_t N,
                                     int32_t HW, int32_t mode, pcg_stream_t stream) {
  PCG_REQUIRE(state && rows && conf, "pcg_class_pick_gather: null state, rows or conf");
  PCG_REQUIRE(mode == PCG_CLASS_PICK_FIRST || mode == PCG_CLASS_PICK_BEST, "pcg_class_pick_gather: mode %d", mode);
  PCG_REQUIRE(K >= 1 && K <= PICK_KMAX, "pcg_class_pick_gather: K %d is outside [1, %d]", K, PICK_KMAX);
  PCG_REQUIRE((X == nullptr) == (sources == nullptr), "pcg_class_pick_gather: X and sources go together");
  if (X) PCG_REQUIRE(N >= 1 && HW >= 1, "pcg_class_pick_gather: X [N, HW] with N %lld, HW %d", (long long)N, HW);
  hipLaunchKernelGGL(class_pick_gather_kernel, dim3((unsigned)K), dim3(NT), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned long long*>(state), X, rows, conf, sources, N, HW, mode);
  return launch_status("class_pick_gather_kernel");
}

extern "C" int pcg_cf_panels(int32_t mode, const float* x, const float* x_cf, const float* mask, int32_t mask_mode, float* out,
                             uint8_t* out_u8, float* vmax, int32_t n, int32_t T, int32_t H, int32_t W, pcg_stream_t stream) {
  PCG_REQUIRE(x && x_cf, "pcg_cf_panels: null x or x_cf");
  PCG_REQUIRE(n >= 1 && H >= 1 && W >= 1, "pcg_cf_panels: n %d, H %d, W %d", n, H, W);
  if (mode == PCG_CF_PANELS_GRID) {
    PCG_REQUIRE(out || out_u8, "pcg_cf_panels: grid mode writes a float image, a uint8 image or both");
    PCG_REQUIRE(T >= 1 && (int64_t)n * H * T * W <= INT32_MAX, "pcg_cf_panels: a grid of %d x %d cells of %d x %d exceeds the index range", n, T,
                H, W);
    hipLaunchKernelGGL(cf_grid_kernel, dim3(blocks_for((size_t)n * H * T * W)), dim3(NT), 0, (hipStream_t)stream, x, x_cf, out, out_u8, n, T,
                       H, W);
    return launch_status("cf_grid_kernel");
  }
  PCG_REQUIRE(mode == PCG_CF_PANELS_PANELS, "pcg_cf_panels: mode %d", mode);
  PCG_REQUIRE(mask && out && vmax, "pcg_cf_panels: panels mode needs mask, out and vmax");
  PCG_REQUIRE(mask_mode == PCG_MASK_SHARED || mask_mode == PCG_MASK_PER_ROW, "pcg_cf_panels: mask mode %d", mask_mode);
  PCG_REQUIRE((int64_t)n * 4 * H * W <= INT32_MAX, "pcg_cf_panels: %d rows of 4 x %d x %d exceed the index range", n, H, W);
  PCG_REQUIRE(((uintptr_t)vmax & 3) == 0, "pcg_cf_panels: vmax is not 4-byte aligned");
  hipLaunchKernelGGL(cf_panels_kernel, dim3(blocks_for((size_t)n * H * W)), dim3(NT), 0, (hipStream_t)stream, x, x_cf, mask, out, vmax, n,
                     H * W, mask_mode);
  return launch_status("cf_panels_kernel");
}
