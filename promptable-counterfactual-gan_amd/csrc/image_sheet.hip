// image_sheet.hip — the normalised image sheets of the trainers: torchvision's make_grid and the pixels of save_image as
// the reference calls them on CPU fp32 tensors: dconv_gan/mnist/mnist_dcgan.py:190 and :222, simple_gan/mnist/mnist_gan.py:141,
// conditional_counteRGAN/mnist/gan_train.py:161-163 and countergan2.py:222-224, conditional_gan/mnist/mnist_wgan_conditional.py:123-125
// and :181-182.
//   image_range   the minimum and maximum of pre_scale * x + pre_shift over n floats -> range [2] (device)
//   image_sheet   one thread per pixel of the grid plane: pad_value or the (normalised) element -> the float grid [C', Hg, Wg], the
//                 uint8 image [Hg, Wg, 3] (or [Hg, Wg]), or both
// Streaming kernels, fp32, wave64.  The sheet pass reads lo and hi from device memory and forms the divisor itself, so nothing is read
// on the host between the two launches and both can be captured in one HIP graph.
//
// The range pass: every workgroup leaves one (min, max) pair in the workspace and takes a ticket; the workgroup that draws the last
// ticket folds the pairs.  The ticket is an atomicInc that wraps at the grid size, so the counter is zero again when the launch ends:
// no state is set between calls (the workspace is zeroed once, when it is allocated).  A minimum and a maximum do not depend on the
// order of their operands: the range is the same bits for any order of workgroups.  Values are reduced as floats (fminf / fmaxf), so
// negative values are ordered as they should be; a NaN operand is dropped by both, so a NaN input cannot fault and its pixels are
// unspecified.
//
// Every pixel operation is ONE fp32 rounding, as in cf_report.hip: plain operators under `#pragma clang fp contract(off)`, so neither
// pre_scale * x + pre_shift nor g * 255 + 0.5 becomes one v_fma_f32; the division is the correctly rounded fp32 division (hipcc's
// default for HIP), not a multiplication by a reciprocal.
#include <cstdint>
#include "pcg_common.h"

#pragma clang fp contract(off)

namespace pcg {
namespace {

constexpr int NT = 256, WAVE = 64, NW = NT / WAVE;
constexpr unsigned RANGE_MAX_BLOCKS = 256;                   // pairs the last workgroup folds: one per thread
constexpr unsigned SHEET_MAX_BLOCKS = 8192;
constexpr size_t WS_HEAD = 16;                               // bytes in front of the pairs: the ticket

struct MinMax {
  float lo, hi;
  __device__ __forceinline__ void take(float v) { lo = fminf(lo, v); hi = fmaxf(hi, v); }
  __device__ __forceinline__ void take(MinMax o) { lo = fminf(lo, o.lo); hi = fmaxf(hi, o.hi); }
};

__device__ __forceinline__ float pre_apply(float v, float scale, float shift, int has_pre) {
  return has_pre ? v * scale + shift : v;                    // two roundings: contraction is off in this file
}

// wave by shuffles, block through LDS; every thread returns the block's pair
__device__ __forceinline__ MinMax block_minmax(MinMax m, float* red) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    m.lo = fminf(m.lo, __shfl_xor(m.lo, o, WAVE));
    m.hi = fmaxf(m.hi, __shfl_xor(m.hi, o, WAVE));
  }
  const int w = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) { red[2 * w] = m.lo; red[2 * w + 1] = m.hi; }
  __syncthreads();
  MinMax r = {red[0], red[1]};
#pragma unroll
  for (int k = 1; k < NW; ++k) r.take(MinMax{red[2 * k], red[2 * k + 1]});
  __syncthreads();
  return r;
}

// x [n]: `head` scalar elements up to the first 16-byte boundary, n4 float4 groups, the rest scalar.  The scalar ends belong to
// workgroup 0.
__global__ void __launch_bounds__(NT) image_range_kernel(const float* __restrict__ x, uint32_t n, uint32_t head, uint32_t n4, float scale,
                                                         float shift, int has_pre, float* __restrict__ range,
                                                         unsigned* __restrict__ ticket, float* __restrict__ pairs) {
  __shared__ float red[2 * NW];
  __shared__ int s_last;
  MinMax m = {__builtin_inff(), -__builtin_inff()};
  const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x + head);
  for (uint32_t q = blockIdx.x * NT + threadIdx.x; q < n4; q += gridDim.x * NT) {
    const float4 v = x4[q];
    m.take(pre_apply(v.x, scale, shift, has_pre));
    m.take(pre_apply(v.y, scale, shift, has_pre));
    m.take(pre_apply(v.z, scale, shift, has_pre));
    m.take(pre_apply(v.w, scale, shift, has_pre));
  }
  if (blockIdx.x == 0) {
    const uint32_t tail0 = head + 4 * n4;                    // head <= 3 and n - tail0 <= 3: one thread each
    if (threadIdx.x < head) m.take(pre_apply(x[threadIdx.x], scale, shift, has_pre));
    if (tail0 + threadIdx.x < n) m.take(pre_apply(x[tail0 + threadIdx.x], scale, shift, has_pre));
  }
  m = block_minmax(m, red);
  if (gridDim.x == 1) {                                      // one workgroup: no pairs, no ticket
    if (threadIdx.x == 0) { range[0] = m.lo; range[1] = m.hi; }
    return;
  }
  if (threadIdx.x == 0) {
    __hip_atomic_store(pairs + 2 * blockIdx.x, m.lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(pairs + 2 * blockIdx.x + 1, m.hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");       // the pair is visible to the device before the ticket is taken
    // wraps to 0 at gridDim.x - 1: the last ticket of a launch leaves the counter as the first one found it
    s_last = atomicInc(ticket, gridDim.x - 1) == gridDim.x - 1;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  __syncthreads();
  if (!s_last) return;
  MinMax f = {__builtin_inff(), -__builtin_inff()};
  if (threadIdx.x < gridDim.x) {                             // gridDim.x <= RANGE_MAX_BLOCKS == NT
    f.lo = __hip_atomic_load(pairs + 2 * threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    f.hi = __hip_atomic_load(pairs + 2 * threadIdx.x + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  f = block_minmax(f, red);
  if (threadIdx.x == 0) { range[0] = f.lo; range[1] = f.hi; }
}

__device__ __forceinline__ uint8_t to_u8(float v) {          // cf_report.hip's: min(255, max(0, floor(v * 255 + 0.5)))
  const float q = floorf(v * 255.f + 0.5f);                  // two roundings
  return (uint8_t)fminf(255.f, fmaxf(0.f, q));               // a NaN becomes 0
}

struct SheetArgs {
  const float* x;          // [N][C][H][W]
  const float* range;      // [2] on the device, or null: lo, hi, d below
  float* grid;             // nullable: [C'][Hg][Wg], C' = 3
  uint8_t* u8;             // nullable: [Hg][Wg][3], or [Hg][Wg] with gray
  float lo, hi, d, pad_value, scale, shift;
  int N, C, H, W, xmaps, pad, Hg, Wg, normalize, has_pre, gray;
};

__global__ void __launch_bounds__(NT) image_sheet_kernel(SheetArgs a) {
  float lo = a.lo, hi = a.hi, d = a.d;
  if (a.normalize && a.range) {
    lo = a.range[0];
    hi = a.range[1];
    d = (float)fmax((double)hi - (double)lo, 1e-5);          // float32(max(double(hi) - double(lo), 1e-5))
  }
  const uint32_t HW = (uint32_t)a.H * a.W, plane = (uint32_t)a.Hg * a.Wg;
  const uint32_t ch = (uint32_t)a.H + a.pad, cw = (uint32_t)a.W + a.pad;
  const uint8_t pad_u8 = to_u8(a.pad_value);
  for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < plane; i += gridDim.x * NT) {
    const uint32_t gy = i / a.Wg, gx = i - gy * a.Wg;
    float v[3] = {a.pad_value, a.pad_value, a.pad_value};
    bool inside = gy >= (uint32_t)a.pad && gx >= (uint32_t)a.pad;
    if (inside) {
      const uint32_t ry = gy - a.pad, rx = gx - a.pad;
      const uint32_t cy = ry / ch, iy = ry - cy * ch, cx = rx / cw, ix = rx - cx * cw;
      const uint32_t k = cy * a.xmaps + cx;
      inside = iy < (uint32_t)a.H && ix < (uint32_t)a.W && cx < (uint32_t)a.xmaps && k < (uint32_t)a.N;
      if (inside) {
        const float* src = a.x + (size_t)k * a.C * HW + iy * a.W + ix;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (c < a.C) {
            float e = pre_apply(src[(size_t)c * HW], a.scale, a.shift, a.has_pre);
            if (a.normalize) e = (fminf(fmaxf(e, lo), hi) - lo) / d;
            v[c] = e;
          } else {
            v[c] = v[0];                                     // C == 1: the channel three times
          }
        }
      }
    }
    if (a.grid) {
      a.grid[i] = v[0];
      a.grid[plane + i] = v[1];
      a.grid[2 * (size_t)plane + i] = v[2];
    }
    if (a.u8) {
      if (a.gray) {
        a.u8[i] = inside ? to_u8(v[0]) : pad_u8;
      } else {
        uint8_t* o = a.u8 + 3 * (size_t)i;
        o[0] = inside ? to_u8(v[0]) : pad_u8;
        o[1] = inside ? to_u8(v[1]) : pad_u8;
        o[2] = inside ? to_u8(v[2]) : pad_u8;
      }
    }
  }
}

}  // namespace
}  // namespace pcg

using namespace pcg;

extern "C" size_t pcg_image_range_workspace_bytes(void) { return WS_HEAD + 2 * sizeof(float) * RANGE_MAX_BLOCKS; }

extern "C" int pcg_image_range(const float* x, int64_t n, float pre_scale, float pre_shift, float* range, void* workspace,
                               size_t workspace_bytes, pcg_stream_t stream) {
  PCG_REQUIRE(x && range && workspace, "pcg_image_range: null x, range or workspace");
  PCG_REQUIRE(n >= 1 && n <= (int64_t)INT32_MAX, "pcg_image_range: n %lld is outside [1, 2^31 - 1]", (long long)n);
  PCG_REQUIRE(((uintptr_t)x & 3) == 0, "pcg_image_range: x is not 4-byte aligned");
  PCG_REQUIRE(((uintptr_t)range & 3) == 0, "pcg_image_range: range is not 4-byte aligned");
  PCG_REQUIRE(((uintptr_t)workspace & 15) == 0, "pcg_image_range: workspace is not 16-byte aligned");
  PCG_REQUIRE(workspace_bytes >= pcg_image_range_workspace_bytes(), "pcg_image_range: workspace of %zu bytes, %zu needed", workspace_bytes,
              pcg_image_range_workspace_bytes());
  uint32_t head = (uint32_t)((4 - (((uintptr_t)x >> 2) & 3)) & 3);       // floats up to the first 16-byte boundary
  if ((int64_t)head > n) head = (uint32_t)n;
  const uint32_t n4 = ((uint32_t)n - head) / 4;
  unsigned blocks = (n4 + NT - 1) / NT;
  if (blocks > RANGE_MAX_BLOCKS) blocks = RANGE_MAX_BLOCKS;
  if (blocks < 1) blocks = 1;
  const int has_pre = !(pre_scale == 1.f && pre_shift == 0.f);
  hipLaunchKernelGGL(image_range_kernel, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, x, (uint32_t)n, head, n4, pre_scale, pre_shift, has_pre,
                     range, reinterpret_cast<unsigned*>(workspace), reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + WS_HEAD));
  return launch_status("image_range_kernel");
}

extern "C" int pcg_image_sheet(const pcg_image_sheet_args* p, pcg_stream_t stream) {
  PCG_REQUIRE(p && p->x, "pcg_image_sheet: null args or x");
  PCG_REQUIRE(p->grid || p->u8, "pcg_image_sheet: writes a float grid, a uint8 image or both");
  PCG_REQUIRE(p->C == 1 || p->C == 3, "pcg_image_sheet: C %d is neither 1 nor 3", p->C);
  PCG_REQUIRE(p->N >= 1 && p->H >= 1 && p->W >= 1 && p->nrow >= 1, "pcg_image_sheet: N %d, H %d, W %d, nrow %d", p->N, p->H, p->W, p->nrow);
  PCG_REQUIRE(p->padding >= 0, "pcg_image_sheet: padding %d", p->padding);
  PCG_REQUIRE(!p->gray || p->C == 1, "pcg_image_sheet: a gray image takes C == 1");
  PCG_REQUIRE(((uintptr_t)p->x & 3) == 0 && ((uintptr_t)p->grid & 3) == 0, "pcg_image_sheet: x or grid is not 4-byte aligned");
  PCG_REQUIRE(((uintptr_t)p->range & 3) == 0, "pcg_image_sheet: range is not 4-byte aligned");
  PCG_REQUIRE((int64_t)p->N * p->C * p->H * p->W <= (int64_t)INT32_MAX, "pcg_image_sheet: %d x %d x %d x %d exceeds the index range", p->N, p->C,
              p->H, p->W);
  // make_grid: a single image is its own grid; else xmaps x ymaps cells of (H + padding) x (W + padding) behind a border of padding
  const bool single = p->N == 1;
  const int64_t pad = single ? 0 : p->padding;
  const int64_t xmaps = p->nrow < p->N ? p->nrow : p->N, ymaps = (p->N + xmaps - 1) / xmaps;
  const int64_t Hg = ymaps * (p->H + pad) + pad, Wg = xmaps * (p->W + pad) + pad;
  PCG_REQUIRE(Hg <= INT32_MAX && Wg <= INT32_MAX && 3 * Hg * Wg <= (int64_t)INT32_MAX, "pcg_image_sheet: a 3 x %lld x %lld grid exceeds the index range",
              (long long)Hg, (long long)Wg);
  SheetArgs a;
  a.x = p->x; a.range = p->normalize ? p->range : nullptr; a.grid = p->grid; a.u8 = p->u8;
  a.lo = p->lo; a.hi = p->hi; a.d = p->d; a.pad_value = p->pad_value; a.scale = p->pre_scale; a.shift = p->pre_shift;
  a.N = p->N; a.C = p->C; a.H = p->H; a.W = p->W; a.xmaps = (int)xmaps; a.pad = (int)pad; a.Hg = (int)Hg; a.Wg = (int)Wg;
  a.normalize = p->normalize ? 1 : 0;
  a.has_pre = !(p->pre_scale == 1.f && p->pre_shift == 0.f);
  a.gray = p->gray ? 1 : 0;
  if (a.normalize && !a.range) PCG_REQUIRE(p->d > 0.f && p->lo <= p->hi, "pcg_image_sheet: value range [%g, %g] with divisor %g", p->lo, p->hi, p->d);
  size_t blocks = ((size_t)Hg * Wg + NT - 1) / NT;
  if (blocks > SHEET_MAX_BLOCKS) blocks = SHEET_MAX_BLOCKS;
  hipLaunchKernelGGL(image_sheet_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, a);
  return launch_status("image_sheet_kernel");
}
