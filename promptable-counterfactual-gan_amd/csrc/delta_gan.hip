// delta_gan.hip — the launches around the convolutions of the additive-delta MNIST CounteRGAN step
// (conditional_counteRGAN/mnist/gan_train.py:117-144 on modules/generator.py and modules/discriminator.py).  All fp32,
// every sum in a fixed order, no floating-point atomics; every entry takes a stream and can be captured.
//
//   pcg_delta_gan_entry      the 2-channel NHWC inputs of G and of D's 2B-row pass (three pcg_embed_concat_fwd launches), the label
//                            index of D's table gradient and the (h,w,c) image of D's Linear weight row; REGATHER: the label map of
//                            D's rows B..2B alone, after Adam(D)
//   pcg_delta_gan_tail_fwd   x_cf = x + delta to the classifier's input and to channel 0 of D's rows B..2B, and mean|delta|
//   pcg_logit_head_fwd       Flatten + Linear(F -> 1) + both BCEWithLogitsLoss terms, the loss's gradient and the bias gradient
//   pcg_logit_head_bwd       the head's grad-input with conv3's LeakyReLU derivative applied, and the weight row's gradient
//   pcg_delta_gan_tail_bwd   d_delta = dD + lambda_cls * dC + (lambda_reg / n) * sign(delta)
//
// Two kernels finish a sum in the last workgroup to arrive (tail_fwd: the chunk sums; head_fwd: the loss over the rows).  The protocol
// is the one of house_residual_fwd_kernel (tabular.hip): thread 0 publishes the workgroup's value with an agent-scope store, waits for
// it, takes a ticket; the workgroup that draws the last ticket re-arms the counter and reads every value back with agent-scope loads.
#include "pcg_common.h"

namespace pcg {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;
constexpr int NT = 256;
constexpr int CHUNK = PCG_DELTA_GAN_CHUNK;      // NT threads x 4 elements
constexpr int TAIL_MAX_GRID = 1024;
constexpr int HB_GROUPS = 16;                   // row groups (waves) of head_bwd_kernel
constexpr int WS_HEAD = 16;                     // bytes in front of the chunk sums: the ticket

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

__device__ __forceinline__ void publish(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float collect(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// thread 0, after its publish(): true in the workgroup that arrives last; the counter is zero again when it returns true
__device__ __forceinline__ bool last_ticket(int* ticket, int n) {
  __builtin_amdgcn_s_waitcnt(0);
  const int t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (t != n - 1) return false;
  __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

template <typename T>
__device__ __forceinline__ T block_tree_256(T v, T* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int k = NT / 2; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  const T s = red[0];
  __syncthreads();
  return s;
}

// ---- entry: one thread per (row, pixel) -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NT) delta_gan_entry_kernel(pcg_delta_gan_entry_args a) {
  const int64_t n = (int64_t)a.B * a.HW;
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  const int nhead = a.head_w ? a.head_C * a.head_P : 0;
  if (i < nhead) {                                            // f = p * C + c  <-  c * P + p
    const int p = (int)i / a.head_C, c = (int)i - p * a.head_C;
    a.head_w_packed[i] = a.head_w[(size_t)c * a.head_P + p];
  }
  if (i >= n) return;
  const int b = (int)(i / a.HW), p = (int)(i - (int64_t)b * a.HW);
  int64_t t = a.target[b];
  t = t < 0 ? 0 : (t >= a.K ? a.K - 1 : t);                   // as embed_concat_fwd_kernel: never read outside the table
  a.d_in[(size_t)(n + i) * 2 + 1] = a.table_d[(size_t)t * a.HW + p];
  if (a.mode == PCG_DELTA_GAN_REGATHER) return;
  int64_t k = a.y[b];
  k = k < 0 ? 0 : (k >= a.K ? a.K - 1 : k);
  const float xv = a.x[i];
  *reinterpret_cast<f32x2*>(a.g_in + (size_t)i * 2) = f32x2{xv, a.table_g[(size_t)t * a.HW + p]};
  *reinterpret_cast<f32x2*>(a.d_in + (size_t)i * 2) = f32x2{xv, a.table_d[(size_t)k * a.HW + p]};
  if (a.labels_2b && p == 0) { a.labels_2b[b] = a.y[b]; a.labels_2b[a.B + b] = a.target[b]; }
}

// ---- tail forward: a workgroup walks chunks of 1024 elements; thread t owns elements 4t..4t+3 of a chunk -------------------------------
__global__ void __launch_bounds__(NT) delta_gan_tail_fwd_kernel(pcg_delta_gan_tail_fwd_args a, int nchunks) {
  __shared__ float redf[NT];
  __shared__ double redd[NT];
  __shared__ int s_last;
  const int64_t n = (int64_t)a.B * a.HW;
  int* ticket = reinterpret_cast<int*>(a.workspace);
  float* partial = reinterpret_cast<float*>(reinterpret_cast<char*>(a.workspace) + WS_HEAD);
  float* __restrict__ dst0 = a.d_in + (size_t)n * 2;          // row B, pixel 0, channel 0
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t i = (int64_t)c * CHUNK + 4 * (int)threadIdx.x;
    float s = 0.f;
    if (i < n) {                                              // n % 4 == 0: a group of four is inside or outside as a whole
      const f32x4 xv = *reinterpret_cast<const f32x4*>(a.x + i), dv = *reinterpret_cast<const f32x4*>(a.delta + i);
      const f32x4 xc = xv + dv;
      *reinterpret_cast<f32x4*>(a.x_cf + i) = xc;
#pragma unroll
      for (int j = 0; j < 4; ++j) dst0[(size_t)(i + j) * 2] = xc[j];
      s = (fabsf(dv[0]) + fabsf(dv[1])) + (fabsf(dv[2]) + fabsf(dv[3]));
    }
    const float cs = block_tree_256(s, redf);
    if (threadIdx.x == 0) publish(partial + c, cs);
  }
  if (threadIdx.x == 0) s_last = last_ticket(ticket, (int)gridDim.x) ? 1 : 0;
  __syncthreads();
  if (!s_last) return;
  double acc = 0.0;
  for (int c = threadIdx.x; c < nchunks; c += NT) acc += (double)collect(partial + c);
  const double tot = block_tree_256(acc, redd);
  if (threadIdx.x == 0) a.loss_reg[0] = (float)(tot / (double)n);
}

// ---- head forward: one workgroup per row ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float bce_elem(float x, float t) {           // bce_logits_kernel's element (pointwise.hip)
  const float mx = fmaxf(-x, 0.f);
  return (1.f - t) * x + mx + logf(expf(-mx) + expf(-x - mx));
}

__global__ void __launch_bounds__(NT) logit_head_fwd_kernel(pcg_logit_head_fwd_args a) {
  __shared__ float redf[NT];
  __shared__ int s_last;
  const int r = blockIdx.x, R = a.R, F4 = a.F >> 2;
  const f32x4* __restrict__ row = reinterpret_cast<const f32x4*>(a.a + (size_t)r * a.F);
  const f32x4* __restrict__ w4 = reinterpret_cast<const f32x4*>(a.w);
  float acc = 0.f;
  for (int q = threadIdx.x; q < F4; q += NT) {
    const f32x4 av = row[q], wv = w4[q];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = fmaf(av[j], wv[j], acc);
  }
  const float dot = block_tree_256(acc, redf);
  if (threadIdx.x == 0) {
    publish(a.logits + r, dot + a.bias[0]);
    s_last = last_ticket(reinterpret_cast<int*>(a.workspace), R) ? 1 : 0;
  }
  __syncthreads();
  if (!s_last) return;
  const int half = a.mode == PCG_LOGIT_HEAD_D ? R / 2 : R;              // rows labelled 1
  const float inv1 = 1.f / (float)half, inv0 = a.mode == PCG_LOGIT_HEAD_D ? 1.f / (float)(R - half) : 0.f;
  float l1 = 0.f, l0 = 0.f, sb = 0.f;
  for (int q = threadIdx.x; q < R; q += NT) {
    const float z = collect(a.logits + q);
    const float t = q < half ? 1.f : 0.f;
    const float l = bce_elem(z, t);
    const float d = (q < half ? inv1 : inv0) * (1.f / (1.f + expf(-z)) - t);
    if (q < half) l1 += l; else l0 += l;
    a.dlogit[q] = d;
    sb += d;
  }
  const float s1 = block_tree_256(l1, redf), s0 = block_tree_256(l0, redf), sd = block_tree_256(sb, redf);
  if (threadIdx.x == 0) {
    a.loss[0] = a.mode == PCG_LOGIT_HEAD_D ? s1 * inv1 + s0 * inv0 : s1 * inv1;
    a.db[0] = sd;
  }
}

// ---- head backward: lane = a 16-byte column group, wave g = row group g of 16 -----------------------------------------------------------
__global__ void __launch_bounds__(64 * HB_GROUPS) logit_head_bwd_kernel(pcg_logit_head_bwd_args a, int rows_per_group) {
#pragma clang fp contract(off)
  __shared__ f32x4 part[HB_GROUPS][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int q = blockIdx.x * 64 + lane, F4 = a.F >> 2;
  const bool live = q < F4;
  f32x4 wv = {0.f, 0.f, 0.f, 0.f}, acc = {0.f, 0.f, 0.f, 0.f};
  if (live) wv = reinterpret_cast<const f32x4*>(a.w)[q];
  const int r0 = g * rows_per_group, r1 = min(r0 + rows_per_group, a.R);
  if (live) {
    for (int r = r0; r < r1; ++r) {
      const float dl = a.dlogit[r];
      const f32x4 av = reinterpret_cast<const f32x4*>(a.a + (size_t)r * a.F)[q];
      f32x4 dv;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        dv[j] = (dl * wv[j]) * (av[j] > 0.f ? 1.f : a.slope);
        acc[j] = fmaf(dl, av[j], acc[j]);
      }
      reinterpret_cast<f32x4*>(a.da + (size_t)r * a.F)[q] = dv;
    }
  }
  if (!a.dw) return;                                                   // uniform: no barrier below is skipped by part of a workgroup
  part[g][lane] = acc;
  __syncthreads();
  if (g == 0 && live) {
    f32x4 s = part[0][lane];
#pragma unroll
    for (int k = 1; k < HB_GROUPS; ++k) s += part[k][lane];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int f = 4 * q + j;
      if (a.dw_C > 0) {
        const int p = f / a.dw_C, c = f - p * a.dw_C;
        a.dw[(size_t)c * a.dw_P + p] = s[j];
      } else {
        a.dw[f] = s[j];
      }
    }
  }
}

// ---- tail backward: one thread per element ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NT) delta_gan_tail_bwd_kernel(pcg_delta_gan_tail_bwd_args a) {
#pragma clang fp contract(off)
  const int64_t n = (int64_t)a.B * a.HW;
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const float dl = a.delta[i];
  const float sg = dl > 0.f ? 1.f : (dl < 0.f ? -1.f : 0.f);
  const float t = a.dD[(size_t)i * a.dD_stride] + a.lambda_cls * a.dC[i];
  a.d_delta[i] = t + a.reg_scale * sg;
}

bool rows_ok(int B, int HW) { return B >= 1 && HW >= 1 && (int64_t)2 * B * HW * 2 <= (int64_t)INT32_MAX; }

}  // namespace
}  // namespace pcg

using namespace pcg;

extern "C" int pcg_delta_gan_entry(const pcg_delta_gan_entry_args* args, pcg_stream_t stream) {
  PCG_REQUIRE(args, "pcg_delta_gan_entry: null arguments");
  const pcg_delta_gan_entry_args& a = *args;
  PCG_REQUIRE(a.B >= 1, "pcg_delta_gan_entry: batch of %d rows", a.B);
  PCG_REQUIRE(a.HW >= 1 && a.K >= 1 && rows_ok(a.B, a.HW), "pcg_delta_gan_entry: HW %d, K %d, or %d rows exceed the index range", a.HW, a.K, a.B);
  PCG_REQUIRE(a.mode == PCG_DELTA_GAN_BUILD || a.mode == PCG_DELTA_GAN_REGATHER, "pcg_delta_gan_entry: mode %d", a.mode);
  PCG_REQUIRE(a.target && a.table_d && a.d_in, "pcg_delta_gan_entry: null target, table_d or d_in");
  if (a.mode == PCG_DELTA_GAN_BUILD)
    PCG_REQUIRE(a.x && a.y && a.table_g && a.g_in, "pcg_delta_gan_entry: null x, y, table_g or g_in");
  PCG_REQUIRE(aligned(a.d_in, 8) && aligned(a.g_in, 8), "pcg_delta_gan_entry: g_in and d_in are written 8 bytes at a time; a pointer is not aligned");
  PCG_REQUIRE(!a.head_w == !a.head_w_packed, "pcg_delta_gan_entry: head_w and head_w_packed go together");
  if (a.head_w)
    PCG_REQUIRE(a.head_C >= 1 && a.head_P >= 1 && (int64_t)a.head_C * a.head_P <= (int64_t)INT32_MAX && a.head_w != a.head_w_packed,
                "pcg_delta_gan_entry: head weight of %d x %d columns (packed out of place)", a.head_C, a.head_P);
  for (int pass = 0; pass < 2; ++pass) {
    const int64_t* h = pass ? a.target_host : a.y_host;
    if (!h) continue;
    for (int b = 0; b < a.B; ++b)
      PCG_REQUIRE(h[b] >= 0 && h[b] < a.K, "pcg_delta_gan_entry: label %lld of row %d (%s) is outside 0..%d", (long long)h[b], b,
                  pass ? "target" : "y", a.K - 1);
  }
  int64_t n = (int64_t)a.B * a.HW;                               // one thread per (row, pixel) and per column of the head weight
  if (a.head_w && (int64_t)a.head_C * a.head_P > n) n = (int64_t)a.head_C * a.head_P;
  hipLaunchKernelGGL(delta_gan_entry_kernel, dim3((unsigned)ceil_div64(n, NT)), dim3(NT), 0, (hipStream_t)stream, a);
  return launch_status("delta_gan_entry_kernel");
}

extern "C" size_t pcg_delta_gan_tail_workspace_bytes(int32_t B, int32_t HW) {
  if (!rows_ok(B, HW)) return 0;
  return WS_HEAD + (size_t)ceil_div64((int64_t)B * HW, CHUNK) * sizeof(float);
}

extern "C" int pcg_delta_gan_tail_fwd(const pcg_delta_gan_tail_fwd_args* args, pcg_stream_t stream) {
  PCG_REQUIRE(args, "pcg_delta_gan_tail_fwd: null arguments");
  const pcg_delta_gan_tail_fwd_args& a = *args;
  PCG_REQUIRE(a.B >= 1, "pcg_delta_gan_tail_fwd: batch of %d rows", a.B);
  PCG_REQUIRE(a.HW >= 4 && a.HW % 4 == 0 && rows_ok(a.B, a.HW), "pcg_delta_gan_tail_fwd: HW %d (a multiple of 4), or %d rows exceed the index range",
              a.HW, a.B);
  PCG_REQUIRE(a.x && a.delta && a.x_cf && a.d_in && a.loss_reg && a.workspace, "pcg_delta_gan_tail_fwd: null x, delta, x_cf, d_in, loss_reg or workspace");
  PCG_REQUIRE(aligned(a.x, 16) && aligned(a.delta, 16) && aligned(a.x_cf, 16) && aligned(a.d_in, 8) && aligned(a.workspace, 16),
              "pcg_delta_gan_tail_fwd: rows are read and written 16 bytes at a time; a pointer is not aligned");
  if (a.workspace_bytes < pcg_delta_gan_tail_workspace_bytes(a.B, a.HW)) {
    set_error("pcg_delta_gan_tail_fwd: workspace of %zu bytes, %zu needed", a.workspace_bytes, pcg_delta_gan_tail_workspace_bytes(a.B, a.HW));
    return PCG_ERR_WORKSPACE;
  }
  PCG_REQUIRE(a.grid >= 0 && a.grid <= TAIL_MAX_GRID, "pcg_delta_gan_tail_fwd: grid %d (0, or 1..%d)", a.grid, TAIL_MAX_GRID);
  const int nchunks = (int)ceil_div64((int64_t)a.B * a.HW, CHUNK);
  int grid = a.grid ? a.grid : TAIL_MAX_GRID;
  if (grid > nchunks) grid = nchunks;
  hipLaunchKernelGGL(delta_gan_tail_fwd_kernel, dim3(grid), dim3(NT), 0, (hipStream_t)stream, a, nchunks);
  return launch_status("delta_gan_tail_fwd_kernel");
}

extern "C" int pcg_logit_head_fwd(const pcg_logit_head_fwd_args* args, pcg_stream_t stream) {
  PCG_REQUIRE(args, "pcg_logit_head_fwd: null arguments");
  const pcg_logit_head_fwd_args& a = *args;
  PCG_REQUIRE(a.mode == PCG_LOGIT_HEAD_D || a.mode == PCG_LOGIT_HEAD_G, "pcg_logit_head_fwd: mode %d", a.mode);
  PCG_REQUIRE(a.R >= 1 && a.R <= 65535, "pcg_logit_head_fwd: %d rows (1..65535)", a.R);
  PCG_REQUIRE(a.mode != PCG_LOGIT_HEAD_D || a.R % 2 == 0, "pcg_logit_head_fwd: mode D takes real and fake halves; %d rows are odd", a.R);
  PCG_REQUIRE(a.F >= 4 && a.F % 4 == 0, "pcg_logit_head_fwd: F %d (a multiple of 4)", a.F);
  PCG_REQUIRE(a.a && a.w && a.bias && a.logits && a.loss && a.dlogit && a.db && a.workspace,
              "pcg_logit_head_fwd: null a, w, bias, logits, loss, dlogit, db or workspace");
  PCG_REQUIRE(aligned(a.a, 16) && aligned(a.w, 16) && aligned(a.workspace, 4), "pcg_logit_head_fwd: a and w are read 16 bytes at a time; a pointer is not aligned");
  hipLaunchKernelGGL(logit_head_fwd_kernel, dim3(a.R), dim3(NT), 0, (hipStream_t)stream, a);
  return launch_status("logit_head_fwd_kernel");
}

extern "C" int pcg_logit_head_bwd(const pcg_logit_head_bwd_args* args, pcg_stream_t stream) {
  PCG_REQUIRE(args, "pcg_logit_head_bwd: null arguments");
  const pcg_logit_head_bwd_args& a = *args;
  PCG_REQUIRE(a.R >= 1 && a.R <= 65535, "pcg_logit_head_bwd: %d rows (1..65535)", a.R);
  PCG_REQUIRE(a.F >= 4 && a.F % 4 == 0, "pcg_logit_head_bwd: F %d (a multiple of 4)", a.F);
  PCG_REQUIRE(a.a && a.w && a.dlogit && a.da, "pcg_logit_head_bwd: null a, w, dlogit or da");
  PCG_REQUIRE(aligned(a.a, 16) && aligned(a.w, 16) && aligned(a.da, 16), "pcg_logit_head_bwd: rows are read and written 16 bytes at a time; a pointer is not aligned");
  PCG_REQUIRE((a.dw_C == 0 && a.dw_P == 0) || (a.dw_C >= 1 && a.dw_P >= 1 && (int64_t)a.dw_C * a.dw_P == a.F),
              "pcg_logit_head_bwd: dw order %d x %d does not cover F %d", a.dw_C, a.dw_P, a.F);
  const int rpg = ceil_div(a.R, HB_GROUPS);
  hipLaunchKernelGGL(logit_head_bwd_kernel, dim3(ceil_div(a.F / 4, 64)), dim3(64 * HB_GROUPS), 0, (hipStream_t)stream, a, rpg);
  return launch_status("logit_head_bwd_kernel");
}

extern "C" int pcg_delta_gan_tail_bwd(const pcg_delta_gan_tail_bwd_args* args, pcg_stream_t stream) {
  PCG_REQUIRE(args, "pcg_delta_gan_tail_bwd: null arguments");
  const pcg_delta_gan_tail_bwd_args& a = *args;
  PCG_REQUIRE(a.B >= 1, "pcg_delta_gan_tail_bwd: batch of %d rows", a.B);
  PCG_REQUIRE(a.HW >= 1 && rows_ok(a.B, a.HW), "pcg_delta_gan_tail_bwd: HW %d, or %d rows exceed the index range", a.HW, a.B);
  PCG_REQUIRE(a.dD && a.dC && a.delta && a.d_delta, "pcg_delta_gan_tail_bwd: null dD, dC, delta or d_delta");
  PCG_REQUIRE(a.dD_stride == 1 || a.dD_stride == 2, "pcg_delta_gan_tail_bwd: dD_stride %d (1: one channel, 2: channel 0 of two)", a.dD_stride);
  const int64_t n = (int64_t)a.B * a.HW;
  hipLaunchKernelGGL(delta_gan_tail_bwd_kernel, dim3((unsigned)ceil_div64(n, NT)), dim3(NT), 0, (hipStream_t)stream, a);
  return launch_status("delta_gan_tail_bwd_kernel");
}
