// maxpool.hip — ReLU + MaxPool2d(2) of an NHWC activation and its backward (conditional_counteRGAN/mnist/modules/classifier.py:9-13),
// fp32, gfx950.  HBM-bound streaming kernels: one thread owns four channels of one pooled pixel, so its four window cells are four
// float4 loads (the lanes of a wave walk C, then the pooled column: every load instruction covers whole contiguous runs of C floats)
// and its results one float4 store plus one 4-byte store of the four window positions.  No LDS, no atomics; grid-stride.
//
// Tie / NaN rule (torch's max_pool2d, which the positions must reproduce): the window is scanned row-major, a later cell replaces the
// running maximum only when it is strictly greater or NaN.  Ties keep the first cell, the all-zero window of a dead ReLU patch
// included; a NaN, once seen, stays unless a later NaN replaces it.
//
// The backward reads p, not z: the chosen cell's ReLU is live exactly when the window's maximum p is not <= 0 (a NaN maximum counts
// as live, as in torch's threshold_backward), so the forward does not keep the convolution's output.
#include "launch_plan.h"

namespace pcg {
namespace {

constexpr unsigned POOL_MAX_BLOCKS = 8192;     // the cap of the pointwise.hip launches

struct PoolP {
  uint32_t H, W, C, Hp, Wp, C4;
  uint32_t items;                              // B * Hp * Wp * C4 work items
  FastDiv dC4, dWp, dHp;
};

// ReLU that lets a NaN through (fmaxf(0, NaN) is 0)
__device__ __forceinline__ float relu_nan(float z) { return (z > 0.f || z != z) ? z : 0.f; }

__device__ __forceinline__ void scan(float v, unsigned k, float& best, unsigned& at) {
  if (v > best || v != v) { best = v; at = k; }
}

__device__ __forceinline__ void item_coords(const PoolP& P, uint32_t i, uint32_t& b, uint32_t& ph, uint32_t& pw, uint32_t& c4) {
  uint32_t pix, t;
  P.dC4.divmod(i, pix, c4);
  P.dWp.divmod(pix, t, pw);
  P.dHp.divmod(t, b, ph);
}

__global__ void __launch_bounds__(256) relu_maxpool2_fwd_kernel(const float4* __restrict__ z, float4* __restrict__ p,
                                                                uchar4* __restrict__ idx, PoolP P) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < P.items; i += gridDim.x * 256u) {
    uint32_t b, ph, pw, c4;
    item_coords(P, i, b, ph, pw, c4);
    const size_t row0 = (((size_t)b * P.H + 2 * ph) * P.W + 2 * pw) * P.C4 + c4;     // float4 index of the window's cell (0, 0)
    const size_t row1 = row0 + (size_t)P.W * P.C4;
    const float4 v0 = z[row0], v1 = z[row0 + P.C4], v2 = z[row1], v3 = z[row1 + P.C4];
    float4 best;
    unsigned ax = 0, ay = 0, az = 0, aw = 0;
    best.x = relu_nan(v0.x); best.y = relu_nan(v0.y); best.z = relu_nan(v0.z); best.w = relu_nan(v0.w);
    scan(relu_nan(v1.x), 1, best.x, ax); scan(relu_nan(v1.y), 1, best.y, ay); scan(relu_nan(v1.z), 1, best.z, az); scan(relu_nan(v1.w), 1, best.w, aw);
    scan(relu_nan(v2.x), 2, best.x, ax); scan(relu_nan(v2.y), 2, best.y, ay); scan(relu_nan(v2.z), 2, best.z, az); scan(relu_nan(v2.w), 2, best.w, aw);
    scan(relu_nan(v3.x), 3, best.x, ax); scan(relu_nan(v3.y), 3, best.y, ay); scan(relu_nan(v3.z), 3, best.z, az); scan(relu_nan(v3.w), 3, best.w, aw);
    p[i] = best;                                                                     // p is [B][Hp][Wp][C]: item order
    idx[i] = make_uchar4((unsigned char)ax, (unsigned char)ay, (unsigned char)az, (unsigned char)aw);
  }
}

__device__ __forceinline__ float4 pick(const float4& g, const uchar4& at, unsigned k) {
  return make_float4(at.x == k ? g.x : 0.f, at.y == k ? g.y : 0.f, at.z == k ? g.z : 0.f, at.w == k ? g.w : 0.f);
}

__global__ void __launch_bounds__(256) relu_maxpool2_bwd_kernel(const float4* __restrict__ dp, const float4* __restrict__ p,
                                                                const uchar4* __restrict__ idx, float4* __restrict__ dz, PoolP P) {
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  const bool odd_h = P.H & 1u, odd_w = P.W & 1u;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < P.items; i += gridDim.x * 256u) {
    uint32_t b, ph, pw, c4;
    item_coords(P, i, b, ph, pw, c4);
    float4 g = dp[i];
    const float4 m = p[i];
    const uchar4 at = idx[i];
    g.x = m.x <= 0.f ? 0.f : g.x; g.y = m.y <= 0.f ? 0.f : g.y; g.z = m.z <= 0.f ? 0.f : g.z; g.w = m.w <= 0.f ? 0.f : g.w;
    const size_t rowlen = (size_t)P.W * P.C4;
    const size_t row0 = (((size_t)b * P.H + 2 * ph) * P.W + 2 * pw) * P.C4 + c4;
    const size_t row1 = row0 + rowlen;
    dz[row0] = pick(g, at, 0); dz[row0 + P.C4] = pick(g, at, 1);
    dz[row1] = pick(g, at, 2); dz[row1 + P.C4] = pick(g, at, 3);
    // floor mode: the last column / row of an odd W / H lies in no window.  The window beside it writes its zeros, so every element
    // of dz is stored exactly once.
    const bool last_w = odd_w && pw == P.Wp - 1, last_h = odd_h && ph == P.Hp - 1;
    if (last_w) { dz[row0 + 2 * P.C4] = zero; dz[row1 + 2 * P.C4] = zero; }
    if (last_h) {
      const size_t row2 = row1 + rowlen;
      dz[row2] = zero; dz[row2 + P.C4] = zero;
      if (last_w) dz[row2 + 2 * P.C4] = zero;
    }
  }
}

bool al16(const void* q) { return ((uintptr_t)q & 15) == 0; }

int make_params(const char* who, int32_t B, int32_t H, int32_t W, int32_t C, PoolP& P) {
  PCG_REQUIRE(B > 0 && H >= 2 && W >= 2 && C > 0, "%s: B, C must be positive and H, W at least 2 (got B=%d H=%d W=%d C=%d)", who, B, H, W, C);
  PCG_REQUIRE(C % 4 == 0, "%s: C must be a multiple of 4 (one thread owns four channels), got %d", who, C);
  PCG_REQUIRE((int64_t)B * H * W * C < ((int64_t)1 << 31), "%s: B*H*W*C must be below 2^31, got %lld", who, (long long)B * H * W * C);
  P.H = H; P.W = W; P.C = C; P.Hp = H / 2; P.Wp = W / 2; P.C4 = C / 4;
  P.items = (uint32_t)B * P.Hp * P.Wp * P.C4;
  P.dC4 = FastDiv(P.C4); P.dWp = FastDiv(P.Wp); P.dHp = FastDiv(P.Hp);
  return PCG_OK;
}

}  // namespace
}  // namespace pcg

using namespace pcg;

extern "C" int pcg_relu_maxpool2_fwd(const float* z, float* p, uint8_t* idx, int32_t B, int32_t H, int32_t W, int32_t C, pcg_stream_t stream) {
  PCG_REQUIRE(z && p && idx, "pcg_relu_maxpool2_fwd: null pointer");
  PoolP P;
  if (int e = make_params("pcg_relu_maxpool2_fwd", B, H, W, C, P)) return e;
  PCG_REQUIRE(al16(z) && al16(p) && ((uintptr_t)idx & 3) == 0, "pcg_relu_maxpool2_fwd: z, p must be 16-byte and idx 4-byte aligned");
  hipLaunchKernelGGL(relu_maxpool2_fwd_kernel, dim3(ew_grid(P.items, POOL_MAX_BLOCKS)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4*>(z), reinterpret_cast<float4*>(p), reinterpret_cast<uchar4*>(idx), P);
  return launch_status("relu_maxpool2_fwd_kernel");
}

extern "C" int pcg_relu_maxpool2_bwd(const float* dp, const float* p, const uint8_t* idx, float* dz, int32_t B, int32_t H, int32_t W, int32_t C,
                                     pcg_stream_t stream) {
  PCG_REQUIRE(dp && p && idx && dz, "pcg_relu_maxpool2_bwd: null pointer");
  PoolP P;
  if (int e = make_params("pcg_relu_maxpool2_bwd", B, H, W, C, P)) return e;
  PCG_REQUIRE(al16(dp) && al16(p) && al16(dz) && ((uintptr_t)idx & 3) == 0,
              "pcg_relu_maxpool2_bwd: dp, p, dz must be 16-byte and idx 4-byte aligned");
  hipLaunchKernelGGL(relu_maxpool2_bwd_kernel, dim3(ew_grid(P.items, POOL_MAX_BLOCKS)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4*>(dp), reinterpret_cast<const float4*>(p), reinterpret_cast<const uchar4*>(idx),
                     reinterpret_cast<float4*>(dz), P);
  return launch_status("relu_maxpool2_bwd_kernel");
}
