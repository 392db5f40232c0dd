// epoch_wg.h — what the "whole training epoch in ONE launch of ONE workgroup" kernels share (moons_cf.hip: DESIGN.md §3.8,
// moons_gan.hip: §3.10), and the torch-exact Adam element update that pointwise.hip's adam_kernel applies as well.
// ONE definition of each: a fused launch, the eager optimizer step that continues after it and the op chain the tests compare it
// with must agree bit for bit.  What differs between the kernels stays in them: thread counts, LDS layouts, the loops over the
// register-resident moments, and how beta^t is formed (adam_corr takes that as a function).
#pragma once
#include "pcg_common.h"

#include <math.h>

namespace pcg {

constexpr size_t LDS_CAP = 160 * 1024;                    // the CU's LDS

__host__ __device__ constexpr int r4(int n) { return (n + 3) & ~3; }

__device__ __forceinline__ float wave_sum(float v) {
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

// ---- Adam -------------------------------------------------------------------------------------------------------------------------
struct AdamK { float w1, one_minus_w1, beta2, one_minus_beta2, eps; };

// The weights are formed in double (as Python does) and rounded to fp32 once.
__host__ __device__ __forceinline__ AdamK adam_k(double beta1, double beta2, double eps) {
  return AdamK{(float)(1.0 - beta1), (float)(1.0 - (1.0 - beta1)), (float)beta2, (float)(1.0 - beta2), (float)eps};
}
template <class Desc>                                      // a kernel descriptor with beta1, beta2, adam_eps
__device__ __forceinline__ AdamK adam_k(const Desc& d) { return adam_k(d.beta1, d.beta2, d.adam_eps); }

// One element, no weight decay (pointwise.hip's adam_one applies that first): torch's lerp / addcmul / bias-corrected step.
// [torch] exp_avg.lerp_(grad, 1-beta1): weight < 0.5 ? a + w(b-a) : b - (b-a)(1-w)
__device__ __forceinline__ void adam_upd(float& p, float g, float& m, float& v, const AdamK& k, float step_size, float bc2_sqrt) {
  m = (k.w1 < 0.5f) ? fmaf(k.w1, g - m, m) : g - (g - m) * k.one_minus_w1;
  v = fmaf(v, k.beta2, k.one_minus_beta2 * g * g);
  const float denom = sqrtf(v) / bc2_sqrt + k.eps;
  p = p - step_size * (m / denom);
}

// pcg_adam_step_capturable's bias corrections for step t: step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t).
// power(beta, t) is the kernel's own way to beta^t (they differ, and a last bit of the result may: DESIGN.md §3.8).  It is called
// here, between the other fp64 operations as before, and not passed in as two values: that order is what keeps moons_cf's
// register allocation (it spills) as it was.
template <class Pow>
__device__ __forceinline__ void adam_corr(double lr, double beta1, double beta2, int64_t t, Pow power, float& step_size, float& bc2_sqrt) {
  const double bc1 = 1.0 - power(beta1, t);
  bc2_sqrt = (float)sqrt(1.0 - power(beta2, t));
  step_size = (float)(lr / bc1);
}

// ---- host: LDS budget and the launch ---------------------------------------------------------------------------------------------
inline bool acts_fit_lds(size_t fixed, size_t act) { return fixed + act <= LDS_CAP; }

// The fixed LDS state must fit; the activations follow it in LDS when they fit too, else the caller's scratch must hold them
// (`align`-byte aligned).  lds: the launch's dynamic LDS size.  `who` names the entry point in the error text.
inline int place_acts(const char* who, size_t fixed, size_t act, const void* scratch, size_t scratch_bytes, size_t align, bool& in_lds,
                      size_t& lds) {
  in_lds = acts_fit_lds(fixed, act);
  PCG_REQUIRE(fixed <= LDS_CAP, "%s: %zu bytes of LDS state exceed the CU's", who, fixed);
  if (!in_lds) PCG_REQUIRE(scratch && scratch_bytes >= act && ((uintptr_t)scratch & (align - 1)) == 0,
                           "%s: scratch %zu bytes < %zu needed (%zu-byte aligned)", who, scratch_bytes, act, align);
  lds = fixed + (in_lds ? act : 0);
  return PCG_OK;
}

// One workgroup of nt threads with `lds` bytes of dynamic LDS (above the 64 KB default: the attribute has to be raised first).
template <class... P, class... A>
int launch_one_wg(void (*kernel)(P...), const char* name, int nt, size_t lds, hipStream_t s, A... args) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) { set_error("hipFuncSetAttribute(max dynamic LDS=%zu): %s", lds, hipGetErrorString(e)); return PCG_ERR_LAUNCH; }
  hipLaunchKernelGGL(kernel, dim3(1), dim3(nt), lds, s, args...);
  return launch_status(name);
}

}  // namespace pcg
