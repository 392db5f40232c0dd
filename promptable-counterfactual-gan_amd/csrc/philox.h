// philox.h — the counter-based Philox-4x32-10 stream of the device draws (rng.hip, delta_cf_eval.hip; counter layout and spans in
// DESIGN.md §3.14, host model oracle/rng_np.py).  Counter value c = offset + idx gives four 32-bit words.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace pcg {
namespace {

struct U4 { uint32_t x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(U4 ctr, uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, ctr.x), lo0 = M0 * ctr.x;
    const uint32_t hi1 = __umulhi(M1, ctr.z), lo1 = M1 * ctr.z;
    ctr = U4{hi1 ^ ctr.y ^ k0, lo1, hi0 ^ ctr.w ^ k1, lo0};
    k0 += W0; k1 += W1;
  }
  return ctr;
}
__device__ __forceinline__ U4 draw(uint64_t seed, uint64_t offset, uint64_t idx) {
  const uint64_t c = offset + idx;
  return philox4x32_10(U4{(uint32_t)c, (uint32_t)(c >> 32), 0x5eed5eedu, 0u}, (uint32_t)seed, (uint32_t)(seed >> 32));
}

}  // namespace
}  // namespace pcg
