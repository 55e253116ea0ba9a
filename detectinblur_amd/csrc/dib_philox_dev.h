// The counter-based normal generator of the noise kernels (dib_postops.hip, dib_deblur_augment.hip): a pure function of (key, element
// index), so a noise field does not depend on the launch geometry or on the order in which elements are visited.
// oracle/dib_oracle.py restates it (philox4x32_10, normal64); tests/test_postops_reference.py holds the kernels' values to that: change
// nothing here without both.
#pragma once
#include <hip/hip_runtime.h>

namespace dib {

__device__ __forceinline__ void philox_round(unsigned (&c)[4], unsigned k0, unsigned k1) {
  const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
  const unsigned hi0 = (unsigned)(p0 >> 32), lo0 = (unsigned)p0, hi1 = (unsigned)(p1 >> 32), lo1 = (unsigned)p1;
  c[0] = hi1 ^ c[1] ^ k0; c[1] = lo1; c[2] = hi0 ^ c[3] ^ k1; c[3] = lo0;
}

// One standard normal per (seed, index): Philox-4x32-10 on counter (index, 0, 0, 0), Box-Muller on its first two words.
__device__ __forceinline__ float normal_at(unsigned long long index, unsigned k0, unsigned k1) {
  unsigned c[4] = {(unsigned)index, (unsigned)(index >> 32), 0u, 0u};
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  const float u1 = ((float)(c[0] >> 8) + 0.5f) * (1.0f / 16777216.0f);     // (0, 1)
  const float u2 = ((float)(c[1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
  return sqrtf(-2.0f * __logf(u1)) * __cosf(6.28318530717958647692f * u2);
}

}  // namespace dib
