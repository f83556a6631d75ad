// lgs_philox.h -- the engine's one counter-based generator: Philox-4x32-10 (Salmon et al., SC'11), plain C++.
// A block is a function of (counter, key) alone, so what a kernel draws does not depend on its grid.
// Users: lgs_supcon.hip (sample indices), lgs_augment.hip (elastic noise, colour jitter), lgs_paste.hip (trial draws),
// lgs_dropout.hip (row keys), lgs_instshift.hip (per-segment decisions).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lgs {

__device__ inline void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1;
    c[3] = (uint32_t)p0;
    c[0] = n0;
    c[2] = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// one N(0, 1) sample from two 32-bit words, Box-Muller in fp32.  The radius' uniform is (w0 + 1) / 2^32 in (0, 1]: w0 + 1 is
// 1 .. 2^32 (fp32 rounds the top of the range to 2^32), so log(0) is never evaluated; the largest radius is sqrt(64 ln 2) = 6.66.
__device__ inline float philox_normal(uint32_t w0, uint32_t w1) {
  const float u1 = ((float)w0 + 1.0f) * 2.3283064365386963e-10f;
  const float u2 = (float)w1 * 2.3283064365386963e-10f;
  return sqrtf(-2.0f * logf(u1)) * cosf(6.2831853071795865f * u2);
}

}  // namespace lgs
