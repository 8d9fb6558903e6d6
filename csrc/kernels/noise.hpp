// The per-element update of ``dst += coef*upd (+ N(0, sigma))`` shared by flat.hip noise_add_kernel
// (plain FedAvg and every defence that ends in ops.add_noise_scaled) and rlr.hip rlr_apply_kernel
// (the robust learning rate: the same update with -coef at the flipped coordinates).  One
// definition, so the compiler contracts the noise expression the same way in both and a kept /
// flipped coordinate gets the bits of dba_add_noise_scaled with +coef / -coef.
#pragma once
#include "common.hpp"

// (float)(upd * coef) (+ sigma * N(0, 1) from the hash RNG at counters 2 i, 2 i + 1 if ``noise``)
template <typename U>
__device__ __forceinline__ float noise_scaled_update(U upd, float coef, float sigma, uint32_t seed, int noise,
                                                     long long i) {
  float u = (float)(upd * (U)coef);
  if (noise) {
    const uint32_t c = (uint32_t)(i * 2);
    const float u1 = uniform01(seed, c), u2 = uniform01(seed, c + 1);
    u += sigma * sqrtf(-2.0f * __logf(u1)) * __cosf(6.283185307179586f * u2);
  }
  return u;
}
