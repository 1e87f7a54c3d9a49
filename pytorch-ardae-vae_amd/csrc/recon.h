// The reconstruction DAEs' perturbation (models/dae/mlp.py:12-18): the ONE definition of x_bar, shared by the unfused kernels and the ones
// that draw for themselves (recon_dae.hip), so both forms give the same bits.
#pragma once
#include "common.h"
#include "philox.h"

namespace ardae {

enum ReconNoise : int { RECON_GAUSSIAN = 0, RECON_UNIFORM = 1 };

// x_bar from the clean value u, the raw draw (a standard normal, or a uniform in [0, 1)) and the noise level s.
//   gaussian (add_gaussian_noise): x + std * eps as one fma, as every other perturbation of this library
//   uniform (add_uniform_noise): eps = 2 val u - val; x + eps - every operation rounded on its own, in the reference's order
__device__ __forceinline__ float recon_xbar(float u, float draw, float s, int noise) {
  if (noise == RECON_GAUSSIAN) return __builtin_fmaf(s, draw, u);
  {
#pragma clang fp contract(off)
    const float two_s = 2.f * s;
    const float scaled = two_s * draw;
    const float e = scaled - s;
    return u + e;
  }
}

// the four [0, 1) uniforms of Philox counter `idx`: the map of philox_uniform_kernel (elementwise.hip), (word >> 8) 2^-24
__device__ __forceinline__ void philox_uniform4(uint64_t seed, uint64_t offset, uint64_t idx, float v[4]) {
  uint32_t r[4];
  philox4(seed, offset, idx, r);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = (r[i] >> 8) * (1.0f / 16777216.0f);
}

}  // namespace ardae
