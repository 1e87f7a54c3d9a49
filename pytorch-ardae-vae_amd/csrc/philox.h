// Philox4x32-10 counter RNG and the device-resident step state: the ONE definition of a draw, shared by the stand-alone draw
// kernels (elementwise.hip) and the kernels that draw for themselves (elementwise.hip, dae_perturb.hip).
#pragma once
#include "common.h"

namespace ardae {

// ------------------------------------------------------------------------------------------ Philox4x32-10
struct Philox {
  uint32_t c[4];
  uint32_t k[2];
};
__device__ __forceinline__ void philox_round(Philox& s) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  const uint32_t hi0 = __umulhi(M0, s.c[0]), lo0 = M0 * s.c[0];
  const uint32_t hi1 = __umulhi(M1, s.c[2]), lo1 = M1 * s.c[2];
  const uint32_t n0 = hi1 ^ s.c[1] ^ s.k[0], n1 = lo1, n2 = hi0 ^ s.c[3] ^ s.k[1], n3 = lo0;
  s.c[0] = n0; s.c[1] = n1; s.c[2] = n2; s.c[3] = n3;
  s.k[0] += 0x9E3779B9u;
  s.k[1] += 0xBB67AE85u;
}
__device__ __forceinline__ void philox4(uint64_t seed, uint64_t offset, uint64_t idx, uint32_t out[4]) {
  Philox s;
  s.c[0] = (uint32_t)idx; s.c[1] = (uint32_t)(idx >> 32);
  s.c[2] = (uint32_t)offset; s.c[3] = (uint32_t)(offset >> 32);
  s.k[0] = (uint32_t)seed; s.k[1] = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) philox_round(s);
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = s.c[i];
}
__device__ __forceinline__ float u01_open(uint32_t x) { return ((x >> 8) + 1u) * (1.0f / 16777216.0f); }  // (0,1]
// the four standard normals of Philox counter `idx` (Box-Muller on the two word pairs): the ONE definition every draw uses -
// the stand-alone kernel and the draws fused into their consumers give the same numbers for the same (seed, offset, element)
__device__ __forceinline__ void philox_normal4(uint64_t seed, uint64_t offset, uint64_t idx, float v[4]) {
  uint32_t r[4];
  philox4(seed, offset, idx, r);
  // Box-Muller on the hardware transcendental units (round 4): v_log_f32 is log2, v_sin_f32 / v_cos_f32 take their argument in
  // REVOLUTIONS, so sin(2 pi u) is one instruction with no range reduction.  ~12 vector-ALU instructions per pair instead of the ~150
  // of logf + sincosf (the draws fused into latent_perturb_reg_kernel made that kernel issue-bound: SQ_WAIT_INST_ANY = a third of its
  // wave cycles).  Absolute accuracy ~1e-6 (measured against float64 Box-Muller on the same words: worst of 2^20 normals 6.9e-7, three to
  // four ulps of the radius at any angle; tests/test_philox_gpu.py bounds every draw by 4 x that) - these are noise samples; what matters
  // is that EVERY draw uses this one definition.
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float rad = __builtin_amdgcn_sqrtf(-1.38629436111989062f * __builtin_amdgcn_logf(u01_open(r[2 * h])));      // sqrt(-2 ln u)
    const float rev = u01_open(r[2 * h + 1]);
    v[2 * h] = rad * __builtin_amdgcn_cosf(rev);
    v[2 * h + 1] = rad * __builtin_amdgcn_sinf(rev);
  }
}

// Device-resident step state (ardae_step_state_advance): lets a captured HIP graph replay the step with fresh noise and
// the right Adam bias correction - kernel arguments are frozen at capture, this block is not.
struct StepState {
  uint64_t rng_offset;     // base offset of this step's Philox draws
  int64_t adam_step;       // t of utils/optim.py:84
  float adam_step_size;    // lr / (1 - beta1^t)
  float adam_sqrt_bc2;     // sqrt(1 - beta2^t)
};

// The train state (ardae_train_state_advance): the step state with the KL weight and the entropy-seed factor of the coming step in
// the block's last 8 bytes (FitState::reserved; no step-state consumer reads them).
struct TrainState {
  StepState step;
  float beta;              // annealing_func(beta_init, beta_fin, beta_annealing, t - 1)
  float seed_scale;        // std_scale * beta / seed_rows
};
static_assert(sizeof(TrainState) == 32, "the train state fills ARDAE_STEP_STATE_BYTES");

// The DAE state (ardae_dae_state_advance): the step state with the noise level of the coming step of notebooks/dae_toy.ipynb in the
// train state's beta slot.
struct DaeState {
  StepState step;
  float sigma;             // sigma_max (1 - perc) + sigma_min perc, perc = min(t / sigma_annealing, 1)
  float pad;
};
static_assert(sizeof(DaeState) == 32, "the DAE state fills ARDAE_STEP_STATE_BYTES");

// The fit state (ardae_fit_state_advance): a step state whose Adam coefficients follow the StepLR schedule, and behind it the
// energy weight and learning rate of the coming iteration and of the one just done (the logged pair).
struct FitState {
  StepState step;
  uint64_t reserved;           // the step state block is 32 bytes (ARDAE_STEP_STATE_BYTES), 24 of them used
  float alpha, lr;             // the coming iteration's
  float alpha_done, lr_done;   // the last finished iteration's
};

}  // namespace ardae
