// What makes the generator's update of notebooks/ardae_fit.ipynb replayable: torch.optim.Adam reading its coefficients from the device,
// and the kernel that advances the fit state - Adam's t, the StepLR learning rate, the annealed energy weight - once per iteration.
#include <algorithm>
#include <cstddef>

#include "ardae_hip.h"
#include "common.h"
#include "philox.h"

// the layout include/ardae_hip.h promises: the step state's 32 bytes first (its *_dev consumers read the head), alpha / lr behind them
static_assert(sizeof(ardae::FitState) == ARDAE_FIT_STATE_BYTES && offsetof(ardae::FitState, alpha) == ARDAE_STEP_STATE_BYTES &&
                  sizeof(ardae::StepState) <= ARDAE_STEP_STATE_BYTES,
              "fit state layout");

namespace ardae {
namespace {

// torch.optim.Adam (torch/optim/adam.py, _single_tensor_adam): lerp, addcmul, sqrt / sqrt(bc2) + eps, addcdiv
__global__ void adam_torch_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t n,
                                  float w, float beta2, float omb2, float eps, const StepState* __restrict__ state) {
  // w = 1 - beta1 and omb2 = 1 - beta2 are formed in double and rounded once, as the Python scalars torch passes to lerp_ / addcmul_ are
  const float step_size = state->adam_step_size, sqrt_bc2 = state->adam_sqrt_bc2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float gi = g[i], m0 = m[i];
    const float diff = gi - m0;
    const float mi = w < 0.5f ? m0 + w * diff : gi - diff * (1.f - w);     // Tensor.lerp_'s two branches
    const float vi = v[i] * beta2 + omb2 * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / sqrt_bc2 + eps;                       // eps AFTER the bias correction
    p[i] = p[i] - step_size * (mi / denom);
  }
}

__global__ void fit_state_advance_kernel(FitState* s, uint64_t rng_inc, double lr0, double beta1, double beta2, int64_t lr_step_size, double lr_gamma,
                                         double lr_min, double alpha_init, double alpha_fin, int64_t alpha_annealing) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  s->alpha_done = s->alpha;
  s->lr_done = s->lr;
  s->step.rng_offset += rng_inc;
  const int64_t t = s->step.adam_step + 1, i = t - 1;
  s->step.adam_step = t;
  const double lr = fmax(lr_min, lr0 * pow(lr_gamma, (double)(i / lr_step_size)));
  const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
  s->step.adam_step_size = (float)(lr / bc1);
  s->step.adam_sqrt_bc2 = (float)sqrt(bc2);
  s->lr = (float)lr;
  const double alpha = alpha_annealing < 0 ? alpha_fin
                                           : alpha_init + (alpha_fin - alpha_init) / (double)alpha_annealing * (double)(i < alpha_annealing ? i : alpha_annealing);
  s->alpha = (float)alpha;
}

}  // namespace
}  // namespace ardae

using namespace ardae;

extern "C" {

int ardae_adam_torch_step_dev(float* p, const float* g, float* exp_avg, float* exp_avg_sq, int64_t n, double beta1, double beta2, double eps,
                              const void* state, void* stream) {
  ARDAE_CHECK_ARG(p && g && exp_avg && exp_avg_sq && n > 0 && state, "adam_torch_step_dev: bad arguments");
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(adam_torch_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, exp_avg, exp_avg_sq, n, (float)(1.0 - beta1),
                     (float)beta2, (float)(1.0 - beta2), (float)eps, (const StepState*)state);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

int ardae_fit_state_advance(void* fit_state, uint64_t rng_inc, double lr0, double beta1, double beta2, int64_t lr_step_size, double lr_gamma,
                            double lr_min, double alpha_init, double alpha_fin, int64_t alpha_annealing, void* stream) {
  ARDAE_CHECK_ARG(fit_state, "fit_state_advance: null state");
  ARDAE_CHECK_ARG(lr_step_size >= 1, "fit_state_advance: lr_step_size must be >= 1 (got %lld)", (long long)lr_step_size);
  ARDAE_CHECK_ARG(alpha_annealing != 0, "fit_state_advance: alpha_annealing must be positive, or negative for none");
  hipLaunchKernelGGL(fit_state_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (FitState*)fit_state, rng_inc, lr0, beta1, beta2,
                     lr_step_size, lr_gamma, lr_min, alpha_init, alpha_fin, alpha_annealing);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
