// The unnormalised densities an implicit sampler is fitted to (utils/energy.py: energy_func1..4 with regularization_func,
// normal_energy_func) with their analytic gradients, and the generator's output seed of notebooks/ardae_fit.ipynb built from them.
//
// One thread per row; a row is evaluated in DOUBLE and rounded once (R is a batch of ~1e3 rows: the kernel is a launch, not a load),
// so energies and gradients are the correctly rounded values of what autograd returns for the reference's functions in float64:
//   - the 1e-9 inside the logs stays: where both exponentials underflow the log term's gradient is exactly zero;
//   - relu(|x| - 6)^2 has gradient 2 relu(|x| - 6) sign(x): zero at the kink;
//   - torch.norm's (sub)gradient at the origin is zero (energy 1).
#include <algorithm>
#include <cstddef>

#include "ardae_hip.h"
#include "common.h"
#include "philox.h"
#include "profile.h"

namespace ardae {
namespace {

constexpr double LOG_EPS = 1e-9;           // utils/energy.py:5
constexpr double HALF_PI = 1.5707963267948966;
constexpr double LOG_2PI = 1.8378770664093453;

// regularization_func, one coordinate
__device__ __forceinline__ void reg_term(double x, double& E, double& g) {
#pragma clang fp contract(off)
  const double r = fabs(x) - 6.0;
  if (r > 0.0) {
    E += r * r;
    g += 2.0 * r * (x > 0.0 ? 1.0 : -1.0);
  }
}

// E and dE/dx of energy_func<kind> (without the regulariser) at (x1, x2)
// No contraction into FMAs: autograd rounds every product, and sums that cancel exactly there (A a + B b on the axis x1 = 0 of energy 1,
// where A == B and a == -b) must cancel exactly here - an FMA would leave the rounding error of one product, ~1e-16, in place of the zero.
__device__ __forceinline__ void energy2d(int kind, double x1, double x2, double& E, double& g1, double& g2) {
#pragma clang fp contract(off)
  if (kind == ARDAE_ENERGY_1) {
    const double n = sqrt(x1 * x1 + x2 * x2), t = (n - 2.0) / 0.4;
    const double a = (x1 - 2.0) / 0.6, b = (x1 + 2.0) / 0.6;
    const double A = exp(-0.5 * a * a), B = exp(-0.5 * b * b), S = A + B + LOG_EPS;
    E = 0.5 * t * t - log(S);
    const double dn = n > 0.0 ? t / (0.4 * n) : 0.0;      // torch.norm: zero gradient at the origin
    g1 = dn * x1 + (A * a + B * b) / (0.6 * S);
    g2 = dn * x2;
    return;
  }
  const double w1 = sin(HALF_PI * x1), dw1 = HALF_PI * cos(HALF_PI * x1);       // sin(2 pi x1 / 4)
  const double u = x2 - w1;
  if (kind == ARDAE_ENERGY_2) {
    E = 0.5 * (u / 0.4) * (u / 0.4);
    g2 = u / 0.16;
    g1 = -g2 * dw1;
    return;
  }
  double sa, w, dw;                                        // first mode's width; second mode's offset and its derivative
  if (kind == ARDAE_ENERGY_3) {
    const double q = (x1 - 1.0) / 0.6;
    sa = 0.35;
    w = 3.0 * exp(-0.5 * q * q);
    dw = -w * q / 0.6;
  } else {
    const double s = 1.0 / (1.0 + exp(-(x1 - 1.0) / 0.3));
    sa = 0.4;
    w = 3.0 * s;
    dw = 3.0 * s * (1.0 - s) / 0.3;
  }
  const double a = u / sa, b = (u + w) / 0.35;
  const double A = exp(-0.5 * a * a), B = exp(-0.5 * b * b), S = A + B + LOG_EPS;
  E = -log(S);
  const double Aa = A * a / sa, Bb = B * b / 0.35;         // -dA/du, -dB/du
  g2 = (Aa + Bb) / S;
  g1 = (Aa * -dw1 + Bb * (dw - dw1)) / S;
}

// out: dE/dx, or (SEED) (alpha dE/dx + score) / R - the three operations rounded separately
template <bool SEED>
__device__ __forceinline__ void emit(float* out, size_t i, double g, const float* score, float alpha, float Rf) {
#pragma clang fp contract(off)
  if (SEED) {      // plain operators: under the pragma none of them is contracted (the __f*_rn wrappers' own bodies are not under it)
    const float ag = alpha * (float)g;
    const float sum = ag + score[i];
    out[i] = sum / Rf;
  }
  else if (out) out[i] = (float)g;
}

// SEED: also partial[block] = the block's energy sum (tree order fixed by the thread index)
template <bool SEED>
__global__ __launch_bounds__(256) void energy_kernel(int kind, const float* __restrict__ x, int R, int d, float mu, float logvar,
                                                     const float* __restrict__ score, float alpha, const FitState* __restrict__ fs,
                                                     float* __restrict__ energy, float* __restrict__ out, double* __restrict__ partial) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (SEED && fs) alpha = fs->alpha;
  const float Rf = (float)R;
  double E = 0.0;
  if (r < R) {
    const size_t i0 = (size_t)r * d;
    if (kind >= ARDAE_ENERGY_1 && kind <= ARDAE_ENERGY_4) {
      const double x1 = x[i0], x2 = x[i0 + 1];
      double g1, g2;
      energy2d(kind, x1, x2, E, g1, g2);
      reg_term(x1, E, g1);
      reg_term(x2, E, g2);
      emit<SEED>(out, i0, g1, score, alpha, Rf);
      emit<SEED>(out, i0 + 1, g2, score, alpha, Rf);
    } else if (kind == ARDAE_ENERGY_NORMAL) {
      const double var = exp((double)logvar);
      for (int k = 0; k < d; ++k) {
        const double c = (double)x[i0 + k] - (double)mu;
        E += 0.5 * ((double)logvar + c * c / var + LOG_2PI);
        emit<SEED>(out, i0 + k, c / var, score, alpha, Rf);
      }
    } else {      // ARDAE_ENERGY_REG
      for (int k = 0; k < d; ++k) {
        double g = 0.0;
        reg_term((double)x[i0 + k], E, g);
        emit<SEED>(out, i0 + k, g, score, alpha, Rf);
      }
    }
    if (energy) energy[r] = (float)E;
  }
  if (SEED) {
    __shared__ double red[256];
    red[threadIdx.x] = E;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
  }
}

// mean[0] = (sum of the nb block sums) / R: thread t adds partials t, t + 256, ... in ascending order, then the same tree
__global__ __launch_bounds__(256) void energy_mean_kernel(const double* __restrict__ partial, int nb, int R, float* __restrict__ mean) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) s += partial[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) mean[0] = (float)(red[0] / (double)R);
}

int check(const char* what, int kind, const float* x, int R, int d) {
  ARDAE_CHECK_ARG(kind >= ARDAE_ENERGY_REG && kind <= ARDAE_ENERGY_NORMAL, "%s: unknown energy %d", what, kind);
  ARDAE_CHECK_ARG(x != nullptr, "%s: null pointer argument", what);
  ARDAE_CHECK_ARG(R > 0 && d > 0 && (int64_t)R * d < (int64_t)1 << 31, "%s: bad batch (R=%d, d=%d)", what, R, d);
  ARDAE_CHECK_ARG(kind < ARDAE_ENERGY_1 || kind > ARDAE_ENERGY_4 || d == 2, "%s: energy_func%d is defined on [R, 2] (got d=%d)", what, kind, d);
  return 0;
}

}  // namespace
}  // namespace ardae

using namespace ardae;

extern "C" {

int ardae_energy(int kind, const float* x, int R, int d, float mu, float logvar, float* energy, float* grad, void* stream) {
  ARDAE_TRY(check("energy", kind, x, R, d));
  const hipStream_t st = (hipStream_t)stream;
  prof_begin(st, "energy_kernel", 60.0 * R, 4.0 * R * (2.0 * d + 1.0));
  hipLaunchKernelGGL(energy_kernel<false>, dim3((unsigned)ceil_div(R, 256)), dim3(256), 0, st, kind, x, R, d, mu, logvar, (const float*)nullptr, 0.f,
                     (const FitState*)nullptr, energy, grad, (double*)nullptr);
  prof_end(st);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

size_t ardae_energy_partial_floats(int R) { return R > 0 ? 2 * (size_t)ceil_div(R, 256) : 0; }

int ardae_energy_seed(int kind, const float* x, const float* score, int R, int d, float mu, float logvar, float alpha, const void* fit_state,
                      float* seed, float* mean_energy, float* partial, void* stream) {
  ARDAE_TRY(check("energy_seed", kind, x, R, d));
  ARDAE_CHECK_ARG(score && seed && mean_energy && partial, "energy_seed: null pointer argument");
  ARDAE_CHECK_ARG((reinterpret_cast<uintptr_t>(partial) & 7) == 0, "energy_seed: partial must be 8-byte aligned (it holds doubles)");
  const hipStream_t st = (hipStream_t)stream;
  const int nb = ceil_div(R, 256);
  prof_begin(st, "energy_seed_kernel", 60.0 * R, 4.0 * R * 3.0 * d);
  hipLaunchKernelGGL(energy_kernel<true>, dim3((unsigned)nb), dim3(256), 0, st, kind, x, R, d, mu, logvar, score, alpha, (const FitState*)fit_state,
                     (float*)nullptr, seed, reinterpret_cast<double*>(partial));
  prof_end(st);
  ARDAE_LAUNCH_CHECK();
  prof_begin(st, "energy_mean_kernel", (double)nb, 8.0 * nb + 4.0);
  hipLaunchKernelGGL(energy_mean_kernel, dim3(1), dim3(256), 0, st, reinterpret_cast<const double*>(partial), nb, R, mean_energy);
  prof_end(st);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
