// Front end of the unconditional AR-DAE update (ardae_cdae_desc.kind 2 / 3): the perturbation of a broadcast batch, and the same with
// its two draws and the score network's first layer in one kernel.  And the plain DAE's perturbation (kind 6 / 7, notebooks/dae_toy.ipynb):
// one noise level for the whole batch, a value or the DAE state's.  And the plain conditional DAE's (kind 10 / 11): the same one noise level on
// the centred, scaled latent samples of ivae_ardae.py:753-767, with the eps draw read or made in the kernel.
//
// Reference: the training cells of notebooks/ardae_toy.ipynb / ardae_fit.ipynb (x.unsqueeze(1).expand(B, nsigma, d).contiguous(),
// std = delta * randn) and add_gaussian_noise (models/graddae/mlp.py:21-23).  Row (b, j) reads x[b]: the broadcast is never written.
#include <algorithm>

#include "ardae_hip.h"
#include "common.h"
#include "elementwise.h"
#include "front_layer.h"
#include "philox.h"
#include "profile.h"

namespace ardae {

// cdae.hip
int dae_front_slots(const ardae_cdae_desc* d, int N, float* workspace, size_t ws_floats, size_t* w1, size_t* b1, float** h1);
int dae_loss_grads_from_h1(const ardae_cdae_desc* d, const float* params, const float* packed, const float* xbar, const float* sigma, const float* eps,
                           int N, float* workspace, size_t ws_floats, float* loss, float* grads, hipStream_t st);

namespace {

constexpr int DP_ROWS = FRONT_ROWS;   // rows per workgroup of the fused kernel
constexpr int DP_DMAX = 8;    // widest input it takes as plain FMAs

__global__ __launch_bounds__(256) void dae_perturb_kernel(const float* __restrict__ x, const float* __restrict__ sigma, const float* __restrict__ eps,
                                                          int64_t n, int nsigma, int d, float* __restrict__ xbar) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = e / d;
    const int k = (int)(e - row * d);
    xbar[e] = __builtin_fmaf(sigma[row], eps[e], x[(row / nsigma) * d + k]);
  }
}

// The plain DAE's perturbation: one noise level s for every row (sp non-null: the device block's, one wave-uniform load)
__global__ __launch_bounds__(256) void dae_noise_perturb_kernel(const float* __restrict__ x, const float* __restrict__ eps, int64_t n, int nsigma, int d,
                                                                float sv, const float* __restrict__ sp, float* __restrict__ xbar,
                                                                float* __restrict__ sigma_out) {
  const float s = sp ? *sp : sv;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = e / d;
    const int k = (int)(e - row * d);
    xbar[e] = __builtin_fmaf(s, eps[e], x[(row / nsigma) * d + k]);
    if (k == 0) sigma_out[row] = s;
  }
}

// The plain conditional DAE's perturbation (the one-noise-level counterpart of latent_perturb_kernel): row (b, i, j) of the B * nz * nstd rows reads
// latent[b, i]; u = std_scale (latent - z0[b]) is rounded as center_scale_kernel rounds it, then xbar = fma(s, eps, u).
__device__ __forceinline__ float latent_noise_xbar(const float* __restrict__ latent, const float* __restrict__ z0, int64_t row, int k, int nz, int nstd,
                                                   int zd, float std_scale, float s, float ep) {
  const int64_t src = row / nstd;
  const float u = std_scale * (latent[src * zd + k] - z0[(src / nz) * zd + k]);
  return __builtin_fmaf(s, ep, u);
}

__global__ __launch_bounds__(256) void latent_noise_perturb_kernel(const float* __restrict__ latent, const float* __restrict__ z0,
                                                                   const float* __restrict__ eps, int64_t n, int nz, int nstd, int zd, float std_scale,
                                                                   float sv, const float* __restrict__ sp, float* __restrict__ xbar,
                                                                   float* __restrict__ sigma_out) {
  const float s = sp ? *sp : sv;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = e / zd;
    const int k = (int)(e - row * zd);
    xbar[e] = latent_noise_xbar(latent, z0, row, k, nz, nstd, zd, std_scale, s, eps[e]);
    if (k == 0) sigma_out[row] = s;
  }
}

// The same with eps made here.  One workgroup per tile of LN_ROWS rows = 16 zd Philox counters; a thread takes counters t, t + 256, ... of its
// tile, i.e. four consecutive elements of the [N, zd] draw each, keyed exactly like ardae_philox_normal_at (element i of the call's rows = element
// first_row zd + i of the draw (seed, off_eps + the block's base offset)).  Rows at or beyond N (a last partial tile) draw and write nothing.
constexpr int LN_ROWS = 64;
__global__ __launch_bounds__(256) void latent_noise_perturb_draw_kernel(const float* __restrict__ latent, const float* __restrict__ z0, int N, int nz,
                                                                        int nstd, int zd, float std_scale, float sv, const DaeState* __restrict__ state,
                                                                        uint64_t seed, uint64_t off_eps, uint64_t first_row,
                                                                        float* __restrict__ xbar, float* __restrict__ sigma_out,
                                                                        float* __restrict__ eps_out, int vec_ok) {
  const float s = state ? state->sigma : sv;
  const uint64_t base_off = state ? state->step.rng_offset : 0;
  const int64_t row0 = (int64_t)blockIdx.x * LN_ROWS;
  const int64_t n = (int64_t)N * zd, e0 = row0 * zd;
  const uint64_t q0 = ((first_row + (uint64_t)row0) * (uint64_t)zd) >> 2;     // first_row and LN_ROWS are multiples of 4
  for (int c = threadIdx.x; c < (LN_ROWS / 4) * zd; c += 256) {
    const int64_t e = e0 + 4 * (int64_t)c;
    if (e >= n) break;
    float v[4], xb[4];
    philox_normal4(seed, off_eps + base_off, q0 + (uint64_t)c, v);
    const int lim = n - e < 4 ? (int)(n - e) : 4;
    for (int i = 0; i < lim; ++i) {
      const int64_t row = (e + i) / zd;
      const int k = (int)(e + i - row * zd);
      xb[i] = latent_noise_xbar(latent, z0, row, k, nz, nstd, zd, std_scale, s, v[i]);
      if (k == 0) sigma_out[row] = s;
    }
    if (lim == 4 && vec_ok) {
      *reinterpret_cast<f32x4*>(xbar + e) = f32x4{xb[0], xb[1], xb[2], xb[3]};
      *reinterpret_cast<f32x4*>(eps_out + e) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
      for (int i = 0; i < lim; ++i) { xbar[e + i] = xb[i]; eps_out[e + i] = v[i]; }
    }
  }
}

// One workgroup per tile of 64 rows.  Phase 1: the tile's Philox counters (16 d of the eps draw, 16 of the sigma draw: at most 144 of the
// 256 threads hold one), then sigma = delta n, xbar = fma(sigma, eps, x[b]) - written out, and kept in LDS.  Phase 2: h_1 =
// act(W1x xbar + sigma w1s + d_1), front_layer.h::front_first_layer (shared with the generator's front end, generator.hip).
// Rows at or beyond N (a last partial tile) draw like the others and write nothing.
__global__ __launch_bounds__(256) void dae_perturb_fwd_kernel(const float* __restrict__ x, int N, int nsigma, int d, float delta, uint64_t seed,
                                                              uint64_t off_sigma, uint64_t off_eps, const StepState* __restrict__ state,
                                                              uint64_t first_row, float* __restrict__ xbar, float* __restrict__ sigma,
                                                              float* __restrict__ eps_out, const float* __restrict__ W1,
                                                              const float* __restrict__ b1, int h, int act, float* __restrict__ h1) {
  __shared__ __attribute__((aligned(16))) float neps[DP_ROWS * DP_DMAX];
  __shared__ __attribute__((aligned(16))) float nsig[DP_ROWS];
  __shared__ float xb[DP_ROWS * DP_DMAX];
  __shared__ float sg[DP_ROWS];
  const int t = threadIdx.x;
  const int row0 = blockIdx.x * DP_ROWS;
  const uint64_t base_off = state ? state->rng_offset : 0;
  const uint64_t r_first = first_row + (uint64_t)row0;   // a multiple of 4
  if (t < 16 * d) {
    float v[4];
    philox_normal4(seed, off_eps + base_off, ((r_first * (uint64_t)d) >> 2) + (uint64_t)t, v);
    *reinterpret_cast<f32x4*>(neps + 4 * t) = f32x4{v[0], v[1], v[2], v[3]};
  } else if (t < 16 * d + 16) {
    const int c = t - 16 * d;
    float v[4];
    philox_normal4(seed, off_sigma + base_off, (r_first >> 2) + (uint64_t)c, v);
    *reinterpret_cast<f32x4*>(nsig + 4 * c) = f32x4{v[0], v[1], v[2], v[3]};
  }
  __syncthreads();
  for (int e = t; e < DP_ROWS * d; e += 256) {
    const int r = e / d, k = e - r * d;
    const int row = row0 + r;
    float s = 0.f, xv = 0.f;
    if (row < N) {
      s = delta * nsig[r];
      const float ep = neps[e];
      xv = __builtin_fmaf(s, ep, x[(size_t)(row / nsigma) * d + k]);
      xbar[(size_t)row * d + k] = xv;
      eps_out[(size_t)row * d + k] = ep;
      if (k == 0) sigma[row] = s;
    }
    xb[e] = xv;
    if (k == 0) sg[r] = s;
  }
  __syncthreads();
  front_first_layer<DP_DMAX, true>(xb, sg, d, row0, N, W1, d + 1, b1, h, act, h1);
}

bool fused_shape_ok(const ardae_cdae_desc* d, int nsigma) {
  return d && (d->kind == 2 || d->kind == 3) && d->context_dim == 0 && d->input_dim >= 1 && d->input_dim <= DP_DMAX &&
         (d->h_dim == 64 || d->h_dim == 128 || d->h_dim == 256) && d->n_layers >= 2 && d->n_layers <= 6 && d->act > ACT_NONE &&
         d->act <= ACT_LAST && nsigma >= 1;
}

}  // namespace
}  // namespace ardae

using namespace ardae;

extern "C" {

int ardae_dae_perturb(const float* x, const float* sigma, const float* eps, int B, int nsigma, int d, float* xbar, void* stream) {
  ARDAE_CHECK_ARG(x && sigma && eps && xbar, "dae_perturb: null pointer argument");
  ARDAE_CHECK_ARG(B > 0 && nsigma > 0 && d > 0 && (int64_t)B * nsigma * d < (int64_t)1 << 31, "dae_perturb: bad batch (B=%d, nsigma=%d, d=%d)", B,
                  nsigma, d);
  const int64_t n = (int64_t)B * nsigma * d;
  const hipStream_t st = (hipStream_t)stream;
  prof_begin(st, "dae_perturb_kernel", 2.0 * (double)n, 4.0 * (2.0 * (double)n + (double)B * nsigma + (double)B * d));
  hipLaunchKernelGGL(dae_perturb_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, st, x, sigma, eps, n, nsigma, d,
                     xbar);
  prof_end(st);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

int ardae_dae_perturb_fused_ok(const ardae_cdae_desc* d, int nsigma) { return fused_shape_ok(d, nsigma) ? 1 : 0; }

int ardae_dae_perturb_loss_grads(const ardae_cdae_desc* d, const float* params, const float* packed, const float* x, int B, int nsigma,
                                 float delta, uint64_t seed, uint64_t offset_sigma, uint64_t offset_eps, const void* state,
                                 uint64_t first_row, float* xbar, float* sigma, float* eps_out, float* workspace,
                                 size_t workspace_floats, float* loss, float* grads, void* stream) {
  ARDAE_CHECK_ARG(d != nullptr, "dae_perturb_loss_grads: desc is NULL");
  ARDAE_CHECK_ARG(B > 0 && nsigma > 0 && (int64_t)B * nsigma < (int64_t)1 << 30, "dae_perturb_loss_grads: bad batch (B=%d, nsigma=%d)", B, nsigma);
  ARDAE_CHECK_ARG(fused_shape_ok(d, nsigma),
                  "dae_perturb_loss_grads: shape not eligible (ardae_dae_perturb_fused_ok): use ardae_philox_normal_at + ardae_dae_perturb + "
                  "ardae_cdae_loss_grads");
  ARDAE_CHECK_ARG(params && packed && x && xbar && sigma && eps_out && workspace && loss && grads, "dae_perturb_loss_grads: null pointer argument");
  ARDAE_CHECK_ARG((first_row & 3) == 0, "dae_perturb_loss_grads: first_row must be a multiple of 4 (one Philox counter = 4 normals)");
  const int N = B * nsigma, h = d->h_dim, z = d->input_dim;
  size_t w1, b1;
  float* h1;
  ARDAE_TRY(dae_front_slots(d, N, workspace, workspace_floats, &w1, &b1, &h1));
  const hipStream_t st = (hipStream_t)stream;
  prof_begin(st, "dae_perturb_fwd_kernel", 2.0 * (double)N * h * (z + 1), 4.0 * ((double)N * h + (double)N * (2 * z + 1) + (double)B * z));
  hipLaunchKernelGGL(dae_perturb_fwd_kernel, dim3((unsigned)ceil_div(N, DP_ROWS)), dim3(256), 0, st, x, N, nsigma, z, delta, seed, offset_sigma,
                     offset_eps, (const StepState*)state, first_row, xbar, sigma, eps_out, params + w1, params + b1, h, d->act,
                     h1);
  prof_end(st);
  ARDAE_LAUNCH_CHECK();
  return dae_loss_grads_from_h1(d, params, packed, xbar, sigma, eps_out, N, workspace, workspace_floats, loss, grads, st);
}

int ardae_dae_noise_perturb(const float* x, const float* eps, int B, int nsigma, int d, float sigma, const void* dae_state, float* xbar,
                            float* sigma_out, void* stream) {
  ARDAE_CHECK_ARG(x && eps && xbar && sigma_out, "dae_noise_perturb: null pointer argument");
  ARDAE_CHECK_ARG(B > 0 && nsigma > 0 && d > 0 && (int64_t)B * nsigma * d < (int64_t)1 << 31, "dae_noise_perturb: bad batch (B=%d, nsigma=%d, d=%d)", B,
                  nsigma, d);
  const int64_t n = (int64_t)B * nsigma * d;
  const hipStream_t st = (hipStream_t)stream;
  const DevFloat s = dae_state ? dae_state_sigma(dae_state) : DevFloat(sigma);
  prof_begin(st, "dae_noise_perturb_kernel", 2.0 * (double)n, 4.0 * (2.0 * (double)n + (double)B * nsigma + (double)B * d));
  hipLaunchKernelGGL(dae_noise_perturb_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, st, x, eps, n, nsigma, d, s.v,
                     s.p, xbar, sigma_out);
  prof_end(st);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

int ardae_latent_noise_perturb(const float* latent, const float* z0, const float* eps, int B, int nz, int nstd, int z, float std_scale, float sigma,
                               const void* dae_state, float* xbar, float* sigma_out, void* stream) {
  ARDAE_CHECK_ARG(latent && z0 && eps && xbar && sigma_out, "latent_noise_perturb: null pointer argument");
  ARDAE_CHECK_ARG(B > 0 && nz > 0 && nstd > 0 && z > 0 && (int64_t)B * nz * nstd * z < (int64_t)1 << 31,
                  "latent_noise_perturb: bad batch (B=%d, nz=%d, nstd=%d, z=%d)", B, nz, nstd, z);
  const int64_t n = (int64_t)B * nz * nstd * z;
  const hipStream_t st = (hipStream_t)stream;
  const DevFloat s = dae_state ? dae_state_sigma(dae_state) : DevFloat(sigma);
  prof_begin(st, "latent_noise_perturb_kernel", 3.0 * (double)n, 4.0 * (2.0 * (double)n + (double)B * nz * (nstd + z) + (double)B * z));
  hipLaunchKernelGGL(latent_noise_perturb_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, st, latent, z0, eps, n, nz,
                     nstd, z, std_scale, s.v, s.p, xbar, sigma_out);
  prof_end(st);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

int ardae_latent_noise_perturb_draw_ok(int nz, int nstd, int z) { return nz > 0 && nstd > 0 && z > 0 ? 1 : 0; }

int ardae_latent_noise_perturb_draw(const float* latent, const float* z0, int B, int nz, int nstd, int z, float std_scale, float sigma,
                                    const void* dae_state, uint64_t seed, uint64_t offset_eps, uint64_t first_row, float* xbar, float* sigma_out,
                                    float* eps_out, void* stream) {
  ARDAE_CHECK_ARG(latent && z0 && xbar && sigma_out && eps_out, "latent_noise_perturb_draw: null pointer argument");
  ARDAE_CHECK_ARG(B > 0 && nz > 0 && nstd > 0 && z > 0 && (int64_t)B * nz * nstd * z < (int64_t)1 << 31,
                  "latent_noise_perturb_draw: bad batch (B=%d, nz=%d, nstd=%d, z=%d)", B, nz, nstd, z);
  ARDAE_CHECK_ARG((first_row & 3) == 0, "latent_noise_perturb_draw: first_row must be a multiple of 4 (one Philox counter = 4 normals)");
  const int N = B * nz * nstd;
  const hipStream_t st = (hipStream_t)stream;
  const int vec_ok = ((reinterpret_cast<uintptr_t>(xbar) | reinterpret_cast<uintptr_t>(eps_out)) & 15) == 0 ? 1 : 0;
  prof_begin(st, "latent_noise_perturb_draw_kernel", 3.0 * (double)N * z, 4.0 * (2.0 * (double)N * z + (double)B * nz * (nstd + z) + (double)B * z));
  hipLaunchKernelGGL(latent_noise_perturb_draw_kernel, dim3((unsigned)ceil_div(N, LN_ROWS)), dim3(256), 0, st, latent, z0, N, nz, nstd, z, std_scale,
                     sigma, (const DaeState*)dae_state, seed, offset_eps, first_row, xbar, sigma_out, eps_out, vec_ok);
  prof_end(st);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
