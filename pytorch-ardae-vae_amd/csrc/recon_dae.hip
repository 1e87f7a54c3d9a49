// Front end and score of the reconstruction DAEs (models/dae/mlp.py: DAE :21-82, ConditionalDAE :85-193).  They reconstruct the clean sample,
// loss = mse(main(x_bar), x), and read the score off the residual, glogprob = (main(x) - x) / std^2.  The network and the loss layer are the res
// kinds' (ardae_cdae_desc.kind 7 / 11 / 13): EPI_DAE_LOSS forms rho = sigma y + eps, and with sigma = 1, eps = -x that is y - x exactly.  So the
// kernels here write, beside x_bar, sigma_out = 1 and target_out = -x, the two buffers ardae_cdae_loss_grads reads.
//
//   philox_uniform_at_kernel   the [0, 1) map of philox_uniform_kernel, keyed like philox_normal_kernel (add_uniform_noise's torch.rand_like)
//   recon_perturb_kernel       x_bar = perturb(u) on a broadcast batch (u = x[b]) or on centred, scaled latent samples (u = std_scale (z - z0[b]))
//   recon_perturb_draw_kernel  the same with the draw made in the kernel (64-row tiles), the bits of the two launches
//   recon_score_kernel         (recon - x) / s^2
#include <algorithm>
#include <initializer_list>

#include "ardae_hip.h"
#include "common.h"
#include "elementwise.h"
#include "philox.h"
#include "profile.h"
#include "recon.h"

namespace ardae {
namespace {

// Thread q owns counter q0 + q = elements 4 (q0 + q) .. + 3 of the draw; the call's element i is element first + i of the draw, first = 4 q0 + lead,
// so a counter's four values land at out[4 q - lead ..]: the first and the last counter of a call may be partial.
__global__ __launch_bounds__(256) void philox_uniform_at_kernel(float* __restrict__ out, int64_t n, uint64_t seed, uint64_t offset,
                                                                const StepState* __restrict__ state, uint64_t q0, int lead) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i0 = q * 4 - lead;
  if (i0 >= n) return;
  if (state) offset += state->rng_offset;
  float v[4];
  philox_uniform4(seed, offset, q0 + (uint64_t)q, v);
  if (i0 >= 0 && i0 + 4 <= n && ((reinterpret_cast<uintptr_t>(out + i0) & 15) == 0)) {
    *reinterpret_cast<f32x4*>(out + i0) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
    for (int i = 0; i < 4; ++i)
      if (i0 + i >= 0 && i0 + i < n) out[i0 + i] = v[i];
  }
}

// The clean value of element (row, k): row (b, i, j) of B * nz * nstd rows reads src[b, i]; z0 non-null: centred and scaled, rounded as
// center_scale_kernel rounds it (the broadcast batch is nz = 1, z0 = NULL: row (b, j) reads x[b])
__device__ __forceinline__ float recon_clean(const float* __restrict__ src, const float* __restrict__ z0, int64_t row, int k, int nz, int nstd, int zd,
                                             float std_scale) {
  const int64_t r = row / nstd;
  const float v = src[r * zd + k];
  return z0 ? std_scale * (v - z0[(r / nz) * zd + k]) : v;
}

// Four consecutive elements e .. e + 3 of the [N, zd] rows (the first `lim` of them exist), e a multiple of 4: their clean values, x_bar from the draws v
// and the target.  quad_in: zd % 4 == 0 and src / z0 are 16-byte aligned - the four lie in one row, found with one division, and are read as one
// 16-byte access each; otherwise element by element.  The expressions are the same in both, so the bits are.
__device__ __forceinline__ void recon_quad(const float* __restrict__ src, const float* __restrict__ z0, int64_t e, int lim, int nz, int nstd, int zd,
                                           float std_scale, float s, int noise, const float v[4], int quad_in, float xb[4], float tg[4],
                                           float* __restrict__ sigma_out) {
  if (quad_in) {
    const int64_t row = e / zd, r = row / nstd;
    const int k = (int)(e - row * zd);
    const f32x4 a = *reinterpret_cast<const f32x4*>(src + r * zd + k);
    const f32x4 c = z0 ? *reinterpret_cast<const f32x4*>(z0 + (r / nz) * zd + k) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float u = z0 ? std_scale * (a[i] - c[i]) : a[i];
      xb[i] = recon_xbar(u, v[i], s, noise);
      tg[i] = -u;
    }
    if (k == 0) sigma_out[row] = 1.f;
    return;
  }
  for (int i = 0; i < lim; ++i) {
    const int64_t row = (e + i) / zd;
    const int k = (int)(e + i - row * zd);
    const float u = recon_clean(src, z0, row, k, nz, nstd, zd, std_scale);
    xb[i] = recon_xbar(u, v[i], s, noise);
    tg[i] = -u;
    if (k == 0) sigma_out[row] = 1.f;
  }
}

// vec: zd % 4 == 0 and every pointer but sigma_out is 16-byte aligned - a thread takes four consecutive elements, 16-byte loads and stores
__global__ __launch_bounds__(256) void recon_perturb_kernel(const float* __restrict__ src, const float* __restrict__ z0, const float* __restrict__ draw,
                                                            int64_t n, int nz, int nstd, int zd, float std_scale, int noise, float sv,
                                                            const float* __restrict__ sp, float* __restrict__ xbar, float* __restrict__ sigma_out,
                                                            float* __restrict__ target_out, int vec) {
  const float s = sp ? *sp : sv;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  if (vec) {        // n = N zd is a multiple of 4
    for (int64_t e = 4 * t0; e < n; e += 4 * stride) {
      const f32x4 dv = *reinterpret_cast<const f32x4*>(draw + e);
      const float v[4] = {dv[0], dv[1], dv[2], dv[3]};
      float xb[4], tg[4];
      recon_quad(src, z0, e, 4, nz, nstd, zd, std_scale, s, noise, v, 1, xb, tg, sigma_out);
      *reinterpret_cast<f32x4*>(xbar + e) = f32x4{xb[0], xb[1], xb[2], xb[3]};
      *reinterpret_cast<f32x4*>(target_out + e) = f32x4{tg[0], tg[1], tg[2], tg[3]};
    }
    return;
  }
  for (int64_t e = t0; e < n; e += stride) {
    const int64_t row = e / zd;
    const int k = (int)(e - row * zd);
    const float u = recon_clean(src, z0, row, k, nz, nstd, zd, std_scale);
    xbar[e] = recon_xbar(u, draw[e], s, noise);
    target_out[e] = -u;
    if (k == 0) sigma_out[row] = 1.f;
  }
}

// One workgroup per tile of RD_ROWS rows = 16 zd Philox counters; a thread takes counters t, t + 256, ... of its tile, four consecutive elements
// of the [N, zd] draw each, keyed exactly like ardae_philox_normal_at / ardae_philox_uniform_at (element i of the call's rows = element
// first_row zd + i of the draw (seed, offset + the block's base offset)).  Rows at or beyond N (a last partial tile) draw and write nothing.
// vec_in: recon_quad's quad_in; vec_ok: the three [N, zd] outputs are 16-byte aligned.
constexpr int RD_ROWS = 64;
__global__ __launch_bounds__(256) void recon_perturb_draw_kernel(const float* __restrict__ src, const float* __restrict__ z0, int N, int nz, int nstd,
                                                                 int zd, float std_scale, int noise, float sv, const DaeState* __restrict__ state,
                                                                 uint64_t seed, uint64_t offset, uint64_t first_row, float* __restrict__ xbar,
                                                                 float* __restrict__ sigma_out, float* __restrict__ target_out,
                                                                 float* __restrict__ draw_out, int vec_in, int vec_ok) {
  const float s = state ? state->sigma : sv;
  const uint64_t base_off = state ? state->step.rng_offset : 0;
  const int64_t row0 = (int64_t)blockIdx.x * RD_ROWS;
  const int64_t n = (int64_t)N * zd, e0 = row0 * zd;
  const uint64_t q0 = ((first_row + (uint64_t)row0) * (uint64_t)zd) >> 2;     // first_row and RD_ROWS are multiples of 4
  for (int c = threadIdx.x; c < (RD_ROWS / 4) * zd; c += 256) {
    const int64_t e = e0 + 4 * (int64_t)c;
    if (e >= n) break;
    float v[4], xb[4], tg[4];
    if (noise == RECON_GAUSSIAN) philox_normal4(seed, offset + base_off, q0 + (uint64_t)c, v);
    else philox_uniform4(seed, offset + base_off, q0 + (uint64_t)c, v);
    const int lim = n - e < 4 ? (int)(n - e) : 4;
    recon_quad(src, z0, e, lim, nz, nstd, zd, std_scale, s, noise, v, vec_in, xb, tg, sigma_out);      // (vec_in: zd % 4 == 0, so lim == 4)
    if (lim == 4 && vec_ok) {
      *reinterpret_cast<f32x4*>(xbar + e) = f32x4{xb[0], xb[1], xb[2], xb[3]};
      *reinterpret_cast<f32x4*>(target_out + e) = f32x4{tg[0], tg[1], tg[2], tg[3]};
      *reinterpret_cast<f32x4*>(draw_out + e) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
      for (int i = 0; i < lim; ++i) { xbar[e + i] = xb[i]; target_out[e + i] = tg[i]; draw_out[e + i] = v[i]; }
    }
  }
}

// glogprob's last line (dae/mlp.py:80-81): var = std^2, (recon - x) / var; out may be recon (a thread reads its elements before it writes them).
// vec: the three pointers are 16-byte aligned - four elements per thread with 16-byte accesses, then the n % 4 last ones
__global__ __launch_bounds__(256) void recon_score_kernel(const float* recon, const float* __restrict__ x, int64_t n, float sv,
                                                          const float* __restrict__ sp, float* out, int vec) {
  const float s = sp ? *sp : sv;
  const float var = s * s;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t n4 = vec ? n & ~(int64_t)3 : 0;
  for (int64_t e = 4 * t0; e < n4; e += 4 * stride) {
    const f32x4 r = *reinterpret_cast<const f32x4*>(recon + e), xv = *reinterpret_cast<const f32x4*>(x + e);
    *reinterpret_cast<f32x4*>(out + e) = f32x4{(r[0] - xv[0]) / var, (r[1] - xv[1]) / var, (r[2] - xv[2]) / var, (r[3] - xv[3]) / var};
  }
  for (int64_t e = n4 + t0; e < n; e += stride) out[e] = (recon[e] - x[e]) / var;
}

bool aligned16(std::initializer_list<const void*> ps) {
  uintptr_t bits = 0;
  for (const void* p : ps) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & 15) == 0;
}

unsigned strided_grid(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 4096); }

int perturb(const char* who, const float* src, const float* z0, const float* draw, int B, int nz, int nstd, int zd, float std_scale, int noise, float sigma,
            const void* dae_state, float* xbar, float* sigma_out, float* target_out, hipStream_t st) {
  ARDAE_CHECK_ARG(src && draw && xbar && sigma_out && target_out, "%s: null pointer argument", who);
  ARDAE_CHECK_ARG(B > 0 && nz > 0 && nstd > 0 && zd > 0 && (int64_t)B * nz * nstd * zd < (int64_t)1 << 31, "%s: bad batch (B=%d, nz=%d, nstd=%d, d=%d)", who,
                  B, nz, nstd, zd);
  ARDAE_CHECK_ARG(noise == RECON_GAUSSIAN || noise == RECON_UNIFORM, "%s: noise must be 0 (gaussian) or 1 (uniform), got %d", who, noise);
  const int64_t n = (int64_t)B * nz * nstd * zd;
  const DevFloat s = dae_state ? dae_state_sigma(dae_state) : DevFloat(sigma);
  prof_begin(st, "recon_perturb_kernel", 4.0 * (double)n, 4.0 * (3.0 * (double)n + (double)B * nz * (nstd + zd) + (double)B * zd));
  const int vec = zd % 4 == 0 && aligned16({src, z0, draw, xbar, target_out}) ? 1 : 0;      // (a null z0 is aligned)
  hipLaunchKernelGGL(recon_perturb_kernel, dim3(strided_grid(vec ? n / 4 : n)), dim3(256), 0, st, src, z0, draw, n, nz, nstd, zd, std_scale, noise, s.v,
                     s.p, xbar, sigma_out, target_out, vec);
  prof_end(st);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

int perturb_draw(const char* who, const float* src, const float* z0, int B, int nz, int nstd, int zd, float std_scale, int noise, float sigma,
                 const void* dae_state, uint64_t seed, uint64_t offset, uint64_t first_row, float* xbar, float* sigma_out, float* target_out,
                 float* draw_out, hipStream_t st) {
  ARDAE_CHECK_ARG(src && xbar && sigma_out && target_out && draw_out, "%s: null pointer argument", who);
  ARDAE_CHECK_ARG(B > 0 && nz > 0 && nstd > 0 && zd > 0 && (int64_t)B * nz * nstd * zd < (int64_t)1 << 31, "%s: bad batch (B=%d, nz=%d, nstd=%d, d=%d)", who,
                  B, nz, nstd, zd);
  ARDAE_CHECK_ARG(noise == RECON_GAUSSIAN || noise == RECON_UNIFORM, "%s: noise must be 0 (gaussian) or 1 (uniform), got %d", who, noise);
  ARDAE_CHECK_ARG((first_row & 3) == 0, "%s: first_row must be a multiple of 4 (one Philox counter = 4 values)", who);
  const int N = B * nz * nstd;
  const int vec_ok = aligned16({xbar, target_out, draw_out}) ? 1 : 0, vec_in = zd % 4 == 0 && aligned16({src, z0}) ? 1 : 0;
  prof_begin(st, "recon_perturb_draw_kernel", 4.0 * (double)N * zd, 4.0 * (3.0 * (double)N * zd + (double)B * nz * (nstd + zd) + (double)B * zd));
  hipLaunchKernelGGL(recon_perturb_draw_kernel, dim3((unsigned)ceil_div(N, RD_ROWS)), dim3(256), 0, st, src, z0, N, nz, nstd, zd, std_scale, noise, sigma,
                     (const DaeState*)dae_state, seed, offset, first_row, xbar, sigma_out, target_out, draw_out, vec_in, vec_ok);
  prof_end(st);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace ardae

using namespace ardae;

extern "C" {

int ardae_philox_uniform_at(float* out, int64_t n, uint64_t seed, uint64_t offset, const void* state, uint64_t first_element, void* stream) {
  ARDAE_CHECK_ARG(out && n > 0, "philox_uniform_at: bad arguments");
  const int lead = (int)(first_element & 3);
  const int64_t q = (n + lead + 3) / 4;
  const hipStream_t st = (hipStream_t)stream;
  prof_begin(st, "philox_uniform_at_kernel", 0.0, 4.0 * (double)n);
  hipLaunchKernelGGL(philox_uniform_at_kernel, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, st, out, n, seed, offset, (const StepState*)state,
                     first_element >> 2, lead);
  prof_end(st);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

int ardae_recon_perturb(const float* x, const float* draw, int B, int nsigma, int d, int noise, float sigma, const void* dae_state, float* xbar,
                        float* sigma_out, float* target_out, void* stream) {
  return perturb("recon_perturb", x, nullptr, draw, B, 1, nsigma, d, 1.f, noise, sigma, dae_state, xbar, sigma_out, target_out, (hipStream_t)stream);
}

int ardae_recon_perturb_draw(const float* x, int B, int nsigma, int d, int noise, float sigma, const void* dae_state, uint64_t seed, uint64_t offset,
                             uint64_t first_row, float* xbar, float* sigma_out, float* target_out, float* draw_out, void* stream) {
  return perturb_draw("recon_perturb_draw", x, nullptr, B, 1, nsigma, d, 1.f, noise, sigma, dae_state, seed, offset, first_row, xbar, sigma_out, target_out,
                      draw_out, (hipStream_t)stream);
}

int ardae_latent_recon_perturb(const float* latent, const float* z0, const float* draw, int B, int nz, int nstd, int z, float std_scale, int noise,
                               float sigma, const void* dae_state, float* xbar, float* sigma_out, float* target_out, void* stream) {
  ARDAE_CHECK_ARG(z0, "latent_recon_perturb: null pointer argument");
  return perturb("latent_recon_perturb", latent, z0, draw, B, nz, nstd, z, std_scale, noise, sigma, dae_state, xbar, sigma_out, target_out,
                 (hipStream_t)stream);
}

int ardae_latent_recon_perturb_draw(const float* latent, const float* z0, int B, int nz, int nstd, int z, float std_scale, int noise, float sigma,
                                    const void* dae_state, uint64_t seed, uint64_t offset, uint64_t first_row, float* xbar, float* sigma_out,
                                    float* target_out, float* draw_out, void* stream) {
  ARDAE_CHECK_ARG(z0, "latent_recon_perturb_draw: null pointer argument");
  return perturb_draw("latent_recon_perturb_draw", latent, z0, B, nz, nstd, z, std_scale, noise, sigma, dae_state, seed, offset, first_row, xbar, sigma_out,
                      target_out, draw_out, (hipStream_t)stream);
}

int ardae_recon_score(const float* recon, const float* x, int n, int d, float sigma, const void* dae_state, float* out, void* stream) {
  ARDAE_CHECK_ARG(recon && x && out, "recon_score: null pointer argument");
  ARDAE_CHECK_ARG(n > 0 && d > 0 && (int64_t)n * d < (int64_t)1 << 31, "recon_score: bad shape (n=%d, d=%d)", n, d);
  const int64_t ne = (int64_t)n * d;
  const hipStream_t st = (hipStream_t)stream;
  const DevFloat s = dae_state ? dae_state_sigma(dae_state) : DevFloat(sigma);
  prof_begin(st, "recon_score_kernel", 2.0 * (double)ne, 12.0 * (double)ne);
  const int vec = aligned16({recon, x, out}) ? 1 : 0;
  hipLaunchKernelGGL(recon_score_kernel, dim3(strided_grid(vec ? (ne + 3) / 4 : ne)), dim3(256), 0, st, recon, x, ne, s.v, s.p, out, vec);
  prof_end(st);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
