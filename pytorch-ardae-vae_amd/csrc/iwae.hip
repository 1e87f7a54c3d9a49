// The proposal of the IWAE evaluator (logprob_w_cov_gaussian_posterior, ivae/mnist.py:378-437) as one kernel per chunk of images, and the
// log-mean-exp that closes it:
//   * iwae_proposal_kernel   mean and centred covariance of an image's encoder samples (utils/stat.py:127-158), the covariance's Cholesky
//                            factor (MultivariateNormal(mu, cov), ivae/mnist.py:397-406), the k proposal samples mu + L e and their
//                            log-density (ivae/mnist.py:408-417) - one workgroup per image, z_dim <= 64
//   * iwae_reduce_kernel     log(mean_j exp(lw_j - max) + 1e-10) + max with lw = -recon - prior - logq (ivae/mnist.py:427-436)
// Both are stream-ordered, read nothing on the host and keep no state.  Mean, covariance, factor and the triangular products are
// accumulated in fp64 in an order that depends on (ke, k, z) only: an image's outputs do not depend on the batch it is launched in.
#include "ardae_hip.h"
#include "cholesky.h"
#include "common.h"
#include "philox.h"

namespace ardae {
namespace {

constexpr int IW_THREADS = 256;
constexpr int IW_TILE = 4096;          // doubles of the streaming tile (32 KiB): zs rows, then covariance partials, then the e rows (as floats)

__global__ __launch_bounds__(IW_THREADS) void iwae_proposal_kernel(const float* __restrict__ zs, const float* __restrict__ prop_noise, int ke,
                                                                   int k, int z, double jitter, uint64_t seed, uint64_t offset,
                                                                   uint64_t first_element, float* __restrict__ newz, float* __restrict__ logq,
                                                                   float* __restrict__ eps_out, float* __restrict__ mu_out,
                                                                   float* __restrict__ chol_out) {
  __shared__ double a[CHOL_MAX][CHOL_PITCH];
  __shared__ double tile[IW_TILE];
  __shared__ double mu_s[CHOL_MAX];
  __shared__ double part[IW_THREADS];
  __shared__ double logdet_s;
  const int t = threadIdx.x;
  const size_t b = blockIdx.x;
  const float* zb = zs + b * (size_t)ke * z;

  // ---- 1. column mean: G row groups x z columns, each group's rows in ascending order, then the groups in ascending order
  const int G = IW_THREADS / z;
  {
    const int g = t / z, c = t - g * z;
    double s = 0.0;
    if (g < G)
      for (int r = g; r < ke; r += G) s += (double)zb[(size_t)r * z + c];
    part[t] = s;
  }
  __syncthreads();
  if (t < z) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += part[g * z + t];
    mu_s[t] = s / (double)ke;
  }
  __syncthreads();

  // ---- 2. centred covariance: the rows stream through LDS in tiles; a thread owns one 4 x 4 block of the matrix for the rows
  //         r = rg (mod RG) of every tile; the RG partial blocks are then added in ascending order
  const int zp = (z + 3) & ~3, nb1 = zp >> 2, nb = nb1 * nb1, RG = IW_THREADS / nb;
  const int rg = t / nb, blk = t - rg * nb, ti = blk / nb1, tj = blk - ti * nb1;
  const bool active = rg < RG;
  const int TR = IW_TILE / zp;
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
  for (int r0 = 0; r0 < ke; r0 += TR) {
    const int rows = min(TR, ke - r0);
    for (int p = t; p < rows * zp; p += IW_THREADS) {
      const int r = p / zp, c = p - r * zp;
      tile[p] = c < z ? (double)zb[(size_t)(r0 + r) * z + c] - mu_s[c] : 0.0;
    }
    __syncthreads();
    if (active)
      for (int r = rg; r < rows; r += RG) {
        const double* row = tile + r * zp;
        double x[4], y[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { x[i] = row[4 * ti + i]; y[i] = row[4 * tj + i]; }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = fma(x[i], y[j], acc[i][j]);
      }
    __syncthreads();
  }
  if (active)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) tile[(rg * nb + blk) * 16 + i * 4 + j] = acc[i][j];
  __syncthreads();
  for (int e = t; e < z * z; e += IW_THREADS) {
    const int i = e / z, j = e - i * z;
    const int at = ((i >> 2) * nb1 + (j >> 2)) * 16 + (i & 3) * 4 + (j & 3);
    double s = 0.0;
    for (int g = 0; g < RG; ++g) s += tile[g * nb * 16 + at];
    s /= (double)(ke - 1);
    a[i][j] = i == j ? s + jitter : s;
  }
  __syncthreads();

  // ---- 3. factor, log-determinant; an image whose covariance is not positive definite gets NaN in newz and logq
  cholesky_lds(a, z, t);
  if (t < z) part[t] = log(a[t][t]);
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int i = 0; i < z; ++i) s += part[i];
    logdet_s = s;
  }
  __syncthreads();
  const double logdet = logdet_s;
  const double poison = isfinite(logdet) ? 0.0 : (double)NAN;
  if (mu_out && t < z) mu_out[b * z + t] = (float)mu_s[t];
  if (chol_out)
    for (int e = t; e < z * z; e += IW_THREADS) {
      const int i = e / z, j = e - i * z;
      chol_out[b * (size_t)z * z + e] = j <= i ? (float)a[i][j] : 0.f;
    }

  // ---- 4. proposal samples, JT rows of e at a time in LDS (row pitch ez, odd); a thread owns one element of newz, so a wave's
  //         global stores are contiguous
  const int ez = z | 1, JT = IW_TILE / z;
  float* et = reinterpret_cast<float*>(tile);
  const size_t ib = b * (size_t)k * z;
  const double lognorm = 0.5 * (double)z * 1.8378770664093454836;      // z/2 log(2 pi)
  for (int j0 = 0; j0 < k; j0 += JT) {
    const int rows = min(JT, k - j0), n = rows * z;
    const size_t base = ib + (size_t)j0 * z;
    __syncthreads();
    if (prop_noise) {
      for (int p = t; p < n; p += IW_THREADS) {
        const int j = p / z, i = p - j * z;
        et[j * ez + i] = prop_noise[base + p];
      }
    } else {
      // element first_element + base + p of the draw (seed, offset), keyed exactly like ardae_philox_normal_at: one counter = 4 normals
      const uint64_t g0 = first_element + base, g1 = g0 + (uint64_t)n;
      const uint64_t c0 = g0 >> 2, nc = ((g1 + 3) >> 2) - c0;
      for (uint64_t c = t; c < nc; c += IW_THREADS) {
        float v[4];
        philox_normal4(seed, offset, c0 + c, v);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const uint64_t g = (c0 + c) * 4 + u;
          if (g >= g0 && g < g1) {
            const int p = (int)(g - g0), j = p / z, i = p - j * z;
            et[j * ez + i] = v[u];
          }
        }
      }
    }
    __syncthreads();
    for (int p = t; p < n; p += IW_THREADS) {
      const int j = p / z, i = p - j * z;
      const float* er = et + j * ez;
      double s = mu_s[i];
      for (int c = 0; c <= i; ++c) s = fma(a[i][c], (double)er[c], s);
      newz[base + p] = (float)(s + poison);
      if (eps_out) eps_out[base + p] = er[i];
    }
    for (int j = t; j < rows; j += IW_THREADS) {
      const float* er = et + j * ez;
      double q = 0.0;
      for (int c = 0; c < z; ++c) q = fma((double)er[c], (double)er[c], q);
      logq[b * (size_t)k + j0 + j] = (float)(-0.5 * q - logdet - lognorm + poison);
    }
  }
}

// One workgroup per image; a thread's rows in ascending order, then a fixed tree over the threads.  NaN rows give a NaN result.
__global__ __launch_bounds__(IW_THREADS) void iwae_reduce_kernel(const float* __restrict__ recon, const float* __restrict__ prior,
                                                                 const float* __restrict__ logq, int k, float* __restrict__ out) {
  __shared__ double sh[IW_THREADS];
  const int t = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * k;
  double m = -INFINITY;
  for (int j = t; j < k; j += IW_THREADS) m = fmax(m, -(double)recon[base + j] - (double)prior[base + j] - (double)logq[base + j]);
  sh[t] = m;
  __syncthreads();
  for (int o = IW_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) sh[t] = fmax(sh[t], sh[t + o]);
    __syncthreads();
  }
  m = sh[0];
  __syncthreads();
  double s = 0.0;
  for (int j = t; j < k; j += IW_THREADS) s += exp(-(double)recon[base + j] - (double)prior[base + j] - (double)logq[base + j] - m);
  sh[t] = s;
  __syncthreads();
  for (int o = IW_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  if (t == 0) out[blockIdx.x] = (float)(log(sh[0] / (double)k + 1e-10) + m);
}

}  // namespace
}  // namespace ardae

using namespace ardae;

extern "C" {

int ardae_iwae_proposal(const float* zs, const float* prop_noise, int B, int ke, int k, int z, float jitter, uint64_t seed, uint64_t offset,
                        uint64_t first_element, float* newz, float* logq, float* eps_out, float* mu, float* chol, void* stream) {
  ARDAE_CHECK_ARG(z >= 1 && z <= CHOL_MAX, "iwae_proposal: need 1 <= z <= 64 (got z=%d)", z);
  ARDAE_CHECK_ARG(B > 0 && ke >= 2 && k >= 1, "iwae_proposal: need B > 0, ke >= 2, k >= 1 (got B=%d, ke=%d, k=%d)", B, ke, k);
  ARDAE_CHECK_ARG((int64_t)ke * z <= INT32_MAX && (int64_t)k * z <= INT32_MAX, "iwae_proposal: an image's rows exceed 2^31 elements (ke=%d, k=%d, z=%d)", ke, k, z);
  ARDAE_CHECK_ARG(jitter >= 0.f && jitter < INFINITY, "iwae_proposal: jitter must be finite and >= 0");
  ARDAE_CHECK_ARG((first_element & 3) == 0, "iwae_proposal: first_element must be a multiple of 4 (one Philox counter = 4 normals)");
  ARDAE_CHECK_ARG(zs && newz && logq, "iwae_proposal: zs, newz and logq must not be NULL");
  hipLaunchKernelGGL(iwae_proposal_kernel, dim3((unsigned)B), dim3(IW_THREADS), 0, (hipStream_t)stream, zs, prop_noise, ke, k, z, (double)jitter,
                     seed, offset, first_element, newz, logq, eps_out, mu, chol);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

int ardae_iwae_reduce(const float* recon, const float* prior, const float* logq, int B, int k, float* out, void* stream) {
  ARDAE_CHECK_ARG(B > 0 && k >= 1, "iwae_reduce: need B > 0, k >= 1 (got B=%d, k=%d)", B, k);
  ARDAE_CHECK_ARG(recon && prior && logq && out, "iwae_reduce: NULL argument");
  hipLaunchKernelGGL(iwae_reduce_kernel, dim3((unsigned)B), dim3(IW_THREADS), 0, (hipStream_t)stream, recon, prior, logq, k, out);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
