// Posterior diagnostics (the `''' visualize '''` block of the training loop, ivae_ardae.py:952-1111) on the device:
//   * philox_normal_scaled_kernel   one draw for all noise levels of a stacked sampler call: the numbers of ardae_philox_normal_at, each
//                                   multiplied by the scale of its slot (model.encode(x, std=s) for s = 0, 0.1, 0.5, 0.8 and the plain pass)
//   * sample_logvar_kernel          log(var(z, dim=1) + eps) of an image's nz sampler rows (ivae_ardae.py:956-957), centred two-pass in fp64
//   * hist2d_kernel                 np.histogram2d (utils/visualization.py:193-204) of two columns of a strided point set, several slots
//                                   per launch: one bins x bins table of 32-bit counters per workgroup in LDS, flushed with 64-bit global adds
//   * hist2d_wide_kernel            the same histogram for tables wider than one workgroup's LDS (the 256-bin heat maps of the final pass,
//                                   ivae_ardae.py:1224-1290, vae.py:677-720): the table is cut into bands of x-bin rows, a workgroup owns one band
// All four are stream-ordered, read nothing on the host and keep no state.  The histogram's sums are integers, so the order of the
// atomic adds does not show in the result; the other two use no atomics and a fixed order.
#include "ardae_hip.h"
#include "common.h"
#include "philox.h"

namespace ardae {
namespace {

constexpr int DG_THREADS = 256;
constexpr int HIST_MAX_BINS = 128;                         // 128 x 128 x 4 B = 64 KiB of LDS per workgroup
constexpr int HIST_WIDE_MAX_BINS = 512;                    // hist2d_wide_kernel: bands of x-bin rows, each at most ...
constexpr int HIST_BAND_CELLS = HIST_MAX_BINS * HIST_MAX_BINS;      // ... 16384 cells: the same 64 KiB of LDS, two workgroups per CU
constexpr int64_t HIST_POINTS_PER_WG = 8192;               // a workgroup's share while the grid stays below HIST_MAX_WGS
constexpr int64_t HIST_MAX_WGS = 2048;                     // per slot; beyond it the shares grow ...
constexpr int64_t HIST_MAX_SHARE = 0x7fffffff;             // ... up to what a 32-bit bin can count

// keyed exactly like philox_normal_kernel (elementwise.hip): thread q owns counter q0 + q = elements 4 (q0 + q) .. + 3 of the draw
__global__ __launch_bounds__(DG_THREADS) void philox_normal_scaled_kernel(float* __restrict__ out, int64_t n, uint64_t seed, uint64_t offset,
                                                                          const StepState* state, uint64_t q0, uint64_t width, uint64_t nslots,
                                                                          const float* __restrict__ scale) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q * 4 >= n) return;
  if (state) offset += state->rng_offset;
  float v[4];
  philox_normal4(seed, offset, q0 + (uint64_t)q, v);
  const uint64_t e0 = (q0 + (uint64_t)q) * 4;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float s = scale[((e0 + u) / width) % nslots];
    v[u] = s == 0.f ? 0.f : v[u] * s;                      // a silent slot is +0, whatever the sign of the draw
  }
  if (q * 4 + 4 <= n && ((reinterpret_cast<uintptr_t>(out) & 15) == 0)) {
    *reinterpret_cast<f32x4*>(out + q * 4) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
    for (int u = 0; u < 4 && q * 4 + u < n; ++u) out[q * 4 + u] = v[u];
  }
}

// One workgroup per image.  Columns in tiles of up to 256; inside a tile G = 256 / w row groups x w columns: a group's rows in ascending
// order, then the groups in ascending order - an order that depends on (nz, zd) only.  Mean first, then the centred squares, in fp64.
__global__ __launch_bounds__(DG_THREADS) void sample_logvar_kernel(const float* __restrict__ z, int nz, int zd, double eps,
                                                                   float* __restrict__ logvar) {
  __shared__ double part[DG_THREADS];
  __shared__ double mean_s[DG_THREADS];
  const int t = threadIdx.x;
  const float* zb = z + (size_t)blockIdx.x * nz * zd;
  for (int c0 = 0; c0 < zd; c0 += DG_THREADS) {
    const int w = min(DG_THREADS, zd - c0), G = DG_THREADS / w;
    const int g = t / w, c = c0 + (t - g * w);
    double s = 0.0;
    if (g < G)
      for (int r = g; r < nz; r += G) s += (double)zb[(size_t)r * zd + c];
    part[t] = s;
    __syncthreads();
    if (t < w) {
      double m = 0.0;
      for (int k = 0; k < G; ++k) m += part[k * w + t];
      mean_s[t] = m / (double)nz;
    }
    __syncthreads();
    s = 0.0;
    if (g < G) {
      const double m = mean_s[t - g * w];
      for (int r = g; r < nz; r += G) {
        const double d = (double)zb[(size_t)r * zd + c] - m;
        s = fma(d, d, s);
      }
    }
    part[t] = s;
    __syncthreads();
    if (t < w) {
      double q = 0.0;
      for (int k = 0; k < G; ++k) q += part[k * w + t];
      logvar[(size_t)blockIdx.x * zd + c0 + t] = (float)log(q / (double)(nz - 1) + eps);        // nz == 1: 0 / 0, NaN as torch.var gives
    }
    __syncthreads();
  }
}

// np.linspace(lo, hi, bins + 1)[k]: k * step + lo with the product and the sum rounded one by one, and hi itself at k = bins
__device__ __forceinline__ double hist_edge(int k, int bins, double lo, double hi, double step) {
#pragma clang fp contract(off)
  const double p = (double)k * step;
  return k == bins ? hi : p + lo;
}

// The bin of v among the edges above: edge[k] <= v < edge[k + 1], v == hi in the last bin, -1 for anything else (outside, inf, NaN).
// The quotient gives a candidate that can be off by one next to an edge; the two neighbouring edges decide.
__device__ __forceinline__ int hist_bin(float vf, int bins, double lo, double hi, double step) {
  const double v = (double)vf;
  if (!(v >= lo && v <= hi)) return -1;
  if (v == hi) return bins - 1;
  int k = (int)((v - lo) / step);
  k = max(0, min(bins - 1, k));
  while (k > 0 && v < hist_edge(k, bins, lo, hi, step)) --k;
  while (k < bins - 1 && v >= hist_edge(k + 1, bins, lo, hi, step)) ++k;
  return k;
}

// blockIdx.y = slot, blockIdx.x = a contiguous share of at most `share` (< 2^31) points: no 32-bit bin can overflow.  The table is
// [x bin][y bin] like numpy's H and the counts it is flushed into; LDS atomics on one dword serialise, which is what a peaked
// posterior costs - the result does not depend on it.
__global__ __launch_bounds__(DG_THREADS) void hist2d_kernel(const float* __restrict__ pts, int64_t n, int64_t row_stride, int64_t slot_stride,
                                                            int col_x, int col_y, double lo, double hi, double step, int bins, int64_t share,
                                                            unsigned long long* __restrict__ counts) {
  __shared__ unsigned int table[HIST_MAX_BINS * HIST_MAX_BINS];
  const int t = threadIdx.x, cells = bins * bins;
  for (int i = t; i < cells; i += DG_THREADS) table[i] = 0u;
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * share, i1 = min(n, i0 + share);
  const float* base = pts + (int64_t)blockIdx.y * slot_stride;
  for (int64_t i = i0 + t; i < i1; i += DG_THREADS) {
    const float* p = base + i * row_stride;
    const int bx = hist_bin(p[col_x], bins, lo, hi, step);
    const int by = hist_bin(p[col_y], bins, lo, hi, step);
    if (bx >= 0 && by >= 0) atomicAdd(&table[bx * bins + by], 1u);
  }
  __syncthreads();
  unsigned long long* out = counts + (size_t)blockIdx.y * cells;
  for (int i = t; i < cells; i += DG_THREADS) {
    const unsigned int c = table[i];
    if (c) atomicAdd(&out[i], (unsigned long long)c);
  }
}

// The table of hist2d_kernel cut into bands of `band_rows` x-bin rows (band_rows * bins <= HIST_BAND_CELLS): blockIdx.z = band, and a
// workgroup counts the points of its share whose x bin falls into its band - every point is counted by exactly one band, the y bin is
// looked up for those points only.  A dropped x (bin -1) lies in no band.  Shares, counters and the flush are hist2d_kernel's.
__global__ __launch_bounds__(DG_THREADS) void hist2d_wide_kernel(const float* __restrict__ pts, int64_t n, int64_t row_stride, int64_t slot_stride,
                                                                 int col_x, int col_y, double lo, double hi, double step, int bins, int band_rows,
                                                                 int64_t share, unsigned long long* __restrict__ counts) {
  __shared__ unsigned int table[HIST_BAND_CELLS];
  const int t = threadIdx.x;
  const int r0 = (int)blockIdx.z * band_rows, rows = min(band_rows, bins - r0), cells = rows * bins;
  for (int i = t; i < cells; i += DG_THREADS) table[i] = 0u;
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * share, i1 = min(n, i0 + share);
  const float* base = pts + (int64_t)blockIdx.y * slot_stride;
  for (int64_t i = i0 + t; i < i1; i += DG_THREADS) {
    const float* p = base + i * row_stride;
    const int r = hist_bin(p[col_x], bins, lo, hi, step) - r0;
    if (r < 0 || r >= rows) continue;
    const int by = hist_bin(p[col_y], bins, lo, hi, step);
    if (by >= 0) atomicAdd(&table[r * bins + by], 1u);
  }
  __syncthreads();
  unsigned long long* out = counts + ((size_t)blockIdx.y * bins + r0) * bins;
  for (int i = t; i < cells; i += DG_THREADS) {
    const unsigned int c = table[i];
    if (c) atomicAdd(&out[i], (unsigned long long)c);
  }
}

// the grid of both histogram kernels along the points: `wgs` shares of `share` points, no share beyond what a 32-bit bin can count
static void hist_shares(int64_t n, int64_t* wgs, int64_t* share) {
  *wgs = ceil_div64(n, HIST_POINTS_PER_WG);
  if (*wgs > HIST_MAX_WGS) *wgs = HIST_MAX_WGS;
  *share = ceil_div64(n, *wgs);
  if (*share > HIST_MAX_SHARE) {
    *share = HIST_MAX_SHARE;
    *wgs = ceil_div64(n, *share);
  }
}

}  // namespace
}  // namespace ardae

using namespace ardae;

extern "C" {

int ardae_philox_normal_scaled_at(float* out, int64_t n, uint64_t seed, uint64_t offset, const void* state, uint64_t first_element, int width,
                                  int nslots, const float* scale, void* stream) {
  ARDAE_CHECK_ARG(n > 0 && width >= 1 && nslots >= 1, "philox_normal_scaled_at: need n > 0, width >= 1, nslots >= 1 (got n=%lld, width=%d, nslots=%d)",
                  (long long)n, width, nslots);
  ARDAE_CHECK_ARG((first_element & 3) == 0, "philox_normal_scaled_at: first_element must be a multiple of 4 (one Philox counter = 4 normals)");
  ARDAE_CHECK_ARG(out && scale, "philox_normal_scaled_at: out and scale must not be NULL");
  const int64_t q = (n + 3) / 4;
  hipLaunchKernelGGL(philox_normal_scaled_kernel, dim3((unsigned)((q + DG_THREADS - 1) / DG_THREADS)), dim3(DG_THREADS), 0, (hipStream_t)stream, out,
                     n, seed, offset, (const StepState*)state, first_element >> 2, (uint64_t)width, (uint64_t)nslots, scale);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

int ardae_sample_logvar(const float* z, int B, int nz, int zd, float eps, float* logvar, void* stream) {
  ARDAE_CHECK_ARG(B > 0 && nz >= 1 && zd >= 1, "sample_logvar: need B > 0, nz >= 1, zd >= 1 (got B=%d, nz=%d, zd=%d)", B, nz, zd);
  ARDAE_CHECK_ARG((int64_t)nz * zd <= INT32_MAX, "sample_logvar: an image's rows exceed 2^31 elements (nz=%d, zd=%d)", nz, zd);
  ARDAE_CHECK_ARG(eps >= 0.f && eps < INFINITY, "sample_logvar: eps must be finite and >= 0");
  ARDAE_CHECK_ARG(z && logvar, "sample_logvar: z and logvar must not be NULL");
  hipLaunchKernelGGL(sample_logvar_kernel, dim3((unsigned)B), dim3(DG_THREADS), 0, (hipStream_t)stream, z, nz, zd, (double)eps, logvar);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

int ardae_hist2d(const float* pts, int64_t n, int64_t row_stride, int nslots, int64_t slot_stride, int col_x, int col_y, double lo, double hi,
                 int bins, int64_t* counts, void* stream) {
  ARDAE_CHECK_ARG(bins >= 1 && bins <= HIST_MAX_BINS, "hist2d: need 1 <= bins <= 128 (got bins=%d): the table is one workgroup's LDS", bins);
  ARDAE_CHECK_ARG(hi > lo && lo > -INFINITY && hi < INFINITY, "hist2d: need finite lo < hi (got lo=%g, hi=%g)", lo, hi);
  ARDAE_CHECK_ARG(n > 0 && nslots >= 1 && nslots <= 65535, "hist2d: need n > 0 and 1 <= nslots <= 65535 (got n=%lld, nslots=%d)", (long long)n, nslots);
  ARDAE_CHECK_ARG(row_stride >= 1 && slot_stride >= 0 && col_x >= 0 && col_y >= 0,
                  "hist2d: need row_stride >= 1, slot_stride >= 0, col_x >= 0, col_y >= 0 (got %lld, %lld, %d, %d)", (long long)row_stride,
                  (long long)slot_stride, col_x, col_y);
  ARDAE_CHECK_ARG(pts && counts, "hist2d: pts and counts must not be NULL");
  int64_t wgs, share;
  hist_shares(n, &wgs, &share);
  ARDAE_CHECK_ARG(wgs <= INT32_MAX, "hist2d: n=%lld points are more than one launch takes", (long long)n);
  const double step = (hi - lo) / (double)bins;                 // np.linspace: delta / div
  hipLaunchKernelGGL(hist2d_kernel, dim3((unsigned)wgs, (unsigned)nslots), dim3(DG_THREADS), 0, (hipStream_t)stream, pts, n, row_stride, slot_stride,
                     col_x, col_y, lo, hi, step, bins, share, reinterpret_cast<unsigned long long*>(counts));
  ARDAE_LAUNCH_CHECK();
  return 0;
}

int ardae_hist2d_wide(const float* pts, int64_t n, int64_t row_stride, int nslots, int64_t slot_stride, int col_x, int col_y, double lo, double hi,
                      int bins, int64_t* counts, void* stream) {
  ARDAE_CHECK_ARG(bins >= 1 && bins <= HIST_WIDE_MAX_BINS, "hist2d_wide: need 1 <= bins <= 512 (got bins=%d)", bins);
  ARDAE_CHECK_ARG(hi > lo && lo > -INFINITY && hi < INFINITY, "hist2d_wide: need finite lo < hi (got lo=%g, hi=%g)", lo, hi);
  ARDAE_CHECK_ARG(n > 0 && nslots >= 1 && nslots <= 65535, "hist2d_wide: need n > 0 and 1 <= nslots <= 65535 (got n=%lld, nslots=%d)", (long long)n,
                  nslots);
  ARDAE_CHECK_ARG(row_stride >= 1 && slot_stride >= 0 && col_x >= 0 && col_y >= 0,
                  "hist2d_wide: need row_stride >= 1, slot_stride >= 0, col_x >= 0, col_y >= 0 (got %lld, %lld, %d, %d)", (long long)row_stride,
                  (long long)slot_stride, col_x, col_y);
  ARDAE_CHECK_ARG(pts && counts, "hist2d_wide: pts and counts must not be NULL");
  int64_t wgs, share;
  hist_shares(n, &wgs, &share);
  ARDAE_CHECK_ARG(wgs <= INT32_MAX, "hist2d_wide: n=%lld points are more than one launch takes", (long long)n);
  const int band_rows = min(bins, HIST_BAND_CELLS / bins);      // 129 bins: 127 rows, 2 bands; 256: 64 rows, 4 bands; 512: 32 rows, 16 bands
  const int nbands = (bins + band_rows - 1) / band_rows;
  const double step = (hi - lo) / (double)bins;                 // np.linspace: delta / div
  hipLaunchKernelGGL(hist2d_wide_kernel, dim3((unsigned)wgs, (unsigned)nslots, (unsigned)nbands), dim3(DG_THREADS), 0, (hipStream_t)stream, pts, n,
                     row_stride, slot_stride, col_x, col_y, lo, hi, step, bins, band_rows, share, reinterpret_cast<unsigned long long*>(counts));
  ARDAE_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
