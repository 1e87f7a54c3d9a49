// The elementwise kernels more than one model family launches (declared in host_util.h).
#include "host_util.h"

namespace ardae {
namespace {

// y = x * act'(S)  (S = saved post-activation)
__global__ void mul_dact_kernel(const float* __restrict__ x, const float* __restrict__ S, int act, float* __restrict__ y, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) y[e] = x[e] * act_d1_rt(act, S[e]);
}

// [B, HW, C] (NHWC rows) <-> [B, C*HW] (PyTorch's .view(B, -1) of NCHW)
__global__ void nhwc_nchw_kernel(const float* __restrict__ in, int HW, int C, float* __restrict__ out, int64_t total, int to_nhwc) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % C);
  const int hw = (int)((e / C) % HW);
  const int64_t b = e / ((int64_t)C * HW);
  const int64_t nchw = (b * C + c) * HW + hw;
  if (to_nhwc) out[e] = in[nchw]; else out[nchw] = in[e];
}

}  // namespace

int launch_mul_dact(const float* x, const float* S, int act, float* y, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(mul_dact_kernel, dim3(nblk(n)), dim3(256), 0, st, x, S, act, y, n);
  ARDAE_LAUNCH_CHECK();
  return 0;
}
int launch_nhwc_nchw(const float* in, int B, int HW, int C, float* out, bool to_nhwc, hipStream_t st) {
  const int64_t total = (int64_t)B * HW * C;
  hipLaunchKernelGGL(nhwc_nchw_kernel, dim3(nblk(total)), dim3(256), 0, st, in, HW, C, out, total, to_nhwc ? 1 : 0);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace ardae
