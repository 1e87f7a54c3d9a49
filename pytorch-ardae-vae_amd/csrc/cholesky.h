// Lower Cholesky factor of one n x n matrix held in LDS: the ONE factorisation, shared by the stand-alone batched kernel
// (eval_kernels.hip, fp32) and the fused IWAE proposal kernel (iwae.hip, fp64).
#pragma once
#include "common.h"

namespace ardae {

constexpr int CHOL_MAX = 64;          // largest n
constexpr int CHOL_PITCH = 65;        // row pitch of the LDS image (elements)

__device__ __forceinline__ float chol_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double chol_sqrt(double x) { return sqrt(x); }

// Right-looking, in place; thread i owns row i (i = the thread's index in the workgroup).  Every thread of the workgroup calls it (it
// holds barriers): threads i >= n only pass them.  On entry the lower triangle is loaded and a barrier has been passed; on return the
// lower triangle holds L (the strict upper triangle is left as it was) and a barrier has been passed.  A not positive definite gives
// NaN on and below the failing pivot.
template <typename T>
__device__ __forceinline__ void cholesky_lds(T (*a)[CHOL_PITCH], int n, int i) {
  for (int k = 0; k < n; ++k) {
    const T d = chol_sqrt(a[k][k]);
    __syncthreads();
    if (i == k) a[k][k] = d;
    if (i > k && i < n) a[i][k] = a[i][k] / d;
    __syncthreads();
    if (i > k && i < n)
      for (int j = k + 1; j <= i; ++j) a[i][j] -= a[i][k] * a[j][k];
    __syncthreads();
  }
}

}  // namespace ardae
