// The second phase of the two fused front ends (dae_perturb.hip: draw + perturbation + first layer of the score network;
// generator.hip: draw + first layer of the generator): h_1 = act(W1 x + b_1 [+ sigma w1s]) for a 64-row tile whose inputs sit in LDS.
#pragma once
#include "common.h"

namespace ardae {

constexpr int FRONT_ROWS = 64;   // rows per workgroup (256 threads) of a fused front end

// K = d <= DMAX, so the layer is nothing but its N x h store.  A lane owns FOUR consecutive columns (its 4 (d + 2) weights stay in
// registers) and h / 4 lanes cover a row, so every store instruction of a wave is 64 x 16 bytes = 1 KiB of consecutive addresses - one
// full row at h 256, two at h 128, four at h 64; the row's inputs are LDS broadcasts.  The dot product is a chain of FMAs in ascending k
// from 0 (the order the FP32 MFMA of the stand-alone layer adds in), then + b_1, then (SIGMA) fma(sigma, w1s, .).
//   xb [FRONT_ROWS, d], sg [FRONT_ROWS] (SIGMA only): the tile's inputs in LDS, written before the barrier that precedes the call
//   W1: [h, ldw] row-major, columns 0 .. d - 1 the inputs' (SIGMA: column d the sigma column); h is 64, 128 or 256
// Rows at or beyond N (a last partial tile) write nothing.
template <int DMAX, bool SIGMA>
__device__ __forceinline__ void front_first_layer(const float* xb, const float* sg, int d, int row0, int N, const float* __restrict__ W1, int ldw,
                                                  const float* __restrict__ b1, int h, int act, float* __restrict__ h1) {
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int lpr = h >> 2, rpw = 64 / lpr;          // lanes per row, rows per wave store
  const int lc = lane % lpr, lr = lane / lpr, c0 = 4 * lc;
  float w[4][DMAX], ws[4], bs[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float* wr = W1 + (size_t)(c0 + j) * ldw;
#pragma unroll
    for (int k = 0; k < DMAX; ++k) w[j][k] = k < d ? wr[k] : 0.f;
    ws[j] = SIGMA ? wr[d] : 0.f;
    bs[j] = b1[c0 + j];
  }
  for (int r = wave * (FRONT_ROWS / 4) + lr; r < (wave + 1) * (FRONT_ROWS / 4); r += rpw) {
    const int row = row0 + r;
    if (row >= N) break;
    const float s = SIGMA ? sg[r] : 0.f;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < DMAX; ++k)
      if (k < d) {
        const float xv = xb[r * d + k];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(xv, w[j][k], acc[j]);
      }
    f32x4 y;
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = act_fwd_rt(act, SIGMA ? __builtin_fmaf(s, ws[j], acc[j] + bs[j]) : acc[j] + bs[j]);
    *reinterpret_cast<f32x4*>(h1 + (size_t)row * h + c0) = y;
  }
}

}  // namespace ardae
