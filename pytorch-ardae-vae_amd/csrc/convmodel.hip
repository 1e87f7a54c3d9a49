// ConvIPVAE (models/ivae/conv.py:44-245 + models/vae/conv.py:79-136; `--model mnist-conv`, BASELINE config #4) on gfx950.
//
// The reference hard-wires the architecture (28x28x1 input; conv 1->16->32->32, k5 s2 p2: 28->14->7->4; fc4 (512+noise)->800,
// fc5 800->z; decoder MLP z->300->512, ConvTranspose2d 32->32 (4->7, zero-padded to 8), 32->16 (8->15), 16->1 (15->29,
// cropped to 28)), so this file does too.  Every (transposed) convolution is im2col / col2im (two small gather kernels,
// NHWC activations as [rows = b*H*W, C]) around the FP32-MFMA linear and wgrad kernels; the conv trunk runs on B rows only,
// fc4's image half enters as a per-image row bias exactly like the MLP sampler (csrc/model.hip).
#include <vector>

#include "ardae_hip.h"
#include "common.h"
#include "auxmodel.h"
#include "convmodel.h"
#include "ipmodel.h"

namespace ardae {
namespace {

// ------------------------------------------------------------------------------------------------ data-movement kernels
// cols[(b*OH+oh)*OW+ow][c*25+kh*5+kw] = x[b][2oh-2+kh][2ow-2+kw][c]  (0 outside H x W); x is NHWC [B,H,W,C]
__global__ void im2col_s2_kernel(const float* __restrict__ x, int H, int W, int C, int OH, int OW, float* __restrict__ cols, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int J = C * 25;
  const int j = (int)(e % J);
  const int64_t row = e / J;
  const int ow = (int)(row % OW), oh = (int)((row / OW) % OH);
  const int64_t b = row / ((int64_t)OW * OH);
  const int c = j / 25, kk = j - c * 25, kh = kk / 5, kw = kk - kh * 5;
  const int h = 2 * oh - 2 + kh, w = 2 * ow - 2 + kw;
  cols[e] = (h >= 0 && h < H && w >= 0 && w < W) ? x[((b * H + h) * W + w) * C + c] : 0.f;
}

// out[b][oh][ow][o] = f( bias[o] + sum_{kh,kw} cols[(b*IH+ih)*IW+iw][o*25+kh*5+kw] ),  ih = (oh+2-kh)/2 exact and in range;
// positions with oh >= VH or ow >= VW are written as 0 (the reference's ZeroPad2d after the activation).  `mulS`: multiply
// by act'(S) instead of applying an activation (backward-data of a convolution followed by the previous layer's act').
__global__ void col2im_s2_kernel(const float* __restrict__ cols, int IH, int IW, int O, int OH, int OW, int VH, int VW,
                                 const float* __restrict__ bias, int act, const float* __restrict__ mulS, float* __restrict__ out,
                                 int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int o = (int)(e % O);
  const int64_t pix = e / O;
  const int ow = (int)(pix % OW), oh = (int)((pix / OW) % OH);
  const int64_t b = pix / ((int64_t)OW * OH);
  float v = 0.f;
  if (oh < VH && ow < VW) {
    v = bias ? bias[o] : 0.f;
#pragma unroll
    for (int kh = 0; kh < 5; ++kh) {
      const int th = oh + 2 - kh;
      if (th < 0 || (th & 1)) continue;
      const int ih = th >> 1;
      if (ih >= IH) continue;
#pragma unroll
      for (int kw = 0; kw < 5; ++kw) {
        const int tw = ow + 2 - kw;
        if (tw < 0 || (tw & 1)) continue;
        const int iw = tw >> 1;
        if (iw >= IW) continue;
        v += cols[((b * IH + ih) * IW + iw) * (int64_t)(O * 25) + o * 25 + kh * 5 + kw];
      }
    }
    if (mulS) v *= act_d1_rt(act, mulS[e]);
    else v = act_fwd_rt(act, v);
  }
  out[e] = v;
}

// x[b][oh][ow][c] = 0 where oh >= VH or ow >= VW; x is NHWC [B, OH, OW, C]: the gradient at zero-padded positions, which a
// dense_bwd has multiplied by act'(0) - 0 for relu and softplus, not for the other activations
__global__ void zero_pad_kernel(float* __restrict__ x, int OH, int OW, int VH, int VW, int C, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int64_t pix = e / C;
  const int ow = (int)(pix % OW), oh = (int)((pix / OW) % OH);
  if (oh >= VH || ow >= VW) x[e] = 0.f;
}

int im2col(const float* x, int Bn, int H, int Wd, int C, int OH, int OW, float* cols, hipStream_t st) {
  const int64_t total = (int64_t)Bn * OH * OW * C * 25;
  hipLaunchKernelGGL(im2col_s2_kernel, dim3(nblk(total)), dim3(256), 0, st, x, H, Wd, C, OH, OW, cols, total);
  ARDAE_LAUNCH_CHECK();
  return 0;
}
int col2im(const float* cols, int Bn, int IH, int IW, int O, int OH, int OW, int VH, int VW, const float* bias, int act, const float* mulS,
           float* out, hipStream_t st) {
  const int64_t total = (int64_t)Bn * OH * OW * O;
  hipLaunchKernelGGL(col2im_s2_kernel, dim3(nblk(total)), dim3(256), 0, st, cols, IH, IW, O, OH, OW, VH, VW, bias, act, mulS, out, total);
  ARDAE_LAUNCH_CHECK();
  return 0;
}
}  // namespace

// ------------------------------------------------------------------------------------------------ shared with csrc/convvae.hip (convmodel.h)
void conv_trunk_carve(Bump& ws, size_t B, ConvWs& W) {
  W.x2 = ws.take(B * 784);
  for (int i = 0; i < 3; ++i) {
    W.cols[i] = ws.take(B * EH[i + 1] * EH[i + 1] * ECH[i] * 25);
    W.hcv[i] = ws.take(B * EH[i + 1] * EH[i + 1] * ECH[i + 1]);
  }
  W.inp = ws.take(B * 512);
}

void conv_decoder_carve(Bump& ws, size_t R, int zd, bool decode_only, ConvWs& W) {
  W.d1 = ws.take(R * 300); W.d2 = ws.take(R * 512); W.g0 = ws.take(R * 512);
  W.c1 = ws.take(R * 16 * 800); W.u1 = ws.take(R * 64 * 32);
  W.c2 = ws.take(R * 64 * 400); W.u2 = ws.take(R * 225 * 16);
  W.c3 = ws.take(R * 225 * 25); W.logit = ws.take(R * 784);
  W.rec_row = ws.take(R); W.pri_row = ws.take(R);
  if (decode_only) return;
  W.dlogit = ws.take(R * 784); W.dc3 = ws.take(R * 225 * 25); W.dp2 = ws.take(R * 225 * 16);
  W.dc2 = ws.take(R * 64 * 400); W.dp1 = ws.take(R * 64 * 32); W.dc1 = ws.take(R * 16 * 800);
  W.dg0 = ws.take(R * 512); W.dd2 = ws.take(R * 512); W.dd1 = ws.take(R * 300);
  W.dzq = ws.take(R * zd); W.dz = ws.take(R * zd); W.ones = ws.take(R * 784);
}

// conv trunk 1 -> 16 -> 32 -> 32 (k5 s2 p2, 28 -> 14 -> 7 -> 4) on the rescaled images x2 [B, 784]: fills cols / hcv and the
// NCHW-flattened output inp [B, 512] (shared by ConvIPVAE, the two trunks of the hierarchical conv model and the conv baseline)
int trunk_fwd(const Lin* conv, const size_t* conv_f, const float* params, const float* packed, const float* x2, float* const* cols,
              float* const* hcv, float* inp, int B, int act, hipStream_t st, bool cols0_ready) {
  const float* cur = x2;
  for (int i = 0; i < 3; ++i) {                                                 // conv_i = im2col + Linear([O, C*25]) + act
    const int OH = EH[i + 1], Kc = ECH[i] * 25;
    if (i > 0 || !cols0_ready) ARDAE_TRY(im2col(cur, B, EH[i], EH[i], ECH[i], OH, OH, cols[i], st));
    ARDAE_TRY(dense_fwd(act, B * OH * OH, ECH[i + 1], cols[i], Kc, Kc, packed + conv_f[i], params + conv[i].b, hcv[i], st));
    cur = hcv[i];
  }
  return launch_nhwc_nchw(hcv[2], B, 16, 32, inp, false, st);                      // h3.view(B,-1) of NCHW
}

// backward of the trunk from d(inp) [B, 512] (NCHW-flat): dh3 / dh2 / dh1 = d(pre-activation) of conv3 / conv2 / conv1 (NHWC rows)
int trunk_bwd(const size_t* conv_b, const float* packed, const float* dinp, float* dinp_t, float* const* hcv, float* dh3, float* dcols3,
              float* dh2, float* dcols2, float* dh1, int B, int act, hipStream_t st) {
  ARDAE_TRY(launch_nhwc_nchw(dinp, B, 16, 32, dinp_t, true, st));                // NCHW-flat -> NHWC rows
  ARDAE_TRY(launch_mul_dact(dinp_t, hcv[2], act, dh3, (int64_t)B * 512, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, B * 16, 800, dh3, 32, 32, packed + conv_b[2], nullptr, dcols3, st));   // conv3 backward-data: dcols = dpre . W3
  ARDAE_TRY(col2im(dcols3, B, 4, 4, 32, 7, 7, 7, 7, nullptr, act, hcv[1], dh2, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, B * 49, 400, dh2, 32, 32, packed + conv_b[1], nullptr, dcols2, st));
  return col2im(dcols2, B, 7, 7, 16, 14, 14, 14, 14, nullptr, act, hcv[0], dh1, st);
}

// the decoder up to u1 [R, 8, 8, 32]: decode.fc and deconv1 with its activation and zero pad
int conv_decode_head_fwd(const ConvLayout& P, const ConvPacked& K, const float* params, const float* packed, const float* z, int R, ConvWs& W,
                         hipStream_t st) {
  const int act = P.act;
  ARDAE_TRY(dense_fwd(act, R, 300, z, P.zd, P.zd, packed + K.dfc_f[0], params + P.dfc[0].b, W.d1, st));
  ARDAE_TRY(dense_fwd(act, R, 512, W.d1, 300, 300, packed + K.dfc_f[1], params + P.dfc[1].b, W.d2, st));
  ARDAE_TRY(launch_nhwc_nchw(W.d2, R, 16, 32, W.g0, true, st));                  // h1.view(R,32,4,4) -> NHWC rows
  // deconv1 32->32: 4x4 -> 7x7, activation, zero-pad to 8x8
  ARDAE_TRY(dense_fwd(ACT_NONE, R * 16, 800, W.g0, 32, 32, packed + K.dcv_f[0], nullptr, W.c1, st));
  return col2im(W.c1, R, 4, 4, 32, 8, 8, 7, 7, params + P.dcv[0].b, act, nullptr, W.u1, st);
}

// the decoder's last two stages as the four unfused launches: u1 -> c2, u2, c3 -> logit [R, 784]
int conv_decode_tail_fwd(const ConvLayout& P, const ConvPacked& K, const float* params, const float* packed, const float* u1, int R, float* c2, float* u2,
                         float* c3, float* logit, hipStream_t st) {
  const int act = P.act;
  // deconv2 32->16: 8x8 -> 15x15, activation
  ARDAE_TRY(dense_fwd(ACT_NONE, R * 64, 400, u1, 32, 32, packed + K.dcv_f[1], nullptr, c2, st));
  ARDAE_TRY(col2im(c2, R, 8, 8, 16, 15, 15, 15, 15, params + P.dcv[1].b, act, nullptr, u2, st));
  // logit deconv 16->1: 15x15 -> 29x29, cropped to 28x28
  ARDAE_TRY(dense_fwd(ACT_NONE, R * 225, 25, u2, 16, 16, packed + K.dcv_f[2], nullptr, c3, st));
  return col2im(c3, R, 15, 15, 1, 28, 28, 28, 28, params + P.dcv[2].b, ACT_NONE, nullptr, logit, st);
}

int conv_decode_fwd(const ConvLayout& P, const ConvPacked& K, const float* params, const float* packed, const float* z, int R, ConvWs& W,
                    hipStream_t st) {
  ARDAE_TRY(conv_decode_head_fwd(P, K, params, packed, z, R, W, st));
  return conv_decode_tail_fwd(P, K, params, packed, W.u1, R, W.c2, W.u2, W.c3, W.logit, st);
}

// decoder backward from W.dlogit (and W.dzq = prior + seed part of dL/dz): fills dc3/dp2/dc2/dp1/dc1/dg0/dd2/dd1 and W.dz
int conv_decoder_bwd(const ConvLayout& P, const ConvPacked& K, const float* packed, ConvWs& W, int R, hipStream_t st) {
  const int act = P.act;
  ARDAE_TRY(launch_fill(W.ones, (int64_t)R * 784, 1.0f, st));
  // ---- decoder backward.  d(cols) of a transposed conv = im2col of the output gradient over the deconv's INPUT grid.
  ARDAE_TRY(im2col(W.dlogit, R, 28, 28, 1, 15, 15, W.dc3, st));                 // cropped row/col 28 has no gradient
  ARDAE_TRY(dense_bwd(act, R * 225, 16, W.dc3, 25, packed + K.dcv_b[2], W.u2, W.dp2, st));   // dpre2 = (dc3 . W3^T) (.) act'(u2)
  ARDAE_TRY(im2col(W.dp2, R, 15, 15, 16, 8, 8, W.dc2, st));
  ARDAE_TRY(dense_bwd(act, R * 64, 32, W.dc2, 400, packed + K.dcv_b[1], W.u1, W.dp1, st));   // zero at the padded positions where act'(0) = 0
  if (act != ACT_RELU && act != ACT_SOFTPLUS) {      // ZeroPad2d passes no gradient: elu, tanh, leaky_relu and swish have act'(0) != 0
    const int64_t total = (int64_t)R * 64 * 32;
    hipLaunchKernelGGL(zero_pad_kernel, dim3(nblk(total)), dim3(256), 0, st, W.dp1, 8, 8, 7, 7, 32, total);
    ARDAE_LAUNCH_CHECK();
  }
  ARDAE_TRY(im2col(W.dp1, R, 8, 8, 32, 4, 4, W.dc1, st));
  ARDAE_TRY(dense_bwd(act, R * 16, 32, W.dc1, 800, packed + K.dcv_b[0], W.g0, W.dg0, st));   // g0 is the (permuted) activated output of decode.fc
  ARDAE_TRY(launch_nhwc_nchw(W.dg0, R, 16, 32, W.dd2, false, st));               // -> d(pre) of decode.fc.fc  [R,512]
  ARDAE_TRY(dense_bwd(act, R, 300, W.dd2, 512, packed + K.dfc_b[1], W.d1, W.dd1, st));
  return dense_bwd(ACT_NONE, R, P.zd, W.dd1, 300, packed + K.dfc_b[0], W.dzq, W.dz, st, W.dzq);   // + prior + injected seed
}

// the decoder's eight weight-gradient problems
void conv_decoder_wgrads(const ConvLayout& P, const ConvWs& W, int R, WgradList& wl) {
  // ConvTranspose2d: dW[in][out*25] = sum_rows input[row][in] * dcols[row][out*25]; its bias = sum of the output gradient
  wl.push(R * 225, 16, 25, W.u2, W.dc3, 25, wl.g(P.dcv[2].w), 25, nullptr);
  wl.push(R * 784, 1, 1, W.dlogit, W.ones, 1, wl.g(P.dcv[2].b), 1, nullptr);
  wl.push(R * 64, 32, 400, W.u1, W.dc2, 400, wl.g(P.dcv[1].w), 400, nullptr);
  wl.push(R * 225, 16, 1, W.dp2, W.ones, 1, wl.g(P.dcv[1].b), 1, nullptr);
  wl.push(R * 16, 32, 800, W.g0, W.dc1, 800, wl.g(P.dcv[0].w), 800, nullptr);
  wl.push(R * 64, 32, 1, W.dp1, W.ones, 1, wl.g(P.dcv[0].b), 1, nullptr);
  wl.push(R, 512, 300, W.dd2, W.d1, 300, wl.g(P.dfc[1].w), 300, wl.g(P.dfc[1].b));
  wl.push(R, 300, P.zd, W.dd1, W.z, P.zd, wl.g(P.dfc[0].w), P.zd, wl.g(P.dfc[0].b));
}

void conv_trunk_wgrads(const Lin* conv, float* const* cols, const float* dh3, const float* dh2, const float* dh1, int B, WgradList& wl) {
  wl.push(B * 16, 32, 800, dh3, cols[2], 800, wl.g(conv[2].w), 800, wl.g(conv[2].b));
  wl.push(B * 49, 32, 400, dh2, cols[1], 400, wl.g(conv[1].w), 400, wl.g(conv[1].b));
  wl.push(B * 196, 16, 25, dh1, cols[0], 25, wl.g(conv[0].w), 25, wl.g(conv[0].b));
}

// ------------------------------------------------------------------------------------------------ the decoder's last two stages as one launch
// conv_tail_kernel (kind 17's decode-only path; ardae_conv_tail variant 1): u1 [R, 8, 8, 32] NHWC - deconv1's activated output with its zero pad ->
//   stage A  u2[oh][ow][o] = act(b2[o] + sum_{kh, kw: (oh+2-kh) even, ih = (oh+2-kh)/2 in [0, 8), same for w} sum_c u1[ih][iw][c] W2[c][o][kh][kw])   15 x 15 x 16
//   stage B  logit[oh][ow] = b3 + the same sum over u2 and W3[c][0][kh][kw], 29 x 29 cropped to 28 x 28
// ONE workgroup of 256 threads per image; u1 and u2 live in LDS, channel-major with a zero halo of one position (c2, u2, c3 never reach global
// memory: 32 x 101 + 16 x 290 floats = 31.5 KiB, five workgroups per CU).  A stride-2 transposed convolution sends tap (kh, kw) to the outputs of
// parity (kh & 1, kw & 1) only, so a thread owns the 2 x 2 output quad (2a + ph, 2b + pw) of input position (a, b): tap kh reads input row
// a + 1 - (kh >> 1) for every thread alike, the 25 taps of a quad are the 25 weights W[c][o][.][.] - the same address in every lane, so they arrive
// by scalar loads and cost no LDS or vector-memory traffic - and out-of-range rows are the halo's zeros.  Stage A: lane = (a, b) of the 8 x 8 grid,
// wave w owns output channels 4w .. 4w + 3 (16 accumulators); stage B: thread = (a, b) of the 15 x 15 grid (4 accumulators).
// The weights come from the packed buffer, re-laid at pack time on 16-byte boundaries (conv_tail_pack_kernel): wt2[c][tap][o] (a wave's four
// channels of a tap are one 16-byte scalar load) and wt3[c][32] (25 taps, padded).
// Summation order of every output, in FP32 FMAs from 0: c ascending, within c the taps (kh, kw) ascending (taps that fall outside are exact zeros);
// then + bias, then the activation.  A row's bits depend on that row alone.
constexpr int CT_THREADS = 256, CT_S1 = 101, CT_S2 = 290;      // strides of a channel's 10 x 10 / 17 x 17 halo grid (odd multiples keep lanes on distinct banks)
// wt2[c][tap][o] = W2[c][o][tap] (12 800 floats), wt3[c][32] = W3[c][0][tap], zero beyond tap 24 (512 floats)
__global__ void conv_tail_pack_kernel(const float* __restrict__ w2, const float* __restrict__ w3, float* __restrict__ wt2, float* __restrict__ wt3) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < 12800) {
    const int o = e & 15, tap = (e >> 4) % 25, c = e / 400;
    wt2[e] = w2[(c * 16 + o) * 25 + tap];
  } else if (e < 12800 + 512) {
    const int i = e - 12800, tap = i & 31, c = i >> 5;
    wt3[i] = tap < 25 ? w3[c * 25 + tap] : 0.f;
  }
}

__global__ __launch_bounds__(CT_THREADS) void conv_tail_kernel(const float* __restrict__ u1, const float* __restrict__ wt2, const float* __restrict__ b2,
                                                               const float* __restrict__ wt3, const float* __restrict__ b3, int act,
                                                               float* __restrict__ logit) {
  __shared__ float s1[32 * CT_S1];
  __shared__ float s2[16 * CT_S2];
  const int t = threadIdx.x;
  const size_t r = blockIdx.x;
  for (int i = t; i < 32 * CT_S1; i += CT_THREADS) s1[i] = 0.f;
  for (int i = t; i < 16 * CT_S2; i += CT_THREADS) s2[i] = 0.f;
  __syncthreads();
  const float* src = u1 + r * 2048;
#pragma unroll
  for (int i = 0; i < 8; ++i) {      // coalesced NHWC reads; element e = (position, channel)
    const int e = t + i * CT_THREADS, pos = e >> 5, c = e & 31;
    s1[c * CT_S1 + ((pos >> 3) + 1) * 10 + (pos & 7) + 1] = src[e];
  }
  __syncthreads();
  {      // ---- stage A
    const int lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6), o0 = wv * 4, a = lane >> 3, b = lane & 7;      // wv: the same in every lane
    const float4* wq = reinterpret_cast<const float4*>(wt2) + wv;
    float acc[4][2][2] = {};
    for (int c = 0; c < 32; ++c) {
      float v[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) v[i][j] = s1[c * CT_S1 + (a + i) * 10 + b + j];      // input rows a - 1 .. a + 1
#pragma unroll
      for (int kh = 0; kh < 5; ++kh)
#pragma unroll
        for (int kw = 0; kw < 5; ++kw) {
          const float4 w = wq[(c * 25 + kh * 5 + kw) * 4];
          const float x = v[2 - (kh >> 1)][2 - (kw >> 1)];
          acc[0][kh & 1][kw & 1] = __builtin_fmaf(x, w.x, acc[0][kh & 1][kw & 1]);
          acc[1][kh & 1][kw & 1] = __builtin_fmaf(x, w.y, acc[1][kh & 1][kw & 1]);
          acc[2][kh & 1][kw & 1] = __builtin_fmaf(x, w.z, acc[2][kh & 1][kw & 1]);
          acc[3][kh & 1][kw & 1] = __builtin_fmaf(x, w.w, acc[3][kh & 1][kw & 1]);
        }
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const float bias = b2[o0 + o];
#pragma unroll
      for (int ph = 0; ph < 2; ++ph)
#pragma unroll
        for (int pw = 0; pw < 2; ++pw) {
          const int oh = 2 * a + ph, ow = 2 * b + pw;
          if (oh < 15 && ow < 15) s2[(o0 + o) * CT_S2 + (oh + 1) * 17 + ow + 1] = act_fwd_rt(act, acc[o][ph][pw] + bias);
        }
    }
  }
  __syncthreads();
  if (t < 225) {      // ---- stage B
    const int a = t / 15, b = t - a * 15;
    float acc[2][2] = {};
    for (int c = 0; c < 16; ++c) {
      float v[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) v[i][j] = s2[c * CT_S2 + (a + i) * 17 + b + j];
      const float* w = wt3 + c * 32;
#pragma unroll
      for (int kh = 0; kh < 5; ++kh)
#pragma unroll
        for (int kw = 0; kw < 5; ++kw) acc[kh & 1][kw & 1] = __builtin_fmaf(v[2 - (kh >> 1)][2 - (kw >> 1)], w[kh * 5 + kw], acc[kh & 1][kw & 1]);
    }
    const float bias = b3[0];
    float* dst = logit + r * 784;
#pragma unroll
    for (int ph = 0; ph < 2; ++ph)
#pragma unroll
      for (int pw = 0; pw < 2; ++pw) {
        const int oh = 2 * a + ph, ow = 2 * b + pw;
        if (oh < 28 && ow < 28) dst[oh * 28 + ow] = acc[ph][pw] + bias;
      }
  }
}

int launch_conv_tail(const float* u1, const float* wt2, const float* b2, const float* wt3, const float* b3, int R, int act, float* logit, hipStream_t st) {
  hipLaunchKernelGGL(conv_tail_kernel, dim3((unsigned)R), dim3(CT_THREADS), 0, st, u1, wt2, b2, wt3, b3, act, logit);
  ARDAE_LAUNCH_CHECK();
  return 0;
}
int launch_conv_tail_pack(const float* w2, const float* w3, float* wt2, float* wt3, hipStream_t st) {
  hipLaunchKernelGGL(conv_tail_pack_kernel, dim3(nblk(CT_W2 + CT_W3)), dim3(256), 0, st, w2, w3, wt2, wt3);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------ ConvIPVAE (kind == 2)
// (Entry finds carve() by argument-dependent lookup, and ConvLayout lives in namespace ardae: this overload does too, file-local)
static void carve(const ConvLayout& P, const ConvPacked&, Bump& ws, int B, int nz, int mode, ConvWs& W) {
  const size_t R = (size_t)B * nz;
  conv_trunk_carve(ws, (size_t)B, W);
  W.rb = ws.take((size_t)B * 800);
  W.t1 = ws.take(R * 800); W.z = ws.take(R * P.zd);
  if (mode == 0) return;
  conv_decoder_carve(ws, R, P.zd, mode == 2, W);
  if (mode == 2) return;
  W.dt1 = ws.take(R * 800);
  W.drb = ws.take((size_t)B * 800); W.dinp = ws.take((size_t)B * 512); W.dinp_t = ws.take((size_t)B * 512);
  W.dh3 = ws.take((size_t)B * 512); W.dcols3 = ws.take((size_t)B * 16 * 800); W.dh2 = ws.take((size_t)B * 49 * 32);
  W.dcols2 = ws.take((size_t)B * 49 * 400); W.dh1 = ws.take((size_t)B * 196 * 16);
}

namespace {

using ConvEntry = Entry<ConvLayout, ConvPacked, ConvWs>;

// the descriptor rules of kinds 2 / 4
int conv_desc_check(const ardae_model_desc* d) {
  ARDAE_TRY(desc_flags_ok(d, 0));
  ARDAE_CHECK_ARG(d->input_dim == 784 && d->noise_dim >= 1 && d->z_dim >= 1, "model: ConvIPVAE is hard-wired to 28x28x1 inputs (input_dim 784)");
  ARDAE_CHECK_ARG(d->act > ACT_NONE && d->act <= ACT_LAST, "model: unknown activation %d (relu, softplus, elu, tanh, leaky_relu, swish)", d->act);
  return 0;
}

// What the shared algorithm (csrc/ipmodel.h) needs to know of ConvIPVAE.
struct ConvTraits : IpTraitsBase {
  using Layout = ConvLayout; using Packed = ConvPacked; using Ws = ConvWs; using Entry = ConvEntry;
  static int desc_check(const ardae_model_desc* d) { return conv_desc_check(d); }
  static unsigned caps(const ardae_model_desc&) { return 0; }
  static IpBufs bufs(const ConvWs& W) { return {W.z, W.logit, nullptr, W.dlogit, nullptr, W.dzq, W.dz, W.rec_row, W.pri_row}; }
  // every weight-gradient problem of the backward, with its scratch taken from ws
  static void wgrads(const ConvLayout& P, const ConvPacked&, const ConvWs& W, const float*, const float* noise, int B, int nz, WgradList& wl, Bump& ws) {
    const int R = B * nz;
    conv_decoder_wgrads(P, W, R, wl);
    wl.push(R, P.zd, 800, W.dz, W.t1, 800, wl.g(P.fc5.w), 800, wl.g(P.fc5.b));
    wl.push(R, 800, P.nd, W.dt1, noise, P.nd, wl.g(P.fc4.w + 512), 512 + P.nd, wl.g(P.fc4.b));   // fc4 noise half (+ bias)
    wl.push(B, 800, 512, W.drb, W.inp, 512, wl.g(P.fc4.w), 512 + P.nd, nullptr);                  // fc4 image half
    conv_trunk_wgrads(P.conv, W.cols, W.dh3, W.dh2, W.dh1, B, wl);
    wl.assign(ws, CONV_WGRAD_HINT);
  }
  static size_t extra_floats(const ConvLayout& P, int B, int nz, int) { return al64((size_t)B * nz * P.nd); }    // a zero-noise buffer for encode(std=0)
  static size_t noise_floats(const ConvLayout& P, int B, int nz) { return (size_t)B * nz * P.nd; }
  static float* zero_noise(Entry& e, size_t n) { return e.ws.take(n); }
  static int sampler_fwd(Entry& e, const float* params, const float* packed, const float* x, const float* noise, int B, int nz, const IpEncodeOut*,
                         hipStream_t st) {
    auto& [P, K, ws, W] = e;
    const int R = B * nz, act = P.act;
    ARDAE_TRY(launch_affine(x, (int64_t)B * 784, 2.f, -1.f, W.x2, st));           // ivae/conv.py:81
    ARDAE_TRY(trunk_fwd(P.conv, K.conv_f, params, packed, W.x2, W.cols, W.hcv, W.inp, B, act, st));
    // fc4 on cat[h3 | noise]: the image half once per image
    ARDAE_TRY(cat_fwd(act, B, nz, 800, W.inp, 512, packed + K.fc4i_f, params + P.fc4.b, noise, P.nd, packed + K.fc4n_f, W.rb, W.t1, st));
    return dense_fwd(ACT_NONE, R, P.zd, W.t1, 800, 800, packed + K.fc5_f, params + P.fc5.b, W.z, st);
  }
  static int decoder_fwd(Entry& e, const float* params, const float* packed, const float* z, int R, hipStream_t st) {
    return conv_decode_fwd(e.P, e.K, params, packed, z, R, e.W, st);
  }
  static int decoder_bwd(Entry& e, const float* packed, int R, Grads&, hipStream_t st) { return conv_decoder_bwd(e.P, e.K, packed, e.W, R, st); }
  static int sampler_bwd(Entry& e, const float*, const float* packed, const float*, const float* noise, int B, int nz, Grads& g, hipStream_t st) {
    auto& [P, K, ws, W] = e;
    const int R = B * nz, act = P.act;
    ARDAE_TRY(dense_bwd(act, R, 800, W.dz, P.zd, packed + K.fc5_b, W.t1, W.dt1, st));
    ARDAE_TRY(launch_segment_sum(W.dt1, 800, B, nz, 800, 1.0f, W.drb, 800, st));
    ARDAE_TRY(dense_fwd(ACT_NONE, B, 512, W.drb, 800, 800, packed + K.fc4i_b, nullptr, W.dinp, st));
    ARDAE_TRY(trunk_bwd(K.conv_b, packed, W.dinp, W.dinp_t, W.hcv, W.dh3, W.dcols3, W.dh2, W.dcols2, W.dh1, B, act, st));
    // ---- weight gradients: one batched launch
    WgradList wl(g.grads, g.beta);
    wgrads(P, K, W, nullptr, noise, B, nz, wl, ws);
    ARDAE_CHECK_ARG(ws.ok, "model_vae_backward: internal workspace accounting error");
    return wl.launch(st);
  }
};

// =====================================================================================================================
// MNISTConvAuxIPVAE (`--model auxconv`, kind == 4): models/ivae/auxconv.py:48-126 - the hierarchical sampler of csrc/auxmodel.hip with
// conv trunks in place of the MLPs (models/vae/auxconv.py:32-140) and ConvIPVAE's decoder (models/vae/conv.py:79-136):
//   per image:   h3a = trunk_a(2x-1); h4a = act(Fa h3a + fa); mu0 = M0 h4a + m0; lv0 = L0 h4a + l0;  h3 = trunk_e(2x-1); rb = Fi h3 + f
//   per sample:  z0 = mu0[b] + exp(lv0[b]/2) eps0;  h4 = act(Fn z0 + rb[b]);  mu = M h4 + m; lv = L h4 + l;  z = mu + exp(lv/2) eps
// Noise layout as for kind 3: one [R, noise_dim + z_dim] tensor per sampler call.  hidden1a context = cat(h4a, h4) [B, 1600].
// =====================================================================================================================
struct AuxConvLayout {
  int nd, zd, act;
  Lin aconv[3], afc, mean0, logvar0, econv[3], efc, mean, logvar;
  ConvLayout dec;      // dfc / dcv only
  size_t total;
  explicit AuxConvLayout(const ardae_model_desc& d) : nd(d.noise_dim), zd(d.z_dim), act(d.act) {
    size_t off = 0;
    auto add = [&](Lin& l, int out, int in, int nbias) { l = next_lin(off, out, in, nbias); };
    add(aconv[0], 16, 25, 16); add(aconv[1], 32, 400, 32); add(aconv[2], 32, 800, 32);
    add(afc, 800, 512, 800); add(mean0, nd, 800, nd); add(logvar0, nd, 800, nd);
    add(econv[0], 16, 25, 16); add(econv[1], 32, 400, 32); add(econv[2], 32, 800, 32);
    add(efc, 800, 512 + nd, 800); add(mean, zd, 800, zd); add(logvar, zd, 800, zd);
    dec.nd = nd; dec.zd = zd; dec.act = act;
    dec.decoder(off);
    total = off;
  }
};

struct AuxConvPacked {
  size_t aconv_f[3], aconv_b[3], afc_f, afc_b, mean0_f, mean0_b, logvar0_f, logvar0_b, econv_f[3], econv_b[3], efci_f, efci_b, efcn_f, efcn_b,
      mean_f, mean_b, logvar_f, logvar_b;
  ConvPacked dec;
  AuxConvPacked(const AuxConvLayout& P, PackList& pl) {
    for (int i = 0; i < 3; ++i) pl.pair(P.aconv[i], aconv_f[i], aconv_b[i]);
    pl.pair(P.afc, afc_f, afc_b); pl.pair(P.mean0, mean0_f, mean0_b); pl.pair(P.logvar0, logvar0_f, logvar0_b);
    for (int i = 0; i < 3; ++i) pl.pair(P.econv[i], econv_f[i], econv_b[i]);
    pl.pair(P.efc, efci_f, efci_b, 0, 512);                            // [800, 512 + nd]: image half | z0 half
    pl.pair(P.efc, efcn_f, efcn_b, 512, P.nd);
    pl.pair(P.mean, mean_f, mean_b); pl.pair(P.logvar, logvar_f, logvar_b);
    dec.decoder_panels(P.dec, pl);
  }
  explicit AuxConvPacked(const AuxConvLayout& P, PackList&& sizing = PackList()) : AuxConvPacked(P, sizing) {}   // offsets only
};

struct AuxConvWs {
  ConvWs D;    // x2, decoder buffers, z, t1 (= h4), dzq / dz, ones, rec_row / pri_row and the decoder's backward buffers
  float *acols[3], *ahcv[3], *ainp, *h4a, *mu0, *lv0, *z0, *ecols[3], *ehcv[3], *einp, *rb, *mu, *lv, *zero;
  // backward
  float *dlv, *dt1, *dz0, *dlv0r, *drb, *dmu0, *dlv0, *dh4a, *dinp_a, *dinp_e, *dinp_t;
  float *dh3[2], *dcols3[2], *dh2[2], *dcols2[2], *dh1[2];    // [0] = aux trunk, [1] = encoder trunk
};

void carve(const AuxConvLayout& P, const AuxConvPacked&, Bump& ws, int B, int nz, int mode, AuxConvWs& W) {
  const size_t R = (size_t)B * nz;
  ConvWs& D = W.D;
  D.x2 = ws.take((size_t)B * 784);
  for (int i = 0; i < 3; ++i) {
    W.acols[i] = ws.take((size_t)B * EH[i + 1] * EH[i + 1] * ECH[i] * 25); W.ahcv[i] = ws.take((size_t)B * EH[i + 1] * EH[i + 1] * ECH[i + 1]);
    W.ecols[i] = ws.take((size_t)B * EH[i + 1] * EH[i + 1] * ECH[i] * 25); W.ehcv[i] = ws.take((size_t)B * EH[i + 1] * EH[i + 1] * ECH[i + 1]);
  }
  W.ainp = ws.take((size_t)B * 512); W.h4a = ws.take((size_t)B * 800); W.mu0 = ws.take((size_t)B * P.nd); W.lv0 = ws.take((size_t)B * P.nd);
  W.einp = ws.take((size_t)B * 512); W.rb = ws.take((size_t)B * 800);
  W.z0 = ws.take(R * P.nd); D.t1 = ws.take(R * 800); W.mu = ws.take(R * P.zd); W.lv = ws.take(R * P.zd); D.z = ws.take(R * P.zd);
  W.zero = ws.take(R * (P.nd + P.zd));
  if (mode == 0) return;
  conv_decoder_carve(ws, R, P.zd, mode == 2, D);
  if (mode == 2) return;
  W.dlv = ws.take(R * P.zd); W.dt1 = ws.take(R * 800); W.dz0 = ws.take(R * P.nd); W.dlv0r = ws.take(R * P.nd);
  W.drb = ws.take((size_t)B * 800); W.dmu0 = ws.take((size_t)B * P.nd); W.dlv0 = ws.take((size_t)B * P.nd); W.dh4a = ws.take((size_t)B * 800);
  W.dinp_a = ws.take((size_t)B * 512); W.dinp_e = ws.take((size_t)B * 512); W.dinp_t = ws.take((size_t)B * 512);
  for (int k = 0; k < 2; ++k) {
    W.dh3[k] = ws.take((size_t)B * 512); W.dcols3[k] = ws.take((size_t)B * 16 * 800); W.dh2[k] = ws.take((size_t)B * 49 * 32);
    W.dcols2[k] = ws.take((size_t)B * 49 * 400); W.dh1[k] = ws.take((size_t)B * 196 * 16);
  }
}
using AuxConvEntry = Entry<AuxConvLayout, AuxConvPacked, AuxConvWs>;

// wgrad_splits hint of the hierarchical conv backward, and the size of its first batch: the 21 problems go out as 10 + 11
constexpr int AUX_WGRAD_HINT = 10;

// keep_hidden = false (forward-only encodes of the cDAE phase): the [R, 800] hidden rows need not exist
int aux_sampler_fwd(const AuxConvLayout& P, const AuxConvPacked& K, const float* params, const float* packed, const float* x, const float* noise,
                    int B, int nz, AuxConvWs& W, bool keep_hidden, hipStream_t st) {
  const int R = B * nz, act = P.act, ldn = P.nd + P.zd;
  ARDAE_TRY(launch_affine(x, (int64_t)B * 784, 2.f, -1.f, W.D.x2, st));
  ARDAE_TRY(trunk_fwd(P.aconv, K.aconv_f, params, packed, W.D.x2, W.acols, W.ahcv, W.ainp, B, act, st));
  ARDAE_TRY(dense_fwd(act, B, 800, W.ainp, 512, 512, packed + K.afc_f, params + P.afc.b, W.h4a, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, B, P.nd, W.h4a, 800, 800, packed + K.mean0_f, params + P.mean0.b, W.mu0, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, B, P.nd, W.h4a, 800, 800, packed + K.logvar0_f, params + P.logvar0.b, W.lv0, st));
  ARDAE_TRY(launch_reparam_fwd(W.mu0, W.lv0, noise, ldn, R, P.nd, nz, W.z0, st));
  ARDAE_TRY(trunk_fwd(P.econv, K.econv_f, params, packed, W.D.x2, W.ecols, W.ehcv, W.einp, B, act, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, B, 800, W.einp, 512, 512, packed + K.efci_f, params + P.efc.b, W.rb, st));   // image half of the encoder's fc, once per image
  if (!keep_hidden) {    // z0 -> 800 -> (mean | logvar) in one launch, hidden rows on chip (linear_shortk.hip::sampler_tail_kernel)
    LinArgs A{}; A.M = R; A.Nout = 800; A.act = act; A.nsrc = 1; A.rowbias = W.rb; A.rowbias_ld = 800; A.rows_per_group = nz;
    A.src[0].x = W.z0; A.src[0].ld = P.nd; A.src[0].K = P.nd; A.src[0].wp = packed + K.efcn_f;
    if (sampler_tail_eligible(A, P.zd)) {
      ARDAE_TRY(launch_sampler_tail(A, packed + K.mean_f, params + P.mean.b, W.mu, P.zd, P.zd, st, packed + K.logvar_f, params + P.logvar.b, W.lv, P.zd));
      return launch_reparam_fwd(W.mu, W.lv, noise + P.nd, ldn, R, P.zd, 1, W.D.z, st);
    }
  }
  { LinArgs A{}; A.rowbias = W.rb; A.rowbias_ld = 800; A.rows_per_group = nz; A.Y = W.D.t1; A.ldY = 800;
    ARDAE_TRY(lin1(EPI_ACT, act, R, 800, W.z0, P.nd, P.nd, packed + K.efcn_f, A, st)); }
  ARDAE_TRY(dense_fwd(ACT_NONE, R, P.zd, W.D.t1, 800, 800, packed + K.mean_f, params + P.mean.b, W.mu, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, R, P.zd, W.D.t1, 800, 800, packed + K.logvar_f, params + P.logvar.b, W.lv, st));
  return launch_reparam_fwd(W.mu, W.lv, noise + P.nd, ldn, R, P.zd, 1, W.D.z, st);
}

// What the shared algorithm (csrc/ipmodel.h) needs to know of MNISTConvAuxIPVAE.
struct AuxConvTraits : IpTraitsBase {
  using Layout = AuxConvLayout; using Packed = AuxConvPacked; using Ws = AuxConvWs; using Entry = AuxConvEntry;
  static int desc_check(const ardae_model_desc* d) { return conv_desc_check(d); }
  static unsigned caps(const ardae_model_desc&) { return CAP_HIDDEN; }
  static IpBufs bufs(const AuxConvWs& W) {
    const ConvWs& D = W.D;
    return {D.z, D.logit, nullptr, D.dlogit, nullptr, D.dzq, D.dz, D.rec_row, D.pri_row};
  }
  // every weight-gradient problem of the backward, with its scratch taken from ws
  static void wgrads(const AuxConvLayout& P, const AuxConvPacked&, const AuxConvWs& W, const float*, const float*, int B, int nz, WgradList& wl, Bump& ws) {
    const int R = B * nz;
    const ConvWs& D = W.D;
    conv_decoder_wgrads(P.dec, D, R, wl);                                                             // decoder (as ConvIPVAE)
    wl.push(R, P.zd, 800, D.dz, D.t1, 800, wl.g(P.mean.w), 800, wl.g(P.mean.b));
    wl.push(R, P.zd, 800, W.dlv, D.t1, 800, wl.g(P.logvar.w), 800, wl.g(P.logvar.b));
    wl.push(R, 800, P.nd, W.dt1, W.z0, P.nd, wl.g(P.efc.w + 512), 512 + P.nd, wl.g(P.efc.b));         // fc z0 half (+ bias)
    wl.push(B, 800, 512, W.drb, W.einp, 512, wl.g(P.efc.w), 512 + P.nd, nullptr);                     // fc image half
    conv_trunk_wgrads(P.econv, W.ecols, W.dh3[1], W.dh2[1], W.dh1[1], B, wl);                           // encoder trunk
    wl.push(B, P.nd, 800, W.dmu0, W.h4a, 800, wl.g(P.mean0.w), 800, wl.g(P.mean0.b));
    wl.push(B, P.nd, 800, W.dlv0, W.h4a, 800, wl.g(P.logvar0.w), 800, wl.g(P.logvar0.b));
    wl.push(B, 800, 512, W.dh4a, W.ainp, 512, wl.g(P.afc.w), 512, wl.g(P.afc.b));
    conv_trunk_wgrads(P.aconv, W.acols, W.dh3[0], W.dh2[0], W.dh1[0], B, wl);                           // aux trunk
    wl.assign(ws, AUX_WGRAD_HINT);
  }
  static size_t noise_floats(const AuxConvLayout& P, int B, int nz) { return (size_t)B * nz * (P.nd + P.zd); }
  static float* zero_noise(Entry& e, size_t) { return e.W.zero; }
  // a forward-only pass keeps the [R, 800] hidden rows only where the hidden context is wanted
  static int sampler_fwd(Entry& e, const float* params, const float* packed, const float* x, const float* noise, int B, int nz, const IpEncodeOut* enc,
                         hipStream_t st) {
    return aux_sampler_fwd(e.P, e.K, params, packed, x, noise, B, nz, e.W, !enc || enc->hidden_out != nullptr, st);
  }
  static int hidden_copy(Entry& e, float* hidden_out, int B, hipStream_t st) {      // cat(h4a, h4)
    ARDAE_TRY(launch_copy2d(e.W.h4a, 800, hidden_out, 1600, B, 800, st));
    return launch_copy2d(e.W.D.t1, 800, hidden_out + 800, 1600, B, 800, st);
  }
  static int decoder_fwd(Entry& e, const float* params, const float* packed, const float* z, int R, hipStream_t st) {
    return conv_decode_fwd(e.P.dec, e.K.dec, params, packed, z, R, e.W.D, st);
  }
  static int decoder_bwd(Entry& e, const float* packed, int R, Grads&, hipStream_t st) { return conv_decoder_bwd(e.P.dec, e.K.dec, packed, e.W.D, R, st); }
  static int sampler_bwd(Entry& e, const float*, const float* packed, const float*, const float*, int B, int nz, Grads& g, hipStream_t st) {
    auto& [P, K, ws, W] = e;
    ConvWs& D = W.D;
    const int R = B * nz, act = P.act;
    // second reparameterisation and the encoder's fc
    ARDAE_TRY(launch_reparam_bwd(D.dz, D.z, W.mu, R, P.zd, 1, W.dlv, st));
    ARDAE_TRY(dense_bwd2(act, R, 800, D.dz, packed + K.mean_b, W.dlv, packed + K.logvar_b, P.zd, D.t1, W.dt1, st));
    ARDAE_TRY(dense_fwd(ACT_NONE, R, P.nd, W.dt1, 800, 800, packed + K.efcn_b, nullptr, W.dz0, st));
    ARDAE_TRY(launch_segment_sum(W.dt1, 800, B, nz, 800, 1.0f, W.drb, 800, st));
    ARDAE_TRY(dense_fwd(ACT_NONE, B, 512, W.drb, 800, 800, packed + K.efci_b, nullptr, W.dinp_e, st));
    ARDAE_TRY(trunk_bwd(K.econv_b, packed, W.dinp_e, W.dinp_t, W.ehcv, W.dh3[1], W.dcols3[1], W.dh2[1], W.dcols2[1], W.dh1[1], B, act, st));
    // first reparameterisation, reduced over the nz samples of each image, and the aux encoder
    ARDAE_TRY(launch_reparam_bwd(W.dz0, W.z0, W.mu0, R, P.nd, nz, W.dlv0r, st));
    ARDAE_TRY(launch_segment_sum(W.dz0, P.nd, B, nz, P.nd, 1.0f, W.dmu0, P.nd, st));
    ARDAE_TRY(launch_segment_sum(W.dlv0r, P.nd, B, nz, P.nd, 1.0f, W.dlv0, P.nd, st));
    ARDAE_TRY(dense_bwd2(act, B, 800, W.dmu0, packed + K.mean0_b, W.dlv0, packed + K.logvar0_b, P.nd, W.h4a, W.dh4a, st));
    ARDAE_TRY(dense_fwd(ACT_NONE, B, 512, W.dh4a, 800, 800, packed + K.afc_b, nullptr, W.dinp_a, st));
    ARDAE_TRY(trunk_bwd(K.aconv_b, packed, W.dinp_a, W.dinp_t, W.ahcv, W.dh3[0], W.dcols3[0], W.dh2[0], W.dcols2[0], W.dh1[0], B, act, st));
    // ---- weight gradients, launched as two batches
    WgradList wl(g.grads, g.beta);
    wgrads(P, K, W, nullptr, nullptr, B, nz, wl, ws);
    ARDAE_CHECK_ARG(ws.ok, "model_vae_backward: internal workspace accounting error");
    ARDAE_TRY(wl.launch(st, AUX_WGRAD_HINT));
    return wl.launch(st);
  }
};

}  // namespace

// (host pass only: a const object with a constant initialiser is otherwise emitted for the device too, where no entry point exists)
#ifndef __HIP_DEVICE_COMPILE__
const Family CONV_FAMILY = ip_family<ConvTraits>();
const Family AUXCONV_FAMILY = ip_family<AuxConvTraits>();
#endif

}  // namespace ardae
