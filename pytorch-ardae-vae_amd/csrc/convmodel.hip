// ConvIPVAE (models/ivae/conv.py:44-245 + models/vae/conv.py:79-136; `--model mnist-conv`, BASELINE config #4) on gfx950.
//
// The reference hard-wires the architecture (28x28x1 input; conv 1->16->32->32, k5 s2 p2: 28->14->7->4; fc4 (512+noise)->800,
// fc5 800->z; decoder MLP z->300->512, ConvTranspose2d 32->32 (4->7, zero-padded to 8), 32->16 (8->15), 16->1 (15->29,
// cropped to 28)), so this file does too.  Every (transposed) convolution is im2col / col2im (two small gather kernels,
// NHWC activations as [rows = b*H*W, C]) around the FP32-MFMA linear and wgrad kernels; the conv trunk runs on B rows only,
// fc4's image half enters as a per-image row bias exactly like the MLP sampler (csrc/model.hip).
// This file: the five conv kernels and their launchers, the bodies of what csrc/convmodel.h declares for every plain-conv kind, and kind 2 itself.
#include "ardae_hip.h"
#include "common.h"
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

// ------------------------------------------------------------------------------------------------ what the conv kinds share (csrc/convmodel.h)
int conv_desc_check(const ardae_model_desc* d) {
  ARDAE_TRY(desc_flags_ok(d, 0));
  ARDAE_CHECK_ARG(d->input_dim == 784 && d->noise_dim >= 1 && d->z_dim >= 1, "model: ConvIPVAE is hard-wired to 28x28x1 inputs (input_dim 784)");
  ARDAE_CHECK_ARG(d->act > ACT_NONE && d->act <= ACT_LAST, "model: unknown activation %d (relu, softplus, elu, tanh, leaky_relu, swish)", d->act);
  return 0;
}
int conv_gauss_desc_check(const ardae_model_desc* d, const char* cls, const char* h_dim_of) {
  ARDAE_CHECK_ARG(d->input_dim == 784, "model: %s is hard-wired to 28x28x1 inputs (input_dim 784), got %d", cls, d->input_dim);
  ARDAE_CHECK_ARG(d->h_dim == 800, "model: h_dim must be 800 for kind %d (%s), got %d", d->kind, h_dim_of, d->h_dim);
  ARDAE_CHECK_ARG(d->n_layers == 1, "model: n_layers must be 1 for kind %d, got %d", d->kind, d->n_layers);
  ARDAE_CHECK_ARG(d->z_dim >= 1, "model: bad dimensions (z_dim %d)", d->z_dim);
  ARDAE_CHECK_ARG(d->act > ACT_NONE && d->act <= ACT_LAST, "model: unknown activation %d (relu, softplus, elu, tanh, leaky_relu, swish)", d->act);
  return 0;
}

// floats of conv i's im2col rows / of its output on B images
static size_t cols_floats(size_t B, int i) { return B * EH[i + 1] * EH[i + 1] * ECH[i] * 25; }
static size_t hcv_floats(size_t B, int i) { return B * EH[i + 1] * EH[i + 1] * ECH[i + 1]; }

void trunk_carve(Bump& ws, size_t B, TrunkBuf& T, const TrunkBuf* first) {
  for (int i = 0; i < 3; ++i) {
    T.cols[i] = i == 0 && first ? first->cols[0] : ws.take(cols_floats(B, i));
    T.hcv[i] = ws.take(hcv_floats(B, i));
  }
  T.inp = ws.take(hcv_floats(B, 2));
}
void trunk_bwd_carve(Bump& ws, size_t B, TrunkBuf& T, TrunkScratch* S, const TrunkScratch* first) {
  T.dinp = ws.take(hcv_floats(B, 2)); T.dh3 = ws.take(hcv_floats(B, 2)); T.dh2 = ws.take(hcv_floats(B, 1)); T.dh1 = ws.take(hcv_floats(B, 0));
  if (!S) return;
  S->dinp_t = first ? first->dinp_t : ws.take(hcv_floats(B, 2));
  S->dcols3 = ws.take(cols_floats(B, 2)); S->dcols2 = ws.take(cols_floats(B, 1));
}
void conv_decoder_carve(Bump& ws, size_t R, int zd, ConvDecRuns runs, ConvDecWs& W) {
  if (runs.head) {
    W.d1 = ws.take(R * 300); W.d2 = ws.take(R * 512); W.g0 = ws.take(R * 512);
    W.c1 = ws.take(R * 16 * 800); W.u1 = ws.take(R * 64 * 32);
  }
  if (runs.tail) {
    W.c2 = ws.take(R * 64 * 400); W.u2 = ws.take(R * 225 * 16);
    W.c3 = ws.take(R * 225 * 25); W.logit = ws.take(R * 784);
  }
  if (runs.loss) { W.rec_row = ws.take(R); W.pri_row = ws.take(R); }
  if (!runs.bwd) return;
  W.dlogit = ws.take(R * 784); W.dc3 = ws.take(R * 225 * 25); W.dp2 = ws.take(R * 225 * 16);
  W.dc2 = ws.take(R * 64 * 400); W.dp1 = ws.take(R * 64 * 32); W.dc1 = ws.take(R * 16 * 800);
  W.dg0 = ws.take(R * 512); W.dd2 = ws.take(R * 512); W.dd1 = ws.take(R * 300);
  W.dzq = ws.take(R * zd); W.dz = ws.take(R * zd); W.ones = ws.take(R * 784);
}

int trunk_fwd(const Lin* conv, const size_t* conv_f, const float* params, const float* packed, const float* x2, const TrunkBuf& T, int B, int act,
              hipStream_t st, bool cols0_ready) {
  const float* cur = x2;
  for (int i = 0; i < 3; ++i) {                                                 // conv_i = im2col + Linear([O, C*25]) + act
    const int OH = EH[i + 1], Kc = ECH[i] * 25;
    if (i > 0 || !cols0_ready) ARDAE_TRY(im2col(cur, B, EH[i], EH[i], ECH[i], OH, OH, T.cols[i], st));
    ARDAE_TRY(dense_fwd(act, B * OH * OH, ECH[i + 1], T.cols[i], Kc, Kc, packed + conv_f[i], params + conv[i].b, T.hcv[i], st));
    cur = T.hcv[i];
  }
  return launch_nhwc_nchw(T.hcv[2], B, 16, 32, T.inp, false, st);                  // h3.view(B,-1) of NCHW
}

int trunk_bwd(const size_t* conv_b, const float* packed, const TrunkBuf& T, const TrunkScratch& S, int B, int act, hipStream_t st) {
  ARDAE_TRY(launch_nhwc_nchw(T.dinp, B, 16, 32, S.dinp_t, true, st));            // NCHW-flat -> NHWC rows
  ARDAE_TRY(launch_mul_dact(S.dinp_t, T.hcv[2], act, T.dh3, (int64_t)B * 512, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, B * 16, 800, T.dh3, 32, 32, packed + conv_b[2], nullptr, S.dcols3, st));   // conv3 backward-data: dcols = dpre . W3
  ARDAE_TRY(col2im(S.dcols3, B, 4, 4, 32, 7, 7, 7, 7, nullptr, act, T.hcv[1], T.dh2, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, B * 49, 400, T.dh2, 32, 32, packed + conv_b[1], nullptr, S.dcols2, st));
  return col2im(S.dcols2, B, 7, 7, 16, 14, 14, 14, 14, nullptr, act, T.hcv[0], T.dh1, st);
}

// the decoder up to u1 [R, 8, 8, 32]: decode.fc and deconv1 with its activation and zero pad
int conv_decode_head_fwd(const ConvDecLayout& P, const ConvDecPacked& K, const float* params, const float* packed, const float* z, int R, ConvDecWs& W,
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
int conv_decode_tail_fwd(const ConvDecLayout& P, const ConvDecPacked& K, const float* params, const float* packed, const float* u1, int R, ConvDecWs& W,
                         hipStream_t st) {
  const int act = P.act;
  // deconv2 32->16: 8x8 -> 15x15, activation
  ARDAE_TRY(dense_fwd(ACT_NONE, R * 64, 400, u1, 32, 32, packed + K.dcv_f[1], nullptr, W.c2, st));
  ARDAE_TRY(col2im(W.c2, R, 8, 8, 16, 15, 15, 15, 15, params + P.dcv[1].b, act, nullptr, W.u2, st));
  // logit deconv 16->1: 15x15 -> 29x29, cropped to 28x28
  ARDAE_TRY(dense_fwd(ACT_NONE, R * 225, 25, W.u2, 16, 16, packed + K.dcv_f[2], nullptr, W.c3, st));
  return col2im(W.c3, R, 15, 15, 1, 28, 28, 28, 28, params + P.dcv[2].b, ACT_NONE, nullptr, W.logit, st);
}

int conv_decode_fwd(const ConvDecLayout& P, const ConvDecPacked& K, const float* params, const float* packed, const float* z, int R, ConvDecWs& W,
                    hipStream_t st) {
  ARDAE_TRY(conv_decode_head_fwd(P, K, params, packed, z, R, W, st));
  return conv_decode_tail_fwd(P, K, params, packed, W.u1, R, W, st);
}

// decoder backward from W.dlogit (and W.dzq = prior + seed part of dL/dz): fills dc3/dp2/dc2/dp1/dc1/dg0/dd2/dd1 and W.dz
int conv_decoder_bwd(const ConvDecLayout& P, const ConvDecPacked& K, const float* packed, ConvDecWs& W, int R, hipStream_t st) {
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
void conv_decoder_wgrads(const ConvDecLayout& P, const ConvDecWs& W, const float* z, int R, WgradList& wl) {
  // ConvTranspose2d: dW[in][out*25] = sum_rows input[row][in] * dcols[row][out*25]; its bias = sum of the output gradient
  wl.push(R * 225, 16, 25, W.u2, W.dc3, 25, wl.g(P.dcv[2].w), 25, nullptr);
  wl.push(R * 784, 1, 1, W.dlogit, W.ones, 1, wl.g(P.dcv[2].b), 1, nullptr);
  wl.push(R * 64, 32, 400, W.u1, W.dc2, 400, wl.g(P.dcv[1].w), 400, nullptr);
  wl.push(R * 225, 16, 1, W.dp2, W.ones, 1, wl.g(P.dcv[1].b), 1, nullptr);
  wl.push(R * 16, 32, 800, W.g0, W.dc1, 800, wl.g(P.dcv[0].w), 800, nullptr);
  wl.push(R * 64, 32, 1, W.dp1, W.ones, 1, wl.g(P.dcv[0].b), 1, nullptr);
  wl.push(R, 512, 300, W.dd2, W.d1, 300, wl.g(P.dfc[1].w), 300, wl.g(P.dfc[1].b));
  wl.push(R, 300, P.zd, W.dd1, z, P.zd, wl.g(P.dfc[0].w), P.zd, wl.g(P.dfc[0].b));
}

void conv_trunk_wgrads(const Lin* conv, const TrunkBuf& T, int B, WgradList& wl) {
  wl.push(B * 16, 32, 800, T.dh3, T.cols[2], 800, wl.g(conv[2].w), 800, wl.g(conv[2].b));
  wl.push(B * 49, 32, 400, T.dh2, T.cols[1], 400, wl.g(conv[1].w), 400, wl.g(conv[1].b));
  wl.push(B * 196, 16, 25, T.dh1, T.cols[0], 25, wl.g(conv[0].w), 25, wl.g(conv[0].b));
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
namespace {

struct ConvLayout {
  int nd, zd, act;
  Lin conv[3], fc4, fc5;
  ConvDecLayout dec;
  size_t total;
  explicit ConvLayout(const ardae_model_desc& d) : nd(d.noise_dim), zd(d.z_dim), act(d.act) {
    size_t off = 0;
    trunk_lins(off, conv);
    fc4 = next_lin(off, 800, 512 + nd); fc5 = next_lin(off, zd, 800);
    dec = ConvDecLayout(zd, act, off);
    total = off;
  }
};

struct ConvPacked {
  size_t conv_f[3], conv_b[3], fc4i_f, fc4i_b, fc4n_f, fc5_f, fc5_b;
  ConvDecPacked dec;
  ConvPacked(const ConvLayout& P, PackList& pl) {
    trunk_panels(P.conv, pl, conv_f, conv_b);
    pl.pair(P.fc4, fc4i_f, fc4i_b, 0, 512);                            // [800, 512 + nd]: image half both ways, noise half forward
    fc4n_f = pl.panel(P.fc4.w + 512, P.fc4.in, 800, P.nd, false);
    pl.pair(P.fc5, fc5_f, fc5_b);
    dec = ConvDecPacked(P.dec, pl);
  }
  explicit ConvPacked(const ConvLayout& P, PackList&& sizing = PackList()) : ConvPacked(P, sizing) {}   // offsets only
};

struct ConvWs {
  float* x2; TrunkBuf T; TrunkScratch S;      // encoder (B rows)
  float *rb, *t1, *z, *dt1, *drb;             // fc4's image half [B, 800]; fc4 / fc5 on R rows and their gradients
  ConvDecWs D;                                // decoder (R rows)
};

void carve(const ConvLayout& P, const ConvPacked&, Bump& ws, int B, int nz, int mode, ConvWs& W) {
  const size_t R = (size_t)B * nz;
  W.x2 = ws.take((size_t)B * 784);
  trunk_carve(ws, (size_t)B, W.T);
  W.rb = ws.take((size_t)B * 800);
  W.t1 = ws.take(R * 800); W.z = ws.take(R * P.zd);
  if (mode == 0) return;
  conv_decoder_carve(ws, R, P.zd, mode == 2 ? CONV_DEC_DECODE : CONV_DEC_TRAIN, W.D);
  if (mode == 2) return;
  W.dt1 = ws.take(R * 800); W.drb = ws.take((size_t)B * 800);
  trunk_bwd_carve(ws, (size_t)B, W.T, &W.S);
}

using ConvEntry = Entry<ConvLayout, ConvPacked, ConvWs>;

// What the shared algorithm (csrc/ipmodel.h) needs to know of ConvIPVAE.
struct ConvTraits : IpTraitsBase {
  using Layout = ConvLayout; using Packed = ConvPacked; using Ws = ConvWs; using Entry = ConvEntry;
  static int desc_check(const ardae_model_desc* d) { return conv_desc_check(d); }
  static unsigned caps(const ardae_model_desc&) { return 0; }
  static IpBufs bufs(const ConvWs& W) { return {W.z, W.D.logit, nullptr, W.D.dlogit, nullptr, W.D.dzq, W.D.dz, W.D.rec_row, W.D.pri_row}; }
  // every weight-gradient problem of the backward, with its scratch taken from ws
  static void wgrads(const ConvLayout& P, const ConvPacked&, const ConvWs& W, const float*, const float* noise, int B, int nz, WgradList& wl, Bump& ws) {
    const int R = B * nz;
    conv_decoder_wgrads(P.dec, W.D, W.z, R, wl);
    wl.push(R, P.zd, 800, W.D.dz, W.t1, 800, wl.g(P.fc5.w), 800, wl.g(P.fc5.b));
    wl.push(R, 800, P.nd, W.dt1, noise, P.nd, wl.g(P.fc4.w + 512), 512 + P.nd, wl.g(P.fc4.b));   // fc4 noise half (+ bias)
    wl.push(B, 800, 512, W.drb, W.T.inp, 512, wl.g(P.fc4.w), 512 + P.nd, nullptr);                // fc4 image half
    conv_trunk_wgrads(P.conv, W.T, B, wl);
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
    ARDAE_TRY(trunk_fwd(P.conv, K.conv_f, params, packed, W.x2, W.T, B, act, st));
    // fc4 on cat[h3 | noise]: the image half once per image
    ARDAE_TRY(cat_fwd(act, B, nz, 800, W.T.inp, 512, packed + K.fc4i_f, params + P.fc4.b, noise, P.nd, packed + K.fc4n_f, W.rb, W.t1, st));
    return dense_fwd(ACT_NONE, R, P.zd, W.t1, 800, 800, packed + K.fc5_f, params + P.fc5.b, W.z, st);
  }
  static int decoder_fwd(Entry& e, const float* params, const float* packed, const float* z, int R, hipStream_t st) {
    return conv_decode_fwd(e.P.dec, e.K.dec, params, packed, z, R, e.W.D, st);
  }
  static int decoder_bwd(Entry& e, const float* packed, int R, Grads&, hipStream_t st) { return conv_decoder_bwd(e.P.dec, e.K.dec, packed, e.W.D, R, st); }
  static int sampler_bwd(Entry& e, const float*, const float* packed, const float*, const float* noise, int B, int nz, Grads& g, hipStream_t st) {
    auto& [P, K, ws, W] = e;
    const int R = B * nz, act = P.act;
    ARDAE_TRY(dense_bwd(act, R, 800, W.D.dz, P.zd, packed + K.fc5_b, W.t1, W.dt1, st));
    ARDAE_TRY(launch_segment_sum(W.dt1, 800, B, nz, 800, 1.0f, W.drb, 800, st));
    ARDAE_TRY(dense_fwd(ACT_NONE, B, 512, W.drb, 800, 800, packed + K.fc4i_b, nullptr, W.T.dinp, st));
    ARDAE_TRY(trunk_bwd(K.conv_b, packed, W.T, W.S, B, act, st));
    // ---- weight gradients: one batched launch
    WgradList wl(g.grads, g.beta);
    wgrads(P, K, W, nullptr, noise, B, nz, wl, ws);
    ARDAE_CHECK_ARG(ws.ok, "model_vae_backward: internal workspace accounting error");
    return wl.launch(st);
  }
};

}  // namespace

// (host pass only: a const object with a constant initialiser is otherwise emitted for the device too, where no entry point exists)
#ifndef __HIP_DEVICE_COMPILE__
const Family CONV_FAMILY = ip_family<ConvTraits>();
#endif

}  // namespace ardae
