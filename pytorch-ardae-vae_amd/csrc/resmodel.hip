// Weight-normalised residual-conv VAEs on gfx950: every kernel of the residual-conv kinds, what they share (csrc/resmodel.h: the residual block, the
// trunk, the decoder of models/vae/resconv.py:79-136, the weight-norm pack and backward, the workspace pieces), the implicit kinds
//   kind 5  ResConvIPVAE           models/ivae/resconv.py:53-245 (`--model resconvct-res`: do_center, enc_type 'res-wn-mlp')
//   kind 6  MNISTResConvAuxIPVAE   models/ivae/auxresconv.py:48-255 + models/vae/auxresconv.py:26-185 (`--model auxresconvct`)
// and the entry points ardae_resconv_tail / ardae_resconv_mid.  The Gaussian kinds on the same trunk and decoder are files of their own: kind 12 in
// csrc/resvae.hip, kind 19 in csrc/auxresvae.hip.  The shipped "implicit resconv" / "hierarchical resconv" recipes (run_vae_dbmnist.sh) train kinds
// 5 / 6 with ELU, an mlp-res cDAE, --std-scale 100.
//
// Every residual block (models/layers2.py:305-352, models/layers.py:66-85) is
//     out = W_h1 f(W_0h x + b_0h) + W_01 x + (b_h1 + b_01)           f = ELU inside ResConv2d, ReLU inside ResLinear
// with weight-normalised operators W = scale * direction / ||direction|| (layers2.py:73-83,255-265; ResMLP's operators skip the
// normalisation, layers.py:47-53 with norm=False).  Here a block is TWO launches of the FP32-MFMA linear kernel: the inner
// operator, then the second operator and the skip as ONE two-source product accumulating into the same output (the concat-input
// form of ardae_linear), with 3x3 convolutions as im2col / col2im gathers around them (NHWC activations as [rows = b*H*W, C]).
// The effective weights are composed once per optimiser step (ardae_model_pack) into the packed buffer; the backward turns
// dL/dW into dL/d(direction), dL/d(scale) in one launch over all operators.  Everything per-image runs on B rows; only the
// sampler's tail runs on the B*nz Monte-Carlo rows, with the per-image half of its concat input hoisted into a row bias.
#include <vector>

#include "ardae_hip.h"
#include "auxmodel.h"
#include "common.h"
#include "resmodel.h"
#include "ipmodel.h"

namespace ardae {
namespace {

// ------------------------------------------------------------------------------------------------ kernels
// weff[o][:] = scale[o] * dir[o][:] * inv,  inv = norm ? 1 / ||dir[o][:]|| : 1   (one workgroup per output row)
// all operators of a model in ONE launch (a re-pack follows every optimiser step: ~50 launches of a few us each otherwise):
// grid (max O, items); item = one weight-normalised operator, or (dir == nullptr) a bias sum  out[i] = a[i] + b[i]
constexpr int WNC_MAX = 64;
struct WnComposeItem {
  const float* dir; const float* scale; float* weff; float* inv; int O, I, norm;   // operator: weff [O, I], inv [O]
  const float* add_a; const float* add_b;                                         // bias sum (dir == nullptr): weff[i] = add_a[i] + add_b[i], O entries
};
struct WnComposeBatch { int n; WnComposeItem it[WNC_MAX]; };
__global__ __launch_bounds__(256) void wn_compose_batch_kernel(const WnComposeBatch b) {
  __shared__ float red[256];
  const WnComposeItem& w = b.it[blockIdx.y];
  const int o = blockIdx.x, t = threadIdx.x;
  if (w.dir == nullptr) {       // bias sum
    const int i = o * 256 + t;
    if (i < w.O) w.weff[i] = w.add_a[i] + w.add_b[i];
    return;
  }
  if (o >= w.O) return;
  const float* d = w.dir + (size_t)o * w.I;
  float s = 0.f;
  for (int i = t; i < w.I; i += 256) s += d[i] * d[i];
  red[t] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (t < k) red[t] += red[t + k];
    __syncthreads();
  }
  const float inv = w.norm ? 1.f / sqrtf(red[0]) : 1.f;
  const float f = w.scale[o] * inv;
  for (int i = t; i < w.I; i += 256) w.weff[(size_t)o * w.I + i] = f * d[i];
  if (t == 0) w.inv[o] = inv;
}

// dL/dW [O, I] -> dL/ddir, dL/dscale (and the bias gradients, plain copies) for up to WNB_MAX operators in one launch
constexpr int WNB_MAX = 48;
struct WnBwdBatch { int n; float beta; WnBwdItem it[WNB_MAX]; };
__global__ __launch_bounds__(256) void wn_backward_kernel(const WnBwdBatch b) {
  __shared__ float red[256];
  const WnBwdItem& w = b.it[blockIdx.y];
  const int t = threadIdx.x;
  for (int o = blockIdx.x; o < w.O; o += gridDim.x) {
    const float* dW = w.dW + (size_t)o * w.I;
    const float* d = w.dir + (size_t)o * w.I;
    float s = 0.f;
    for (int i = t; i < w.I; i += 256) s += dW[i] * d[i];
    __syncthreads();
    red[t] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
      if (t < k) red[t] += red[t + k];
      __syncthreads();
    }
    const float s1 = red[0], inv = w.inv[o], sc = w.scale[o];
    const float f = sc * inv, c = w.norm ? inv * inv * s1 : 0.f;
    float* gd = w.gdir + (size_t)o * w.I;
    for (int i = t; i < w.I; i += 256) {
      const float v = f * (dW[i] - d[i] * c);
      gd[i] = b.beta != 0.f ? b.beta * gd[i] + v : v;
    }
    if (t == 0) {
      w.gscale[o] = (b.beta != 0.f ? b.beta * w.gscale[o] : 0.f) + s1 * inv;
      w.gbias[o] = (b.beta != 0.f ? b.beta * w.gbias[o] : 0.f) + w.db[o];
    }
  }
}

// cols[(b*OH+oh)*OW+ow][c*9+kh*3+kw] = x[b][s*oh-1+kh][s*ow-1+kw][c]  (0 outside); x NHWC [B,H,W,C]: 3x3, padding 1, stride s
__global__ void im2col3_kernel(const float* __restrict__ x, int H, int W, int C, int OH, int OW, int s, float* __restrict__ cols, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int J = C * 9;
  const int j = (int)(e % J);
  const int64_t row = e / J;
  const int ow = (int)(row % OW), oh = (int)((row / OW) % OH);
  const int64_t b = row / ((int64_t)OW * OH);
  const int c = j / 9, kk = j - c * 9, kh = kk / 3, kw = kk - kh * 3;
  const int h = s * oh - 1 + kh, w = s * ow - 1 + kw;
  cols[e] = (h >= 0 && h < H && w >= 0 && w < W) ? x[((b * H + h) * W + w) * C + c] : 0.f;
}

// transpose of im2col3 as a gather: dx[b][h][w][c] = sum_{kh,kw: (h+1-kh) % s == 0, oh = (h+1-kh)/s in range} dcols[(b,oh,ow)][c*9+kh*3+kw]
// mulS: multiply by act'(S[e]) on the way out (the activation in front of the convolution: one launch less per block)
__global__ void col2im3_kernel(const float* __restrict__ dcols, int H, int W, int C, int OH, int OW, int s, float* __restrict__ dx, int64_t total,
                               const float* __restrict__ mulS, int act) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % C);
  const int64_t pix = e / C;
  const int w = (int)(pix % W), h = (int)((pix / W) % H);
  const int64_t b = pix / ((int64_t)W * H);
  float v = 0.f;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int th = h + 1 - kh;
    if (th < 0 || th % s) continue;
    const int oh = th / s;
    if (oh >= OH) continue;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int tw = w + 1 - kw;
      if (tw < 0 || tw % s) continue;
      const int ow = tw / s;
      if (ow >= OW) continue;
      v += dcols[((b * OH + oh) * OW + ow) * (int64_t)(C * 9) + c * 9 + kh * 3 + kw];
    }
  }
  dx[e] = mulS ? v * act_d1_rt(act, mulS[e]) : v;
}

__global__ void act_inplace_kernel(float* __restrict__ x, int act, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) x[e] = act_fwd_rt(act, x[e]);
}

// bilinear x2 upsampling, align_corners=True (nn.Upsample in models/vae/resconv.py:96-106), NHWC; src = o (IH-1)/(OH-1)
__device__ __forceinline__ void up_src(int o, int IH, int OH, int& i0, int& i1, float& f) {
  const float s = OH > 1 ? (float)o * (float)(IH - 1) / (float)(OH - 1) : 0.f;
  i0 = (int)floorf(s);
  if (i0 > IH - 1) i0 = IH - 1;
  i1 = i0 + 1 < IH ? i0 + 1 : IH - 1;
  f = s - (float)i0;
}
__global__ void upsample2_fwd_kernel(const float* __restrict__ x, int IH, int C, float* __restrict__ y, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int OH = 2 * IH;
  const int c = (int)(e % C);
  const int64_t pix = e / C;
  const int ow = (int)(pix % OH), oh = (int)((pix / OH) % OH);
  const int64_t b = pix / ((int64_t)OH * OH);
  int h0, h1, w0, w1; float fh, fw;
  up_src(oh, IH, OH, h0, h1, fh); up_src(ow, IH, OH, w0, w1, fw);
  const float* xb = x + b * (int64_t)IH * IH * C + c;
  const float v00 = xb[(h0 * IH + w0) * C], v01 = xb[(h0 * IH + w1) * C], v10 = xb[(h1 * IH + w0) * C], v11 = xb[(h1 * IH + w1) * C];
  y[e] = (1.f - fh) * ((1.f - fw) * v00 + fw * v01) + fh * ((1.f - fw) * v10 + fw * v11);
}
// transpose as a gather over the (few) output pixels that read input pixel (ih, iw)
__global__ void upsample2_bwd_kernel(const float* __restrict__ dy, int IH, int C, float* __restrict__ dx, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int OH = 2 * IH;
  const int c = (int)(e % C);
  const int64_t pix = e / C;
  const int iw = (int)(pix % IH), ih = (int)((pix / IH) % IH);
  const int64_t b = pix / ((int64_t)IH * IH);
  // outputs o with floor(src(o)) in {i-1, i}: src(o) in (i-1, i+1)  ->  o in ((i-1) r, (i+1) r), r = (OH-1)/(IH-1)
  const float r = IH > 1 ? (float)(OH - 1) / (float)(IH - 1) : 1.f;
  int lo_h = (int)floorf((float)(ih - 1) * r) - 1, hi_h = (int)ceilf((float)(ih + 1) * r) + 1;
  int lo_w = (int)floorf((float)(iw - 1) * r) - 1, hi_w = (int)ceilf((float)(iw + 1) * r) + 1;
  if (lo_h < 0) lo_h = 0; if (lo_w < 0) lo_w = 0;
  if (hi_h > OH - 1) hi_h = OH - 1; if (hi_w > OH - 1) hi_w = OH - 1;
  const float* dyb = dy + b * (int64_t)OH * OH * C + c;
  float v = 0.f;
  for (int oh = lo_h; oh <= hi_h; ++oh) {
    int h0, h1; float fh;
    up_src(oh, IH, OH, h0, h1, fh);
    const float wh = (h0 == ih ? 1.f - fh : 0.f) + (h1 == ih ? fh : 0.f);
    if (wh == 0.f) continue;
    for (int ow = lo_w; ow <= hi_w; ++ow) {
      int w0, w1; float fw;
      up_src(ow, IH, OH, w0, w1, fw);
      const float ww = (w0 == iw ? 1.f - fw : 0.f) + (w1 == iw ? fw : 0.f);
      if (ww != 0.f) v += wh * ww * dyb[(oh * OH + ow) * C];
    }
  }
  dx[e] = v;
}
// [B, HS, HS, C] -> [B, HD, HD, C]: crop (HD < HS: slicer[:, :, :-1, :-1]) or zero-pad (HD > HS: its transpose)
__global__ void crop_pad_kernel(const float* __restrict__ x, int HS, int HD, int C, float* __restrict__ y, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % C);
  const int64_t pix = e / C;
  const int w = (int)(pix % HD), h = (int)((pix / HD) % HD);
  const int64_t b = pix / ((int64_t)HD * HD);
  y[e] = (h < HS && w < HS) ? x[((b * HS + h) * HS + w) * C + c] : 0.f;
}
// NormalDistribution.clip_logvar 'spm4' (models/reparam.py:30-31): y = softplus(x + 4) - 4; backward: dx = dy * sigmoid(x + 4)
// identity != 0 (the clipped class of ivae/auxresconv2.py:71-72 builds its heads WITHOUT the clip): y = x, dx = dy
__global__ void spm4_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ y, int64_t n, int identity) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  if (identity) { y[e] = dy ? dy[e] : x[e]; return; }
  const float u = x[e] + 4.f;
  if (dy) y[e] = dy[e] / (1.f + expf(-u));
  else y[e] = (u > 20.f ? u : log1pf(expf(u))) - 4.f;
}

// The decoder's last stage as ONE launch (kind 12's decode-only path; ardae_resconv_tail variant 1): upsample 14 -> 28 (up_src and the expression
// of upsample2_fwd_kernel), then dec[6] = ResConv2d(16 -> 1):  hmid = ELU(conv3x3_a(u28) + b_a),  logit = conv3x3_h(hmid) + conv3x3_s(u28) + (b_h + b_s).
// One workgroup per image; nothing but the 784 logits leaves the chip (the unfused launches write u28, two column matrices and hmid: ~134k floats a row).
//   LDS: u28 as 16 channel planes of 30 x 30 (a zero halo: the padding taps read it), hmid as one such plane, the 2 x 144 + 9 effective weights: 64.3 KB,
//        two workgroups a CU.  4-byte reads and every write bank on word % 32 and conflict within a 32-lane half: the planes are planar and a half-wave
//        owns ONE image row (28 of its 32 lanes), so its reads are 28 consecutive words - no conflict; the weight reads are broadcasts.  The
//        interpolation walks (pixel, channel) with the channel fastest: coalesced reads of the NHWC y14 (L2 / L1 resident, each value read by at most
//        four outputs), and the plane stride 930 = 2 mod 32 puts a half-wave's 16 channels x 2 pixels on 32 different banks.
//   Work: half-wave r < 7 owns rows r, r + 7, r + 14, r + 21, a lane one column position in them: a channel's 18 weights are read once for the four
//        pixels, 72 FMAs against 36 + 18 LDS reads.  Each pixel's sums run over ascending (c, kh, kw) from zero, the biases added last, whatever R is:
//        a row's bits do not depend on the rows of the call.
constexpr int RT_THREADS = 256, RT_PIX = 4, RT_C = 16, RT_P = 30, RT_PLANE = RT_P * RT_P, RT_STRIDE = RT_PLANE + 30, RT_HALO = 4 * RT_P - 4;
__global__ __launch_bounds__(RT_THREADS) void resconv_tail_kernel(const float* __restrict__ y14, const float* __restrict__ wa, const float* __restrict__ ba,
                                                                  const float* __restrict__ wh, const float* __restrict__ wsk,
                                                                  const float* __restrict__ bsum, float* __restrict__ logits) {
  __shared__ float u[RT_C * RT_STRIDE];
  __shared__ float hm[RT_PLANE];
  __shared__ float w_a[RT_C * 9], w_s[RT_C * 9], w_h[12];
  const int t = threadIdx.x;
  const float* __restrict__ yb = y14 + (size_t)blockIdx.x * (196 * RT_C);
  for (int i = t; i < RT_C * 9; i += RT_THREADS) { w_a[i] = wa[i]; w_s[i] = wsk[i]; }
  if (t < 9) w_h[t] = wh[t];
  // the zero halo of the 16 + 1 planes: top row, bottom row, then the two end cells of rows 1 .. 28
  for (int i = t; i < (RT_C + 1) * RT_HALO; i += RT_THREADS) {
    const int c = i / RT_HALO, j = i - c * RT_HALO;
    int r, q;
    if (j < RT_P) { r = 0; q = j; }
    else if (j < 2 * RT_P) { r = RT_P - 1; q = j - RT_P; }
    else { const int k = j - 2 * RT_P; r = 1 + (k >> 1); q = (k & 1) ? RT_P - 1 : 0; }
    float* plane = c < RT_C ? u + c * RT_STRIDE : hm;
    plane[r * RT_P + q] = 0.f;
  }
  for (int e = t; e < 784 * RT_C; e += RT_THREADS) {
    const int c = e & (RT_C - 1), pix = e >> 4, ow = pix % 28, oh = pix / 28;
    int h0, h1, w0, w1; float fh, fw;
    up_src(oh, 14, 28, h0, h1, fh); up_src(ow, 14, 28, w0, w1, fw);
    const float* xb = yb + c;
    const float v00 = xb[(h0 * 14 + w0) * RT_C], v01 = xb[(h0 * 14 + w1) * RT_C], v10 = xb[(h1 * 14 + w0) * RT_C], v11 = xb[(h1 * 14 + w1) * RT_C];
    u[c * RT_STRIDE + (oh + 1) * RT_P + ow + 1] = (1.f - fh) * ((1.f - fw) * v00 + fw * v01) + fh * ((1.f - fw) * v10 + fw * v11);
  }
  __syncthreads();
  const int w = t & 31, hb = t >> 5;          // pixel i of the thread: (hb + 7 i, w); padded position of tap (kh, kw): (hb + 7 i + kh, w + kw)
  const bool on = hb < 28 / RT_PIX && w < 28;
  float aa[RT_PIX], as[RT_PIX];
#pragma unroll
  for (int i = 0; i < RT_PIX; ++i) aa[i] = as[i] = 0.f;
  if (on) {
#pragma unroll 2
    for (int c = 0; c < RT_C; ++c) {
      float ka[9], ks[9];
#pragma unroll
      for (int j = 0; j < 9; ++j) { ka[j] = w_a[c * 9 + j]; ks[j] = w_s[c * 9 + j]; }
      const float* uc = u + c * RT_STRIDE + hb * RT_P + w;
#pragma unroll
      for (int i = 0; i < RT_PIX; ++i)
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            const float v = uc[(7 * i + kh) * RT_P + kw];
            aa[i] = __builtin_fmaf(ka[kh * 3 + kw], v, aa[i]);
            as[i] = __builtin_fmaf(ks[kh * 3 + kw], v, as[i]);
          }
    }
    const float b = ba[0];
#pragma unroll
    for (int i = 0; i < RT_PIX; ++i) hm[(hb + 7 * i + 1) * RT_P + w + 1] = act_fwd_rt(ACT_ELU, aa[i] + b);
  }
  __syncthreads();
  if (on) {
    const float bs = bsum[0];
    float* __restrict__ out = logits + (size_t)blockIdx.x * 784;
#pragma unroll
    for (int i = 0; i < RT_PIX; ++i) {
      float o = 0.f;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) o = __builtin_fmaf(w_h[kh * 3 + kw], hm[(hb + 7 * i + kh) * RT_P + w + kw], o);
      out[(hb + 7 * i) * 28 + w] = (o + as[i]) + bs;
    }
  }
}

// The decoder's 14 x 14 stage as ONE launch (kind 19's decode-only path; ardae_resconv_mid variant 1): crop dec[3]'s output y8 [R, 8, 8, 32] to 7 x 7
// (slicer[:, :, :-1, :-1]), upsample 7 -> 14 (up_src and the expression of upsample2_fwd_kernel), dec[4] = ResConv2d(32 -> 16) + ELU and
// dec[5] = ResConv2d(16 -> 16) + ELU; writes y14 [R, 14, 14, 16], which resconv_tail_kernel reads.  One workgroup of four waves per image, so a row's
// bits do not depend on the rows of the call; per row 8 KiB come in and 12.25 KiB go out (the unfused launches write and re-read ~141k column floats).
//   Products: v_mfma_f32_16x16x4_f32, M = 16 output positions (p = 14 oh + ow; 196 = 12 tiles + one of 4), N = the 16 output channels, K walking
//        c * 9 + kh * 3 + kw in the order of the effective weights, four per instruction.  Lane l holds A[m = l & 15][k = l >> 4], gathered from the
//        planes by one ds_read_b32, B[k = l >> 4][n = l & 15] and D[m = 4 (l >> 4) + i][n = l & 15], i < 4.  conv_0h and conv_01 of a block read the
//        same A: one gather feeds two MFMAs.  Wave w owns tiles w, w + 4, w + 8 (wave 0 also tile 12) and reads a k-step's B once for all of them;
//        the pad lanes of tile 12 gather position 195 again (inside LDS) and their results are never stored.  conv_01's sums stay in registers and
//        seed conv_h1's accumulators; the block's bias sum and the ELU come last.
//   B:   resconv_mid_pack_kernel lays the six effective weights out so that lane l's values of four consecutive k-steps are one float4:
//        wp[(g * 64 + l) * 4 + j] = weff[n = l & 15][k = 16 g + 4 j + (l >> 4)] - a wave reads 1 KiB per load, coalesced, the four waves the same lines.
//   LDS: channel planes of 16 x 16 (position (oh, ow) at (oh + 1, ow + 1); the zero halo is what the padding taps read) at a plane stride of 272
//        floats: u14 32 planes (34 KiB); dec[4]'s hidden map 16 planes (17 KiB); dec[4]'s output goes where u14's first 16 planes were once dec[4]
//        has read them, dec[5]'s hidden map where dec[4]'s was; y8 staged as [64][33] (8.25 KiB) - 59.25 KiB, two workgroups a CU.
//        Banks (word % 32, conflicts counted within a 32-lane half): in a gather lanes 0 .. 15 read one tap at 16 consecutive positions, words
//        a .. a + 13, a + 16, a + 17 (the tile crosses one image row); lanes 16 .. 31 read the next k: the same words shifted by 1 (next kw) or 14 (next
//        kh) - 32 consecutive words, shared ones broadcast - or by 272 - 34 = 14 mod 32 (next channel): no conflict, which is what the stride is for.
//        The epilogue's plane writes have lanes 0 .. 15 on 16 planes, stride 272 = 16 mod 32: 8-way, 12 .. 16 such writes a wave and stage against
//        ~300 MFMAs.  The interpolation walks (channel, pixel) with the pixel fastest: plane writes on consecutive words, y8's stage read at
//        (pos * 33 + c), pos within 9 of each other in a half: distinct banks or the same word.
constexpr int RM_THREADS = 256, RM_STRIDE = 272, RM_U = 32 * RM_STRIDE, RM_H = 16 * RM_STRIDE, RM_Y8 = 64 * 33;
// offsets of the six operators in the packed mid weights: dec[4].a, dec[4].s (K = 288), dec[4].h, dec[5].a, dec[5].s, dec[5].h (K = 144)
constexpr int RM_W4A = 0, RM_W4S = 16 * 288, RM_W4H = 2 * 16 * 288, RM_W5A = RM_W4H + 16 * 144, RM_W5S = RM_W5A + 16 * 144, RM_W5H = RM_W5S + 16 * 144;
static_assert(RM_W5H + 16 * 144 == RM_WTOTAL, "csrc/resmodel.h reserves the packed mid weights");
using f32x4 = float __attribute__((ext_vector_type(4)));

struct MidPackArgs { const float* weff[6]; int K[6], off[6]; };
__global__ void resconv_mid_pack_kernel(const MidPackArgs a, float* __restrict__ wp) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= RM_WTOTAL) return;
  int o = 5;
  while (o > 0 && e < a.off[o]) --o;
  const int i = e - a.off[o], g = i >> 8, l = (i >> 2) & 63, j = i & 3;
  wp[e] = a.weff[o][(l & 15) * a.K[o] + 16 * g + 4 * j + (l >> 4)];
}

// acc0[t] (+ acc1[t] where DUAL) += the 3 x 3 convolution of the CIN planes at src with the packed weights w0 (w1), for the wave's tiles t
template <int CIN, bool DUAL>
__device__ __forceinline__ void rm_conv(const float* src, const float4* __restrict__ w0, const float4* __restrict__ w1, int lane, int wave,
                                        const int (&base)[4], f32x4 (&acc0)[4], f32x4 (&acc1)[4]) {
  const int kq = lane >> 4;
#pragma unroll 1
  for (int g = 0; g < CIN * 9 / 16; ++g) {
    const float4 f0 = w0[g * 64 + lane];
    float4 f1 = f0;
    if (DUAL) f1 = w1[g * 64 + lane];
    const float b0[4] = {f0.x, f0.y, f0.z, f0.w}, b1[4] = {f1.x, f1.y, f1.z, f1.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = 16 * g + 4 * j + kq, c = k / 9, r = k - 9 * c, kh = r / 3, kw = r - 3 * kh;
      const float* p = src + c * RM_STRIDE + kh * 16 + kw;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t < 3 || wave == 0) {          // wave-uniform: tile wave + 4 t < 13
          const float a = p[base[t]];
          acc0[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0[j], acc0[t], 0, 0, 0);
          if (DUAL) acc1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1[j], acc1[t], 0, 0, 0);
        }
      }
    }
  }
}
// ELU(acc + bias[n]) of the wave's tiles into the planes at dst, or (GLOBAL) into the image's NHWC rows [196, 16]
template <bool GLOBAL>
__device__ __forceinline__ void rm_store(const f32x4 (&acc)[4], const float* __restrict__ bias, int lane, int wave, float* dst) {
  const int n = lane & 15, m0 = 4 * (lane >> 4);
  const float b = bias[n];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t < 3 || wave == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int p = 16 * (wave + 4 * t) + m0 + i;
        if (p < 196) {
          const float v = act_fwd_rt(ACT_ELU, acc[t][i] + b);
          if (GLOBAL) dst[p * 16 + n] = v;
          else dst[n * RM_STRIDE + (p / 14 + 1) * 16 + p % 14 + 1] = v;
        }
      }
    }
  }
}
__global__ __launch_bounds__(RM_THREADS) void resconv_mid_kernel(const float* __restrict__ y8, const float* __restrict__ wp, const float* __restrict__ ba4,
                                                                 const float* __restrict__ bs4, const float* __restrict__ ba5,
                                                                 const float* __restrict__ bs5, float* __restrict__ y14) {
  __shared__ float u[RM_U];          // u14; then dec[4]'s output in its first 16 planes
  __shared__ float hm[RM_H];         // dec[4]'s hidden map, then dec[5]'s
  __shared__ float y8s[RM_Y8];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float* __restrict__ yb = y8 + (size_t)blockIdx.x * 2048;
  for (int i = t; i < RM_U; i += RM_THREADS) u[i] = 0.f;
  for (int i = t; i < RM_H; i += RM_THREADS) hm[i] = 0.f;
  for (int e = t; e < 2048; e += RM_THREADS) y8s[(e >> 5) * 33 + (e & 31)] = yb[e];
  __syncthreads();
  // crop + upsample: source rows / columns 0 .. 6 only (IH = 7 on the stride-8 map)
  for (int e = t; e < 196 * 32; e += RM_THREADS) {
    const int c = e / 196, pix = e - c * 196, oh = pix / 14, ow = pix - oh * 14;
    int h0, h1, w0, w1; float fh, fw;
    up_src(oh, 7, 14, h0, h1, fh); up_src(ow, 7, 14, w0, w1, fw);
    const float* xb = y8s + c;
    const float v00 = xb[(h0 * 8 + w0) * 33], v01 = xb[(h0 * 8 + w1) * 33], v10 = xb[(h1 * 8 + w0) * 33], v11 = xb[(h1 * 8 + w1) * 33];
    u[c * RM_STRIDE + (oh + 1) * 16 + ow + 1] = (1.f - fh) * ((1.f - fw) * v00 + fw * v01) + fh * ((1.f - fw) * v10 + fw * v11);
  }
  int base[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int p = 16 * (wave + 4 * j) + (lane & 15);
    if (p > 195) p = 195;
    base[j] = (p / 14) * 16 + p % 14;
  }
  const float4* __restrict__ w4 = reinterpret_cast<const float4*>(wp);
  f32x4 aa[4], as[4];
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) aa[j] = as[j] = zero;
  __syncthreads();
  // dec[4]: hidden = ELU(conv_0h(u14) + b_0h), skip = conv_01(u14); out = ELU(conv_h1(hidden) + skip + (b_h1 + b_01))
  rm_conv<32, true>(u, w4 + RM_W4A / 4, w4 + RM_W4S / 4, lane, wave, base, aa, as);
  rm_store<false>(aa, ba4, lane, wave, hm);
  __syncthreads();                   // every wave has read u14 and written its part of the hidden map
  rm_conv<16, false>(hm, w4 + RM_W4H / 4, nullptr, lane, wave, base, as, aa);
  rm_store<false>(as, bs4, lane, wave, u);
#pragma unroll
  for (int j = 0; j < 4; ++j) aa[j] = as[j] = zero;
  __syncthreads();
  // dec[5] on dec[4]'s output
  rm_conv<16, true>(u, w4 + RM_W5A / 4, w4 + RM_W5S / 4, lane, wave, base, aa, as);
  rm_store<false>(aa, ba5, lane, wave, hm);
  __syncthreads();
  rm_conv<16, false>(hm, w4 + RM_W5H / 4, nullptr, lane, wave, base, as, aa);
  rm_store<true>(as, bs5, lane, wave, y14 + (size_t)blockIdx.x * (196 * 16));
}

#define RES_LAUNCH(kernel, n, ...)                                                          \
  do {                                                                                        \
    hipLaunchKernelGGL(kernel, dim3(nblk(n)), dim3(256), 0, st, __VA_ARGS__);                 \
    ARDAE_LAUNCH_CHECK();                                                                     \
  } while (0)

}  // namespace

// ================================================================================================ what the residual-conv kinds share (csrc/resmodel.h)
int res_gauss_desc_check(const ardae_model_desc* d, const char* cls, const char* elu_assert) {
  ARDAE_CHECK_ARG((d->flags & ~ARDAE_MODEL_NO_CENTER) == 0, "model: flags must be 0 or ARDAE_MODEL_NO_CENTER for kind %d, got %d", d->kind, d->flags);
  ARDAE_CHECK_ARG(d->input_dim == 784, "model: %s is hard-wired to 28x28x1 inputs (input_dim 784), got %d", cls, d->input_dim);
  ARDAE_CHECK_ARG(d->n_layers == 1, "model: n_layers must be 1 for kind %d, got %d", d->kind, d->n_layers);
  ARDAE_CHECK_ARG(d->h_dim >= 1 && d->z_dim >= 1, "model: bad dimensions (h_dim = c_dim %d, z_dim %d)", d->h_dim, d->z_dim);
  ARDAE_CHECK_ARG(d->act == ACT_ELU, "model: kind %d takes ELU only (--model-nonlin elu; %s asserts it), got activation %d", d->kind, elu_assert, d->act);
  return 0;
}

// ------------------------------------------------------------------------------------------------ workspace carving
size_t blk_rows(const Blk& b, int images) { return (size_t)images * b.Hout * b.Hout; }
void blk_carve(const Blk& b, int images, Bump& ws, BlkBuf& u) {
  const size_t R = blk_rows(b, images);
  u.colsx = b.conv ? ws.take(R * b.a.I) : nullptr;
  u.hmid = ws.take(R * b.Cout);
  u.colsh = b.conv ? ws.take(R * b.h.I) : nullptr;
  u.out = ws.take(R * b.Cout);
}
static size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }

void res_trunk_carve(const ResLayout& P, Bump& ws, int B, ResWs& W) {
  W.x2 = ws.take((size_t)B * 784);
  W.tb.resize(P.trunk.size());
  for (size_t i = 0; i < P.trunk.size(); ++i) blk_carve(P.trunk[i], B, ws, W.tb[i]);
  W.flat = ws.take((size_t)B * 512);
  W.inp = W.tb.back().out;
}

void res_decoder_carve(const ResLayout& P, Bump& ws, size_t R, DecRuns runs, ResWs& W) {
  auto on = [&](size_t i) { return i < 4 || (i < 6 ? runs.mid : runs.tail); };
  float *colsx = nullptr, *colsh = nullptr;
  if (!runs.keep) {
    size_t cx = 0, ch = 0;
    for (size_t i = 0; i < P.dec.size(); ++i)
      if (on(i) && P.dec[i].conv) { cx = max_sz(cx, blk_rows(P.dec[i], (int)R) * P.dec[i].a.I); ch = max_sz(ch, blk_rows(P.dec[i], (int)R) * P.dec[i].h.I); }
    colsx = ws.take(cx); colsh = ws.take(ch);
  }
  W.db.assign(P.dec.size(), BlkBuf{nullptr, nullptr, nullptr, nullptr});
  for (size_t i = 0; i < P.dec.size(); ++i) {
    const Blk& b = P.dec[i];
    const size_t rows = blk_rows(b, (int)R);
    BlkBuf& u = W.db[i];
    if (on(i)) {          // blk_carve's order
      u.colsx = !b.conv ? nullptr : runs.keep ? ws.take(rows * b.a.I) : colsx;
      u.hmid = ws.take(rows * b.Cout);
      u.colsh = !b.conv ? nullptr : runs.keep ? ws.take(rows * b.h.I) : colsh;
    }
    if (on(i) || i == 5) u.out = ws.take(rows * b.Cout);
  }
  W.d4 = ws.take(R * 512); W.u8 = ws.take(R * 64 * 32);
  W.c7 = runs.mid ? ws.take(R * 49 * 32) : nullptr; W.u14 = runs.mid ? ws.take(R * 196 * 32) : nullptr;
  W.u28 = runs.tail ? ws.take(R * 784 * 16) : nullptr;
}

void res_bwd_carve(const ResLayout& P, Bump& ws, int B, size_t R, size_t head_wgrad_floats, ResWs& W) {
  W.rec_row = ws.take(R); W.pri_row = ws.take(R); W.dlogit = ws.take(R * 784); W.dzq = ws.take(R * P.zd);
  // the largest per-block scratch: decoder convs at 28 x 28 (R images) and the trunk's first convs (B images)
  size_t mg = 0, mc = 0;
  auto upd = [&](const Blk& b, size_t images) {
    const size_t rows = images * b.Hout * b.Hout;
    mg = max_sz(mg, rows * b.Cout);
    mc = max_sz(mc, rows * max_sz(b.h.I, b.a.I));
  };
  for (auto& b : P.trunk) upd(b, B);
  for (auto& b : P.dec) upd(b, R);
  W.sc.g = ws.take(mg); W.sc.dh = ws.take(mg); W.sc.dcols = ws.take(mc);
  const size_t act_max = max_sz(R * 784 * 16, (size_t)B * 196 * 16);     // largest activation map (decoder 28 x 28 x 16)
  W.da = ws.take(act_max); W.dbuf = ws.take(act_max);
  W.dflat = ws.take((size_t)B * 512); W.dinp = ws.take((size_t)B * P.cdim);
  W.dR0 = ws.take(R * max_sz(P.hdim, P.cdim)); W.dR1 = ws.take(R * max_sz(P.hdim, P.cdim));
  W.dB0 = ws.take((size_t)B * max_sz(P.hdim, P.cdim)); W.dB1 = ws.take((size_t)B * max_sz(P.hdim, P.cdim)); W.dB2 = ws.take((size_t)B * max_sz(P.hdim, P.cdim));
  W.dweff = ws.take(P.total); W.dbias = ws.take(P.total / 8 + 4096);
  size_t wsf = head_wgrad_floats;
  auto wupd = [&](const Blk& b, size_t images) {
    const int rows = (int)(images * b.Hout * b.Hout);
    wsf = max_sz(wsf, wgrad_scratch_floats(rows, b.Cout, b.h.I) + wgrad_scratch_floats(rows, b.Cout, b.s.I) + wgrad_scratch_floats(rows, b.Cout, b.a.I));
  };
  for (auto& b : P.trunk) wupd(b, B);
  for (auto& b : P.dec) wupd(b, R);
  W.wscratch_floats = wsf + 1024;
  W.wscratch = ws.take(W.wscratch_floats);
}

// ------------------------------------------------------------------------------------------------ forward pieces
int blk_fwd(const Blk& b, const BlkPk& k, const float* params, const float* packed, const float* x, int images, int act_out, BlkBuf& u, hipStream_t st) {
  const int R = (int)blk_rows(b, images);
  const float* cx = x;
  if (b.conv) {
    RES_LAUNCH(im2col3_kernel, (int64_t)R * b.a.I, x, b.Hin, b.Hin, b.Cin, b.Hout, b.Hout, b.stride, u.colsx, (int64_t)R * b.a.I);
    cx = u.colsx;
  }
  // conv blocks: ELU as the epilogue activation (their Cout <= 32 columns run on the generic kernel either way)
  ARDAE_TRY(dense_fwd(b.conv ? ACT_ELU : ACT_RELU, R, b.Cout, cx, b.a.I, b.a.I, packed + k.a.f, params + b.a.bias, u.hmid, st));
  const float* ch = u.hmid;
  if (b.conv) {
    RES_LAUNCH(im2col3_kernel, (int64_t)R * b.h.I, u.hmid, b.Hout, b.Hout, b.Cout, b.Hout, b.Hout, 1, u.colsh, (int64_t)R * b.h.I);
    ch = u.colsh;
  }
  LinArgs A{}; A.bias = packed + k.bsum; A.Y = u.out; A.ldY = b.Cout;
  // the activation behind a conv block rides in the epilogue too; linear blocks keep it apart (their h-wide N-row products stay
  // eligible for the software-pipelined kernel, which is not instantiated for ELU)
  const int act_epi = b.conv ? act_out : ACT_NONE;
  ARDAE_TRY(lin2(EPI_ACT, act_epi, R, b.Cout, ch, b.h.I, b.h.I, packed + k.h.f, cx, b.a.I, b.s.I, packed + k.s.f, A, st));
  if (act_out != act_epi) RES_LAUNCH(act_inplace_kernel, (int64_t)R * b.Cout, u.out, act_out, (int64_t)R * b.Cout);
  return 0;
}

int tail_fused(const Blk& b, const BlkPk& k, const float* params, const float* packed, const float* y14, int R, float* logits, hipStream_t st) {
  hipLaunchKernelGGL(resconv_tail_kernel, dim3((unsigned)R), dim3(RT_THREADS), 0, st, y14, packed + k.a.weff, params + b.a.bias, packed + k.h.weff,
                     packed + k.s.weff, packed + k.bsum, logits);
  ARDAE_LAUNCH_CHECK();
  return 0;
}
static bool knob_off(const char* name) {
  const char* knob = debug_knob(name);
  return !(knob && knob[0] == '1');
}
bool tail_fused_default() { return knob_off("ARDAE_RESCONV_TAIL_UNFUSED"); }
bool mid_fused_default() { return knob_off("ARDAE_RESCONV_MID_UNFUSED"); }
int mid_fused(const ResLayout& P, const ResPacked& K, const float* params, const float* packed, const float* mid_w, const float* y8, int R, float* y14,
              hipStream_t st) {
  hipLaunchKernelGGL(resconv_mid_kernel, dim3((unsigned)R), dim3(RM_THREADS), 0, st, y8, mid_w, params + P.dec[4].a.bias, packed + K.dec[4].bsum,
                     params + P.dec[5].a.bias, packed + K.dec[5].bsum, y14);
  ARDAE_LAUNCH_CHECK();
  return 0;
}
int mid_unfused(const ResLayout& P, const ResPacked& K, const float* params, const float* packed, const float* y8, int R, float* c7, float* u14, BlkBuf& u4,
                BlkBuf& u5, hipStream_t st) {
  RES_LAUNCH(crop_pad_kernel, (int64_t)R * 49 * 32, y8, 8, 7, 32, c7, (int64_t)R * 49 * 32);    // slicer[:, :, :-1, :-1]
  RES_LAUNCH(upsample2_fwd_kernel, (int64_t)R * 196 * 32, (const float*)c7, 7, 32, u14, (int64_t)R * 196 * 32);
  ARDAE_TRY(blk_fwd(P.dec[4], K.dec[4], params, packed, u14, R, ACT_ELU, u4, st));
  return blk_fwd(P.dec[5], K.dec[5], params, packed, u4.out, R, ACT_ELU, u5, st);
}

int res_trunk_fwd(const ResLayout& P, const ResPacked& K, const float* params, const float* packed, const float* x, int B, ResWs& W, hipStream_t st) {
  if (P.center) ARDAE_TRY(launch_affine(x, (int64_t)B * 784, 2.f, -1.f, W.x2, st));       // do_center (ivae/resconv.py:131-132)
  else ARDAE_TRY(launch_affine(x, (int64_t)B * 784, 1.f, 0.f, W.x2, st));
  const float* cur = W.x2;
  for (size_t i = 0; i < 5; ++i) {
    ARDAE_TRY(blk_fwd(P.trunk[i], K.trunk[i], params, packed, cur, B, ACT_ELU, W.tb[i], st));
    cur = W.tb[i].out;
  }
  ARDAE_TRY(launch_nhwc_nchw(cur, B, 16, 32, W.flat, false, st));
  return blk_fwd(P.trunk[5], K.trunk[5], params, packed, W.flat, B, ACT_ELU, W.tb[5], st);
}

int res_decoder_fwd(const ResLayout& P, const ResPacked& K, const float* params, const float* packed, const float* z, int R, ResWs& W, float* logits,
                    hipStream_t st, bool fused_tail, const float* fused_mid_w) {
  ARDAE_TRY(blk_fwd(P.dec[0], K.dec[0], params, packed, z, R, ACT_ELU, W.db[0], st));
  ARDAE_TRY(blk_fwd(P.dec[1], K.dec[1], params, packed, W.db[0].out, R, ACT_ELU, W.db[1], st));
  ARDAE_TRY(launch_nhwc_nchw(W.db[1].out, R, 16, 32, W.d4, true, st));                                    // view(-1, 32, 4, 4) -> NHWC
  RES_LAUNCH(upsample2_fwd_kernel, (int64_t)R * 64 * 32, W.d4, 4, 32, W.u8, (int64_t)R * 64 * 32);
  ARDAE_TRY(blk_fwd(P.dec[2], K.dec[2], params, packed, W.u8, R, ACT_ELU, W.db[2], st));
  ARDAE_TRY(blk_fwd(P.dec[3], K.dec[3], params, packed, W.db[2].out, R, ACT_ELU, W.db[3], st));
  if (fused_mid_w) ARDAE_TRY(mid_fused(P, K, params, packed, fused_mid_w, W.db[3].out, R, W.db[5].out, st));
  else ARDAE_TRY(mid_unfused(P, K, params, packed, W.db[3].out, R, W.c7, W.u14, W.db[4], W.db[5], st));
  if (fused_tail) return tail_fused(P.dec[6], K.dec[6], params, packed, W.db[5].out, R, logits, st);
  RES_LAUNCH(upsample2_fwd_kernel, (int64_t)R * 784 * 16, W.db[5].out, 14, 16, W.u28, (int64_t)R * 784 * 16);
  ARDAE_TRY(blk_fwd(P.dec[6], K.dec[6], params, packed, W.u28, R, ACT_NONE, W.db[6], st));
  if (logits && logits != W.db[6].out) ARDAE_TRY(launch_copy(W.db[6].out, (size_t)R * 784, logits, st));
  return 0;
}

// ------------------------------------------------------------------------------------------------ backward pieces
int flush_wgrad(WgradList& wl, float* scratch, size_t scratch_floats, hipStream_t st) {
  while (wl.pending()) {
    const size_t n = std::min<size_t>(wl.pending(), ARDAE_WGRAD_MAX_PROBLEMS);
    Bump ws(scratch, scratch_floats);
    wl.assign(ws, (int)n, n);
    ARDAE_CHECK_ARG(ws.ok, "res model: weight-gradient scratch too small");
    ARDAE_TRY(wl.launch(st, n));
  }
  return 0;
}
size_t wgrad_scratch_floats(int M, int O, int I) {
  const int s = wgrad_splits(M, O, I, 3);
  const int s1 = wgrad_splits(M, O, I, 1), s20 = wgrad_splits(M, O, I, ARDAE_WGRAD_MAX_PROBLEMS);
  const int sm = std::max(s, std::max(s1, s20));
  return al64((size_t)sm * O * I) + al64((size_t)sm * 2 * O);
}

int blk_bwd(const Blk& b, const BlkPk& k, const float* packed, const float* x, int images, int act_out, const BlkBuf& u, const float* d_out, float* d_x,
            const BwdScratch& sc, const BlkGrad& gr, float* wscratch, size_t wscratch_floats, hipStream_t st) {
  const int R = (int)blk_rows(b, images);
  const int64_t nout = (int64_t)R * b.Cout;
  const float* g = d_out;
  if (act_out != ACT_NONE) {
    ARDAE_TRY(launch_mul_dact(d_out, u.out, act_out, sc.g, nout, st));
    g = sc.g;
  }
  const float* cx = b.conv ? u.colsx : x;
  const float* ch = b.conv ? u.colsh : u.hmid;
  // d hmid
  if (b.conv) {
    ARDAE_TRY(dense_fwd(ACT_NONE, R, b.h.I, g, b.Cout, b.Cout, packed + k.h.b, nullptr, sc.dcols, st));
    RES_LAUNCH(col2im3_kernel, nout, sc.dcols, b.Hout, b.Hout, b.Cout, b.Hout, b.Hout, 1, sc.dh, nout, (const float*)u.hmid, (int)ACT_ELU);
  } else {
    ARDAE_TRY(dense_bwd(ACT_RELU, R, b.Cout, g, b.Cout, packed + k.h.b, u.hmid, sc.dh, st));
  }
  // weight gradients of the three operators (their bias gradients: column sums of d hmid / g; b_h1 and b_01 share g's)
  WgradList wl(nullptr);
  wl.push(R, b.Cout, b.h.I, g, ch, b.h.I, gr.h.dW, b.h.I, gr.h.db);
  wl.push(R, b.Cout, b.s.I, g, cx, b.s.I, gr.s.dW, b.s.I, gr.s.db);
  wl.push(R, b.Cout, b.a.I, sc.dh, cx, b.a.I, gr.a.dW, b.a.I, gr.a.db);
  ARDAE_TRY(flush_wgrad(wl, wscratch, wscratch_floats, st));
  if (!d_x) return 0;
  // d x = W_01^T g + W_0h^T d hmid
  if (b.conv) {
    LinArgs A{}; A.Y = sc.dcols; A.ldY = b.a.I;
    ARDAE_TRY(lin2(EPI_ACT, ACT_NONE, R, b.a.I, g, b.Cout, b.Cout, packed + k.s.b, sc.dh, b.Cout, b.Cout, packed + k.a.b, A, st));
    const int64_t nin = (int64_t)images * b.Hin * b.Hin * b.Cin;
    RES_LAUNCH(col2im3_kernel, nin, sc.dcols, b.Hin, b.Hin, b.Cin, b.Hout, b.Hout, b.stride, d_x, nin, (const float*)nullptr, 0);
  } else {
    LinArgs A{}; A.Y = d_x; A.ldY = b.a.I;
    ARDAE_TRY(lin2(EPI_ACT, ACT_NONE, R, b.a.I, g, b.Cout, b.Cout, packed + k.s.b, sc.dh, b.Cout, b.Cout, packed + k.a.b, A, st));
  }
  return 0;
}

WnGrad GradMap::wn(const WN& w, const WNPk& k) {
  if (w.plain) return WnGrad{grads + w.dir, grads + w.bias, grads_beta};     // nn.Linear operator: the weight gradient IS the parameter gradient
  WnGrad g; g.dW = dweff + w.dir; g.db = dbias + boff; g.beta = 0.f; boff += al64(w.O);
  WnBwdItem it; it.dW = g.dW; it.dir = params + w.dir; it.scale = params + w.scale; it.inv = packed + k.inv; it.db = g.db;
  it.gdir = grads + w.dir; it.gscale = grads + w.scale; it.gbias = grads + w.bias; it.O = w.O; it.I = w.I; it.norm = w.norm ? 1 : 0;
  items.push_back(it);
  return g;
}
GradMap grad_map(ResWs& W, const float* params, const float* packed, float* grads, float grads_beta) {
  return GradMap{W.dweff, W.dbias, 0, {}, params, packed, grads, grads_beta};
}

int res_decoder_bwd(const ResLayout& P, const ResPacked& K, const float* packed, const float* z, ResWs& W, int R, GradMap& gm, hipStream_t st) {
  // ---- decoder backward (d_out ping-pongs between W.da and W.dbuf)
  std::vector<BlkGrad> gd(P.dec.size());
  for (size_t i = 0; i < P.dec.size(); ++i) gd[i] = gm.blk(P.dec[i], K.dec[i]);
  ARDAE_TRY(blk_bwd(P.dec[6], K.dec[6], packed, W.u28, R, ACT_NONE, W.db[6], W.dlogit, W.da, W.sc, gd[6], W.wscratch, W.wscratch_floats, st));      // -> d u28 [R,28,28,16]
  RES_LAUNCH(upsample2_bwd_kernel, (int64_t)R * 196 * 16, W.da, 14, 16, W.dbuf, (int64_t)R * 196 * 16);
  ARDAE_TRY(blk_bwd(P.dec[5], K.dec[5], packed, W.db[4].out, R, ACT_ELU, W.db[5], W.dbuf, W.da, W.sc, gd[5], W.wscratch, W.wscratch_floats, st));
  ARDAE_TRY(blk_bwd(P.dec[4], K.dec[4], packed, W.u14, R, ACT_ELU, W.db[4], W.da, W.dbuf, W.sc, gd[4], W.wscratch, W.wscratch_floats, st));          // -> d u14 [R,14,14,32]
  RES_LAUNCH(upsample2_bwd_kernel, (int64_t)R * 49 * 32, W.dbuf, 7, 32, W.da, (int64_t)R * 49 * 32);                                                 // -> d c7
  RES_LAUNCH(crop_pad_kernel, (int64_t)R * 64 * 32, W.da, 7, 8, 32, W.dbuf, (int64_t)R * 64 * 32);                                                    // -> d (block 3 out) [R,8,8,32]
  ARDAE_TRY(blk_bwd(P.dec[3], K.dec[3], packed, W.db[2].out, R, ACT_ELU, W.db[3], W.dbuf, W.da, W.sc, gd[3], W.wscratch, W.wscratch_floats, st));
  ARDAE_TRY(blk_bwd(P.dec[2], K.dec[2], packed, W.u8, R, ACT_ELU, W.db[2], W.da, W.dbuf, W.sc, gd[2], W.wscratch, W.wscratch_floats, st));            // -> d u8
  RES_LAUNCH(upsample2_bwd_kernel, (int64_t)R * 16 * 32, W.dbuf, 4, 32, W.da, (int64_t)R * 16 * 32);                                                 // -> d d4 (NHWC)
  ARDAE_TRY(launch_nhwc_nchw(W.da, R, 16, 32, W.dbuf, false, st));                                                                                    // -> NCHW-flat [R,512]
  ARDAE_TRY(blk_bwd(P.dec[1], K.dec[1], packed, W.db[0].out, R, ACT_ELU, W.db[1], W.dbuf, W.da, W.sc, gd[1], W.wscratch, W.wscratch_floats, st));
  ARDAE_TRY(blk_bwd(P.dec[0], K.dec[0], packed, z, R, ACT_ELU, W.db[0], W.da, W.dbuf, W.sc, gd[0], W.wscratch, W.wscratch_floats, st));               // -> dz (decoder part) [R,zd]
  ARDAE_TRY(launch_axpy(W.dbuf, (int64_t)R * P.zd, 1.f, W.dzq, st));                                                                                 // dz total in W.dzq
  return 0;
}

int res_trunk_wn_bwd(const ResLayout& P, const ResPacked& K, const float* packed, ResWs& W, int B, GradMap& gm, float grads_beta, hipStream_t st) {
  // ---- trunk backward
  std::vector<BlkGrad> gt(P.trunk.size());
  for (size_t i = 0; i < P.trunk.size(); ++i) gt[i] = gm.blk(P.trunk[i], K.trunk[i]);
  ARDAE_TRY(blk_bwd(P.trunk[5], K.trunk[5], packed, W.flat, B, ACT_ELU, W.tb[5], W.dinp, W.dflat, W.sc, gt[5], W.wscratch, W.wscratch_floats, st));
  ARDAE_TRY(launch_nhwc_nchw(W.dflat, B, 16, 32, W.da, true, st));                                  // NCHW-flat gradient -> NHWC [B,4,4,32]
  float *cur = W.da, *nxt = W.dbuf;
  for (int i = 4; i >= 0; --i) {
    const float* xin = i == 0 ? W.x2 : W.tb[i - 1].out;
    ARDAE_TRY(blk_bwd(P.trunk[i], K.trunk[i], packed, xin, B, ACT_ELU, W.tb[i], cur, i == 0 ? nullptr : nxt, W.sc, gt[i], W.wscratch, W.wscratch_floats, st));
    std::swap(cur, nxt);
  }
  // ---- dL/dW -> dL/d(direction, scale), bias gradients
  for (size_t i0 = 0; i0 < gm.items.size(); i0 += WNB_MAX) {
    WnBwdBatch bt;
    bt.n = (int)std::min<size_t>(WNB_MAX, gm.items.size() - i0);
    bt.beta = grads_beta;
    for (int i = 0; i < bt.n; ++i) bt.it[i] = gm.items[i0 + i];
    hipLaunchKernelGGL(wn_backward_kernel, dim3(32, bt.n), dim3(256), 0, st, bt);
    ARDAE_LAUNCH_CHECK();
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------ pack
int res_pack(const ResLayout& P, const ResPacked& K, const HeadBlks& head, PackList& pl, hipStream_t st) {
  const float* params = pl.params; float* packed = pl.packed;
  // what the panels are packed FROM: the weight-normalised operators' effective weights and every projected-skip block's bias sum,
  // composed into the packed buffer ahead of the pack launch
  std::vector<WnComposeItem> comp;
  auto wn = [&](const WN& w, const WNPk& k) {
    if (!w.plain) comp.push_back(WnComposeItem{params + w.dir, params + w.scale, packed + k.weff, packed + k.inv, w.O, w.I, w.norm ? 1 : 0, nullptr, nullptr});
  };
  auto blk = [&](const Blk& b, const BlkPk& k) {
    wn(b.a, k.a); wn(b.h, k.h);
    if (b.same) return;          // identity skip: no third operator, the block's bias is b_h1
    wn(b.s, k.s);
    comp.push_back(WnComposeItem{nullptr, nullptr, packed + k.bsum, nullptr, b.Cout, 0, 0, params + b.h.bias, params + b.s.bias});   // bsum = b_h + b_s
  };
  for (size_t i = 0; i < P.trunk.size(); ++i) blk(P.trunk[i], K.trunk[i]);
  for (auto& h : head) blk(*h.first, *h.second);
  for (size_t i = 0; i < P.dec.size(); ++i) blk(P.dec[i], K.dec[i]);
  for (size_t i0 = 0; i0 < comp.size(); i0 += WNC_MAX) {
    WnComposeBatch cb;
    cb.n = (int)std::min<size_t>(WNC_MAX, comp.size() - i0);
    int maxo = 1;
    for (int i = 0; i < cb.n; ++i) {
      cb.it[i] = comp[i0 + i];
      maxo = std::max(maxo, cb.it[i].dir ? cb.it[i].O : ceil_div(cb.it[i].O, 256));
    }
    hipLaunchKernelGGL(wn_compose_batch_kernel, dim3(maxo, cb.n), dim3(256), 0, st, cb);
    ARDAE_LAUNCH_CHECK();
  }
  return pl.launch(st);
}
int launch_mid_pack(const ResPacked& K, float* packed, size_t mid_w, hipStream_t st) {
  MidPackArgs a;
  const WNPk* ops[6] = {&K.dec[4].a, &K.dec[4].s, &K.dec[4].h, &K.dec[5].a, &K.dec[5].s, &K.dec[5].h};
  const int off[6] = {RM_W4A, RM_W4S, RM_W4H, RM_W5A, RM_W5S, RM_W5H};
  for (int i = 0; i < 6; ++i) { a.weff[i] = packed + ops[i]->weff; a.K[i] = i < 2 ? 288 : 144; a.off[i] = off[i]; }
  hipLaunchKernelGGL(resconv_mid_pack_kernel, dim3(nblk(RM_WTOTAL)), dim3(256), 0, st, a, packed + mid_w);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

// ================================================================================================ kinds 5 / 6: the implicit-posterior families
namespace {

// One operator of ResConvIPVAE's sampler head `encode.fc` (models/ivae/resconv.py:101-116) on the B nz rows: a ResLinear (inner ReLU) or a
// plain Linear, reading [trunk output | noise] (concat: the first one) or its predecessor's output, with ELU behind it or not
struct HeadOp { bool res; Blk b; Lin l; int in, out; bool concat; int act; };
// desc.flags bits 1-3 of kind 5: which head (ivae_ardae.py:323-442)
enum { HEAD_RES_WN_MLP = 0, HEAD_MLP = 1, HEAD_RES_MLP = 2, HEAD_RES_WN_MLP_LIN = 3, HEAD_RES_MLP_LIN = 4 };

struct IpResLayout : ResLayout {
  int kind;
  bool clipped;                  // kind 6 + ARDAE_MODEL_CLIPPED: MNISTResConvAuxIPVAEClipped (no 'spm4' clip, z0 keeps an unscaled eps0)
  std::vector<HeadOp> head;      // kind 5: encode.fc (the shipped recipe: ResLinear(cdim + nd -> hdim), ELU, ResLinear(hdim -> zd), un-normalised WN operators)
  Lin mu0{}, lv0{}, efc{}, mu{}, lv{};   // kind 6: aux_encode.reparam.{mean,logvar}_fn, encode.fc.0, encode.reparam.{mean,logvar}_fn
  explicit IpResLayout(const ardae_model_desc& d)
      : ResLayout(d, d.kind == 5 ? 512 : d.h_dim), kind(d.kind), clipped(d.kind == 6 && (d.flags & ARDAE_MODEL_CLIPPED)) {
    ResWalk w;
    trunk_blocks(w);
    if (kind == 5) {
      // encode.fc in the reference's parameter order (models/ivae/resconv.py:101-116, models/layers.py:477-515,559-622)
      const int ht = (d.flags >> 1) & 7, nl = d.n_layers, cin = cdim + nd;
      auto res_op = [&](int out, int in, bool plain, int act, bool concat) {
        HeadOp o; o.res = true; o.b = w.block(out, in, false, 1, 1, false, plain, in == out); o.in = in; o.out = out; o.concat = concat; o.act = act;
        o.l = Lin{0, 0, 0, 0};
        head.push_back(o);
      };
      auto lin_op = [&](int out, int in, int act, bool concat) {
        HeadOp o; o.res = false; o.l = w.lin(out, in); o.in = in; o.out = out; o.concat = concat; o.act = act; o.b = Blk{};
        head.push_back(o);
      };
      if (ht == HEAD_MLP) {                       // MLP(cin -> hdim x nl -> zd), ELU after the hidden layers
        for (int i = 0; i < nl; ++i) lin_op(hdim, i == 0 ? cin : hdim, ACT_ELU, i == 0);
        lin_op(zd, hdim, ACT_NONE, false);
      } else if (ht == HEAD_RES_WN_MLP || ht == HEAD_RES_MLP) {   // ResMLP(cin -> hdim x nl -> zd): ResLinear blocks, ELU between them
        const bool plain = ht == HEAD_RES_MLP;
        for (int i = 0; i < nl; ++i) res_op(hdim, i == 0 ? cin : hdim, plain, ACT_ELU, i == 0);
        res_op(zd, hdim, plain, ACT_NONE, false);
      } else {                                    // Sequential(ResMLP(cin -> hdim x (nl - 1) -> hdim, ELU on its output), Linear(hdim -> zd))
        const bool plain = ht == HEAD_RES_MLP_LIN;
        for (int i = 0; i < nl - 1; ++i) res_op(hdim, i == 0 ? cin : hdim, plain, ACT_ELU, i == 0);
        res_op(hdim, nl - 1 == 0 ? cin : hdim, plain, ACT_ELU, nl - 1 == 0);
        lin_op(zd, hdim, ACT_NONE, false);
      }
    } else {
      mu0 = w.lin(nd, cdim); lv0 = w.lin(nd, cdim); efc = w.lin(cdim, cdim + nd); mu = w.lin(zd, cdim); lv = w.lin(zd, cdim);
    }
    decoder_blocks(w);
    total = w.off;
  }
};

struct IpResPacked : ResPacked {
  struct HeadPk { BlkPk k; LinPk lk; };
  std::vector<HeadPk> head;
  LinPk mu0{}, lv0{}, efc{}, mu{}, lv{};
  IpResPacked(const IpResLayout& P, PackList& pl) {
    ResPackWalk w{pl};
    trunk_panels(P, w);
    if (P.kind == 5) {
      for (auto& o : P.head) {
        HeadPk hp{};
        if (o.res) hp.k = w.blk(o.b, o.concat ? P.cdim : 0); else hp.lk = w.lin(o.l, o.concat ? P.cdim : 0);
        head.push_back(hp);
      }
    } else { mu0 = w.lin(P.mu0, 0); lv0 = w.lin(P.lv0, 0); efc = w.lin(P.efc, P.cdim); mu = w.lin(P.mu, 0); lv = w.lin(P.lv, 0); }
    decoder_panels(P, w);
  }
  explicit IpResPacked(const IpResLayout& P, PackList&& sizing = PackList()) : IpResPacked(P, sizing) {}   // offsets only
};

// the descriptor rules of kinds 5 / 6
int res_desc_check(const ardae_model_desc* d) {
  ARDAE_TRY(desc_flags_ok(d, ARDAE_MODEL_NO_CENTER | ARDAE_MODEL_HEAD_MASK | ARDAE_MODEL_CLIPPED));
  ARDAE_CHECK_ARG(d->input_dim == 784 && d->noise_dim >= 1 && d->z_dim >= 1 && d->h_dim >= 1 && d->act == ACT_ELU && (d->kind == 6 || (d->n_layers >= 1 && d->n_layers <= 4)),
                  "model: the residual-conv models are 28x28x1, ELU, and (kind 5) 1 .. 4 hidden layers in the sampler head");
  const int ht = (d->flags >> 1) & 7;
  ARDAE_CHECK_ARG(d->kind != 5 || ht <= HEAD_RES_MLP_LIN, "model: unknown sampler head %d (desc.flags bits 1-3)", ht);
  ARDAE_CHECK_ARG(d->kind == 5 || ht == 0, "model: the sampler-head bits of desc.flags belong to kind 5");
  ARDAE_CHECK_ARG(d->kind == 6 || !(d->flags & ARDAE_MODEL_CLIPPED), "model: ARDAE_MODEL_CLIPPED belongs to kind 6");
  // a concat block needs its projected skip (same_dim would make the skip the 612-wide concat itself)
  ARDAE_CHECK_ARG(d->kind != 5 || ht == HEAD_MLP || 512 + d->noise_dim != d->h_dim,
                  "model: ResConvIPVAE with c_dim + noise_dim == h_dim (identity skip over the concat input) is not built");
  return 0;
}

// the sampler's rows (R = B*nz) beside the shared buffers
struct IpResWs : ResWs {
  float *zero;                                                      // zero noise for encode(std=0)
  struct HeadBuf { float *rba, *rbs, *hmid, *out; };                // kind 5, per head operator: per-image row biases [B,out] (concat), ResLinear hidden [R,out], output [R,out]
  std::vector<HeadBuf> hb; float* z;                                // z [R,zd]
  float *mu0, *lv0r, *lv0, *z0, *rbh, *hh, *mu, *lvr, *lv;          // kind 6
};

// mode 0: encode (trunk + sampler forward), 1: vae forward + backward, 2: decode only (B = rows, nz = 1)
void carve(const IpResLayout& P, const IpResPacked&, Bump& ws, int B, int nz, int mode, IpResWs& W) {
  const size_t R = (size_t)B * nz;
  if (mode != 2) {
    res_trunk_carve(P, ws, B, W);
    W.zero = ws.take(R * (P.nd + P.zd));
    if (P.kind == 5) {
      W.hb.resize(P.head.size());
      for (size_t i = 0; i < P.head.size(); ++i) {
        const HeadOp& o = P.head[i];
        W.hb[i].rba = o.concat ? ws.take((size_t)B * o.out) : nullptr;
        W.hb[i].rbs = (o.concat && o.res) ? ws.take((size_t)B * o.out) : nullptr;
        W.hb[i].hmid = o.res ? ws.take(R * o.out) : nullptr;
        W.hb[i].out = ws.take(R * o.out);
      }
      W.z = ws.take(R * P.zd);
    } else {
      W.mu0 = ws.take((size_t)B * P.nd); W.lv0r = ws.take((size_t)B * P.nd); W.lv0 = ws.take((size_t)B * P.nd); W.z0 = ws.take(R * P.nd);
      W.rbh = ws.take((size_t)B * P.cdim); W.hh = ws.take(R * P.cdim); W.mu = ws.take(R * P.zd); W.lvr = ws.take(R * P.zd); W.lv = ws.take(R * P.zd);
      W.z = ws.take(R * P.zd);
    }
  }
  if (mode != 0) res_decoder_carve(P, ws, R, DecRuns{true, true, true}, W);
  if (mode != 1) return;
  // the sampler tail's weight gradients: all problems of a head operator in one batch (kind 5); kind 6's nine in one list
  const int Ri = (int)R;
  size_t need = 2 * (wgrad_scratch_floats(Ri, P.hdim, P.hdim) + wgrad_scratch_floats(Ri, P.hdim, P.cdim + P.nd) + wgrad_scratch_floats(Ri, P.zd, P.hdim)) +
                3 * wgrad_scratch_floats(B, P.nd, P.cdim) + 2 * wgrad_scratch_floats(B, P.hdim, P.cdim);
  for (auto& o : P.head) {
    const int cin = o.concat ? P.nd : o.in;
    size_t op = 3 * wgrad_scratch_floats(Ri, o.out, std::max(cin, o.out));
    if (o.concat) op += 2 * wgrad_scratch_floats(B, o.out, P.cdim);
    need = max_sz(need, op);
  }
  res_bwd_carve(P, ws, B, R, need, W);
}

using ResEntry = Entry<IpResLayout, IpResPacked, IpResWs>;

// sampler tail on R = B*nz rows; noise [R, nd] (kind 5) or [R, nd + zd] rows [eps0 | eps] (kind 6); z -> z_out
// raw0 (clipped class, std = 0 pass only - `noise` is then the zero block): the unscaled eps0 [R, nd] z0 keeps, or NULL (zeros)
int sampler_fwd(const IpResLayout& P, const IpResPacked& K, const float* params, const float* packed, const float* noise, int B, int nz, IpResWs& W,
                float* z_out, float* hidden_out, hipStream_t st, const float* raw0 = nullptr, bool std0 = false) {
  const int R = B * nz;
  if (P.kind == 5) {
    // encode.fc operator by operator; the per-image half of a concat input enters as a row bias (computed once per image)
    const float* x = nullptr;
    for (size_t i = 0; i < P.head.size(); ++i) {
      const HeadOp& o = P.head[i];
      const IpResPacked::HeadPk& hk = K.head[i];
      IpResWs::HeadBuf& u = W.hb[i];
      float* out = i + 1 == P.head.size() ? z_out : u.out;
      if (o.res) {
        const Blk& b = o.b; const BlkPk& k = hk.k;
        if (o.concat) {
          // rba = W0h[:, :c] inp + b0h, rbs = W01[:, :c] inp + (bh1 + b01)
          ARDAE_TRY(dense_fwd(ACT_NONE, B, o.out, W.inp, P.cdim, P.cdim, packed + k.a_fi, params + b.a.bias, u.rba, st));
          ARDAE_TRY(dense_fwd(ACT_NONE, B, o.out, W.inp, P.cdim, P.cdim, packed + k.s_fi, packed + k.bsum, u.rbs, st));
          { LinArgs A{}; A.rowbias = u.rba; A.rowbias_ld = o.out; A.rows_per_group = nz; A.Y = u.hmid; A.ldY = o.out;
            ARDAE_TRY(lin1(EPI_ACT, ACT_RELU, R, o.out, noise, P.nd, P.nd, packed + k.a_fn, A, st)); }
          { LinArgs A{}; A.rowbias = u.rbs; A.rowbias_ld = o.out; A.rows_per_group = nz; A.Y = out; A.ldY = o.out;
            ARDAE_TRY(lin2(EPI_ACT, ACT_NONE, R, o.out, u.hmid, o.out, o.out, packed + k.h.f, noise, P.nd, P.nd, packed + k.s_fn, A, st)); }
        } else {
          ARDAE_TRY(dense_fwd(ACT_RELU, R, o.out, x, o.in, o.in, packed + k.a.f, params + b.a.bias, u.hmid, st));
          if (!b.same) {
            LinArgs A{}; A.bias = packed + k.bsum; A.Y = out; A.ldY = o.out;
            ARDAE_TRY(lin2(EPI_ACT, ACT_NONE, R, o.out, u.hmid, o.out, o.out, packed + k.h.f, x, o.in, o.in, packed + k.s.f, A, st));
          } else {   // identity skip (ResLinear(same_dim=True), models/layers.py:82-84)
            ARDAE_TRY(dense_fwd(ACT_NONE, R, o.out, u.hmid, o.out, o.out, packed + k.h.f, params + b.h.bias, out, st));
            ARDAE_TRY(launch_axpy(x, (int64_t)R * o.out, 1.f, out, st));
          }
        }
      } else {
        const Lin& l = o.l; const LinPk& k = hk.lk;
        if (o.concat) {
          ARDAE_TRY(cat_fwd(ACT_NONE, B, nz, o.out, W.inp, P.cdim, packed + k.fi, params + l.b, noise, P.nd, packed + k.fn, u.rba, out, st));
        } else {
          ARDAE_TRY(dense_fwd(ACT_NONE, R, o.out, x, o.in, o.in, packed + k.f, params + l.b, out, st));
        }
      }
      if (o.act != ACT_NONE) RES_LAUNCH(act_inplace_kernel, (int64_t)R * o.out, out, o.act, (int64_t)R * o.out);
      x = out;
    }
    return 0;
  }
  const int ldn = P.nd + P.zd;
  ARDAE_TRY(dense_fwd(ACT_NONE, B, P.nd, W.inp, P.cdim, P.cdim, packed + K.mu0.f, params + P.mu0.b, W.mu0, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, B, P.nd, W.inp, P.cdim, P.cdim, packed + K.lv0.f, params + P.lv0.b, W.lv0r, st));
  RES_LAUNCH(spm4_kernel, (int64_t)B * P.nd, W.lv0r, (const float*)nullptr, W.lv0, (int64_t)B * P.nd, (int)P.clipped);
  // clipped: z0 = mu0 + (std exp(lv0 / 2) + 1) eps0; the std = 0 pass (noise = zeros) takes its unscaled draw from raw0 (none: z0 = mu0)
  if (P.clipped && !(std0 && !raw0)) ARDAE_TRY(launch_reparam_fwd(W.mu0, W.lv0, noise, ldn, R, P.nd, nz, W.z0, st, 1.f, std0 ? raw0 : nullptr, P.nd));
  else ARDAE_TRY(launch_reparam_fwd(W.mu0, W.lv0, noise, ldn, R, P.nd, nz, W.z0, st));
  ARDAE_TRY(cat_fwd(ACT_NONE, B, nz, P.cdim, W.inp, P.cdim, packed + K.efc.fi, params + P.efc.b, W.z0, P.nd, packed + K.efc.fn, W.rbh, W.hh, st));
  RES_LAUNCH(act_inplace_kernel, (int64_t)R * P.cdim, W.hh, (int)ACT_ELU, (int64_t)R * P.cdim);
  if (hidden_out) ARDAE_TRY(launch_copy(W.hh, (size_t)R * P.cdim, hidden_out, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, R, P.zd, W.hh, P.cdim, P.cdim, packed + K.mu.f, params + P.mu.b, W.mu, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, R, P.zd, W.hh, P.cdim, P.cdim, packed + K.lv.f, params + P.lv.b, W.lvr, st));
  RES_LAUNCH(spm4_kernel, (int64_t)R * P.zd, W.lvr, (const float*)nullptr, W.lv, (int64_t)R * P.zd, (int)P.clipped);
  return launch_reparam_fwd(W.mu, W.lv, noise + P.nd, ldn, R, P.zd, 1, z_out, st);
}

// ardae_model_pack: the head's ResLinear blocks are composed with the trunk's and the decoder's
int ipres_pack(const ardae_model_desc& d, const float* params, float* packed, hipStream_t st) {
  const IpResLayout P(d);
  PackList pl(params, packed);
  const IpResPacked K(P, pl);
  HeadBlks head;
  for (size_t i = 0; i < P.head.size(); ++i)
    if (P.head[i].res) head.push_back({&P.head[i].b, &K.head[i].k});
  return res_pack(P, K, head, pl, st);
}

// What the shared algorithm (csrc/ipmodel.h) needs to know of the residual-conv models (the weight gradients go out block by block through
// flush_wgrad, their scratch carved up front: there is no list to size)
struct ResTraits : IpTraitsBase {
  using Layout = IpResLayout; using Packed = IpResPacked; using Ws = IpResWs; using Entry = ResEntry;
  using Grads = GradMap;      // built before the decoder's backward, used again by the sampler's and the trunk's
  [[maybe_unused]] static constexpr bool direct_z = true;      // a forward-only encode: the last launch of the sampler writes the caller's buffer itself
  static int desc_check(const ardae_model_desc* d) { return res_desc_check(d); }
  // the hidden1a context is the aux model's h; the raw form belongs to its clipped class
  static unsigned caps(const ardae_model_desc& d) { return d.kind != 6 ? 0 : (d.flags & ARDAE_MODEL_CLIPPED) ? CAP_HIDDEN | CAP_HIDDEN_RAW : CAP_HIDDEN; }
  static IpBufs bufs(const IpResWs& W) {      // the decoder's backward adds its dz to what the loss kernel left in dzq
    return {W.z, W.db[6].out, nullptr, W.dlogit, nullptr, W.dzq, W.dzq, W.rec_row, W.pri_row};
  }
  static void wgrads(const IpResLayout&, const IpResPacked&, const IpResWs&, const float*, const float*, int, int, WgradList&, Bump&) {}
  static size_t noise_floats(const IpResLayout& P, int B, int nz) { return (size_t)B * nz * (P.nd + P.zd); }
  static float* zero_noise(Entry& e, size_t) { return e.W.zero; }
  // (a forward-only pass copies the hidden context out in passing)
  static int sampler_fwd(Entry& e, const float* params, const float* packed, const float* x, const float* noise, int B, int nz, const IpEncodeOut* enc,
                         hipStream_t st) {
    auto& [P, K, ws, W] = e;
    ARDAE_TRY(res_trunk_fwd(P, K, params, packed, x, B, W, st));
    if (!enc) return ardae::sampler_fwd(P, K, params, packed, noise, B, nz, W, W.z, nullptr, st);
    ARDAE_CHECK_ARG(!enc->raw0 || (P.clipped && enc->std0), "res model: raw0 is the clipped class's unscaled eps0 of a std = 0 pass (noise NULL)");
    return ardae::sampler_fwd(P, K, params, packed, noise, B, nz, W, enc->z_out ? enc->z_out : W.z, enc->hidden_out, st, enc->raw0, enc->std0);
  }
  static int decoder_fwd(Entry& e, const float* params, const float* packed, const float* z, int R, hipStream_t st) {
    return res_decoder_fwd(e.P, e.K, params, packed, z, R, e.W, nullptr, st);
  }
  static GradMap grads_of(Entry& e, const float* params, const float* packed, float* g, float beta) { return grad_map(e.W, params, packed, g, beta); }
  static int decoder_bwd(Entry& e, const float* packed, int R, GradMap& gm, hipStream_t st) { return res_decoder_bwd(e.P, e.K, packed, e.W.z, e.W, R, gm, st); }
  // the sampler's backward -> W.dinp [B, cdim], then the trunk's
  static int sampler_bwd(Entry& e, const float*, const float* packed, const float*, const float* noise, int B, int nz, GradMap& gm, hipStream_t st) {
    ARDAE_TRY(e.P.kind == 5 ? head_bwd(e, packed, noise, B, nz, gm, st) : aux_bwd(e, packed, noise, B, nz, gm, st));
    return res_trunk_wn_bwd(e.P, e.K, packed, e.W, B, gm, gm.grads_beta, st);
  }
  // kind 5: encode.fc backwards, operator by operator: g = dL/d(output of the operator) [R, out]
  static int head_bwd(Entry& e, const float* packed, const float* noise, int B, int nz, GradMap& gm, hipStream_t st) {
    auto& [P, K, ws, W] = e;
    const int R = B * nz;
    WgradList wl(gm.grads);              // plain nn.Linear gradients are written in place by the wgrad kernel (no weight norm)
    auto pw = [&](int M, int O, int I, const float* G, const float* X, int ldX, const WnGrad& g, int col0, int ldout, bool bias) {
      wl.push(M, O, I, G, X, ldX, g.dW + col0, ldout, bias ? g.db : nullptr).beta = g.beta;
    };
    float* g = W.dzq;
    float* pp[2] = {W.dR0, W.dR1};
    for (int i = (int)P.head.size() - 1; i >= 0; --i) {
      const HeadOp& o = P.head[i];
      const IpResPacked::HeadPk& hk = K.head[i];
      const IpResWs::HeadBuf& u = W.hb[i];
      const float* out = i + 1 == (int)P.head.size() ? W.z : u.out;
      const float* x = i == 0 ? nullptr : W.hb[i - 1].out;        // the operator's input (post-activation output of its predecessor)
      float* dx = pp[i & 1];
      if (o.act != ACT_NONE) ARDAE_TRY(launch_mul_dact(g, out, o.act, g, (int64_t)R * o.out, st));
      if (o.res) {
        const Blk& b = o.b; const BlkPk& k = hk.k;
        const BlkGrad gr = gm.blk(b, k);
        float* dh = W.sc.dh;       // [R, out]: d hmid = (g W_h1) relu'(hmid)
        ARDAE_TRY(dense_bwd(ACT_RELU, R, o.out, g, o.out, packed + k.h.b, u.hmid, dh, st));
        pw(R, o.out, o.out, g, u.hmid, o.out, gr.h, 0, o.out, true);
        if (o.concat) {
          const int I0 = P.cdim + P.nd;
          ARDAE_TRY(launch_segment_sum(g, o.out, B, nz, o.out, 1.f, W.dB0, o.out, st));       // d rbs [B, out]
          ARDAE_TRY(launch_segment_sum(dh, o.out, B, nz, o.out, 1.f, W.dB1, o.out, st));      // d rba [B, out]
          pw(R, o.out, P.nd, g, noise, P.nd, gr.s, P.cdim, I0, true);                           // noise columns of W_01 (+ its bias)
          pw(B, o.out, P.cdim, W.dB0, W.inp, P.cdim, gr.s, 0, I0, false);                       // image columns of W_01
          pw(R, o.out, P.nd, dh, noise, P.nd, gr.a, P.cdim, I0, true);
          pw(B, o.out, P.cdim, W.dB1, W.inp, P.cdim, gr.a, 0, I0, false);
          ARDAE_TRY(flush_wgrad(wl, W.wscratch, W.wscratch_floats, st));
          LinArgs A{}; A.Y = W.dinp; A.ldY = P.cdim;
          ARDAE_TRY(lin2(EPI_ACT, ACT_NONE, B, P.cdim, W.dB0, o.out, o.out, packed + k.s_bi, W.dB1, o.out, o.out, packed + k.a_bi, A, st));
        } else {
          if (!b.same) pw(R, o.out, o.in, g, x, o.in, gr.s, 0, o.in, true);
          pw(R, o.out, o.in, dh, x, o.in, gr.a, 0, o.in, true);
          ARDAE_TRY(flush_wgrad(wl, W.wscratch, W.wscratch_floats, st));
          if (!b.same) {
            LinArgs A{}; A.Y = dx; A.ldY = o.in;
            ARDAE_TRY(lin2(EPI_ACT, ACT_NONE, R, o.in, g, o.out, o.out, packed + k.s.b, dh, o.out, o.out, packed + k.a.b, A, st));
          } else {   // identity skip: dx = dh W_0h + g
            ARDAE_TRY(dense_fwd(ACT_NONE, R, o.in, dh, o.out, o.out, packed + k.a.b, nullptr, dx, st));
            ARDAE_TRY(launch_axpy(g, (int64_t)R * o.in, 1.f, dx, st));
          }
        }
      } else {
        const Lin& l = o.l; const LinPk& k = hk.lk;
        const WnGrad gl{gm.grads + l.w, gm.grads + l.b, gm.grads_beta};
        if (o.concat) {
          ARDAE_TRY(launch_segment_sum(g, o.out, B, nz, o.out, 1.f, W.dB0, o.out, st));       // d rba [B, out]
          pw(R, o.out, P.nd, g, noise, P.nd, gl, P.cdim, l.in, true);
          pw(B, o.out, P.cdim, W.dB0, W.inp, P.cdim, gl, 0, l.in, false);
          ARDAE_TRY(flush_wgrad(wl, W.wscratch, W.wscratch_floats, st));
          ARDAE_TRY(dense_fwd(ACT_NONE, B, P.cdim, W.dB0, o.out, o.out, packed + k.bi, nullptr, W.dinp, st));
        } else {
          pw(R, o.out, o.in, g, x, o.in, gl, 0, l.in, true);
          ARDAE_TRY(flush_wgrad(wl, W.wscratch, W.wscratch_floats, st));
          ARDAE_TRY(dense_fwd(ACT_NONE, R, o.in, g, o.out, o.out, packed + k.b, nullptr, dx, st));
        }
      }
      g = dx;
    }
    return 0;
  }
  // kind 6: the two reparameterisations and their heads backwards
  static int aux_bwd(Entry& e, const float* packed, const float* noise, int B, int nz, GradMap& gm, hipStream_t st) {
    auto& [P, K, ws, W] = e;
    const int R = B * nz, ldn = P.nd + P.zd;
    WgradList wl(gm.grads);              // plain nn.Linear gradients are written in place by the wgrad kernel (no weight norm)
    auto plain_wgrad = [&](int M, const Lin& l, const float* G, const float* X, int ldX, int col0, int I, bool bias) {
      wl.push(M, l.out, I, G, X, ldX, gm.grads + l.w + col0, l.in, bias ? gm.grads + l.b : nullptr).beta = gm.grads_beta;
    };
    // z = mu + exp(lv/2) eps,  lv = spm4(lvr)
    float* dlv = W.sc.g;           // [R, zd]
    ARDAE_TRY(launch_reparam_bwd(W.dzq, W.z, W.mu, R, P.zd, 1, dlv, st));
    RES_LAUNCH(spm4_kernel, (int64_t)R * P.zd, W.lvr, (const float*)dlv, dlv, (int64_t)R * P.zd, (int)P.clipped);
    plain_wgrad(R, P.mu, W.dzq, W.hh, P.cdim, 0, P.cdim, true);
    plain_wgrad(R, P.lv, dlv, W.hh, P.cdim, 0, P.cdim, true);
    float* dhh = W.dR0;            // [R, cdim]
    { LinArgs A{}; A.Y = dhh; A.ldY = P.cdim; ARDAE_TRY(lin2(EPI_ACT, ACT_NONE, R, P.cdim, W.dzq, P.zd, P.zd, packed + K.mu.b, dlv, P.zd, P.zd, packed + K.lv.b, A, st)); }
    ARDAE_TRY(launch_mul_dact(dhh, W.hh, ACT_ELU, dhh, (int64_t)R * P.cdim, st));
    ARDAE_TRY(launch_segment_sum(dhh, P.cdim, B, nz, P.cdim, 1.f, W.dB0, P.cdim, st));      // d rbh [B, cdim]
    plain_wgrad(R, P.efc, dhh, W.z0, P.nd, P.cdim, P.nd, true);                              // z0 columns + bias
    plain_wgrad(B, P.efc, W.dB0, W.inp, P.cdim, 0, P.cdim, false);                           // image columns
    float* dz0 = W.dR1;            // [R, nd] = dhh W_fc[:, cdim:]
    ARDAE_TRY(dense_fwd(ACT_NONE, R, P.nd, dhh, P.cdim, P.cdim, packed + K.efc.bn, nullptr, dz0, st));
    // z0 = mu0[b] + exp(lv0[b] / 2) eps0,  lv0 = spm4(lv0r): reduce over the nz rows of an image first
    float* dlv0_rows = W.sc.dh;    // [R, nd]
    ARDAE_TRY(launch_reparam_bwd(dz0, W.z0, W.mu0, R, P.nd, nz, dlv0_rows, st, P.clipped ? 1.f : 0.f, noise, ldn));
    ARDAE_TRY(launch_segment_sum(dz0, P.nd, B, nz, P.nd, 1.f, W.dB1, P.nd, st));            // d mu0 [B, nd]
    ARDAE_TRY(launch_segment_sum(dlv0_rows, P.nd, B, nz, P.nd, 1.f, W.dB2, P.nd, st));      // d lv0 [B, nd]
    RES_LAUNCH(spm4_kernel, (int64_t)B * P.nd, W.lv0r, (const float*)W.dB2, W.dB2, (int64_t)B * P.nd, (int)P.clipped);
    plain_wgrad(B, P.mu0, W.dB1, W.inp, P.cdim, 0, P.cdim, true);
    plain_wgrad(B, P.lv0, W.dB2, W.inp, P.cdim, 0, P.cdim, true);
    ARDAE_TRY(flush_wgrad(wl, W.wscratch, W.wscratch_floats, st));
    // d inp = d rbh W_fc[:, :cdim] + d mu0 W_mu0 + d lv0r W_lv0
    float* part = W.dflat;         // [B, cdim] scratch (cdim <= 512)
    { LinArgs A{}; A.Y = part; A.ldY = P.cdim;
      ARDAE_TRY(lin2(EPI_ACT, ACT_NONE, B, P.cdim, W.dB0, P.cdim, P.cdim, packed + K.efc.bi, W.dB1, P.nd, P.nd, packed + K.mu0.b, A, st)); }
    return dense_bwd(ACT_NONE, B, P.cdim, W.dB2, P.nd, packed + K.lv0.b, part, W.dinp, st, part);       // V * 1 + Q
  }
};

}  // namespace

// (host pass only: a const object with a constant initialiser is otherwise emitted for the device too, where no entry point exists)
#ifndef __HIP_DEVICE_COMPILE__
const Family RES_FAMILY = ip_family<ResTraits>(ipres_pack);
#endif

}  // namespace ardae

using namespace ardae;

// ================================================================================================ ardae_resconv_tail / ardae_resconv_mid
// what the unfused launches keep, carved once for the call and for its *_workspace_floats: u28 and dec[6]'s columns, hidden map and output ...
struct TailBufs { float* u28; BlkBuf u; };
static TailBufs tail_carve(const ResLayout& P, int R, Bump& ws) {
  TailBufs t{ws.take((size_t)R * 784 * 16), {}};
  blk_carve(P.dec[6], R, ws, t.u);
  return t;
}
// ... c7, u14 and the columns, hidden maps and outputs of dec[4] / dec[5]
struct MidBufs { float *c7, *u14; BlkBuf u4, u5; };
static MidBufs mid_carve(const ResLayout& P, int R, Bump& ws) {
  MidBufs m{ws.take((size_t)R * 49 * 32), ws.take((size_t)R * 196 * 32), {}, {}};
  blk_carve(P.dec[4], R, ws, m.u4); blk_carve(P.dec[5], R, ws, m.u5);
  return m;
}
// the decoder's blocks of the two kinds ardae_resconv_tail takes (their descriptor rules: the Family row's)
static ResDecoderView decoder_view(const ardae_model_desc* d) { return d->kind == 19 ? auxresvae_decoder_view(*d) : resvae_decoder_view(*d); }

extern "C" {

size_t ardae_resconv_tail_workspace_floats(const ardae_model_desc* d, int R, int variant) {
  if (!d || (d->kind != 12 && d->kind != 19) || family(d).desc_check(d) || R <= 0 || R >= (1 << 20) || variant < 0 || variant > 2) return 0;
  if (variant == 1 || (variant == 0 && tail_fused_default())) return 0;
  Bump ws;
  tail_carve(decoder_view(d).P, R, ws);
  return ws.off;
}

int ardae_resconv_tail(const ardae_model_desc* d, const float* params, const float* packed, const float* y14, int R, int variant, float* workspace,
                       size_t workspace_floats, float* logits, void* stream) {
  ARDAE_CHECK_ARG(d != nullptr, "resconv_tail: desc is NULL");
  ARDAE_CHECK_ARG(d->kind == 12 || d->kind == 19, "resconv_tail: kind must be 12 (MNISTResConvVAE) or 19 (MNISTResConvAuxVAE), got %d", d->kind);
  ARDAE_TRY(family(d).desc_check(d));
  ARDAE_CHECK_ARG(variant >= 0 && variant <= 2, "resconv_tail: variant must be 0 (the library's choice), 1 (fused) or 2 (unfused), got %d", variant);
  ARDAE_CHECK_ARG(params && packed && y14 && logits, "resconv_tail: null pointer argument");
  ARDAE_CHECK_ARG(R > 0 && R < (1 << 20), "resconv_tail: bad batch (R=%d)", R);
  if (variant == 0) variant = tail_fused_default() ? 1 : 2;
  hipStream_t st = (hipStream_t)stream;
  const auto [P, K, mid_w] = decoder_view(d);
  if (variant == 1) return tail_fused(P.dec[6], K.dec[6], params, packed, y14, R, logits, st);
  const size_t need = ardae_resconv_tail_workspace_floats(d, R, 2);
  ARDAE_CHECK_ARG(workspace, "resconv_tail: null pointer argument (the unfused launches need a workspace)");
  ARDAE_CHECK_ARG(workspace_floats >= need, "resconv_tail: workspace too small (%zu < %zu floats)", workspace_floats, need);
  Bump ws(workspace, workspace_floats);
  TailBufs t = tail_carve(P, R, ws);
  RES_LAUNCH(upsample2_fwd_kernel, (int64_t)R * 784 * 16, y14, 14, 16, t.u28, (int64_t)R * 784 * 16);
  ARDAE_TRY(blk_fwd(P.dec[6], K.dec[6], params, packed, t.u28, R, ACT_NONE, t.u, st));
  return launch_copy(t.u.out, (size_t)R * 784, logits, st);
}

size_t ardae_resconv_mid_workspace_floats(const ardae_model_desc* d, int R, int variant) {
  if (!d || d->kind != 19 || family(d).desc_check(d) || R <= 0 || R >= (1 << 20) || variant < 0 || variant > 2) return 0;
  if (variant == 1 || (variant == 0 && mid_fused_default())) return 0;
  Bump ws;
  mid_carve(auxresvae_decoder_view(*d).P, R, ws);
  return ws.off;
}

int ardae_resconv_mid(const ardae_model_desc* d, const float* params, const float* packed, const float* y8, int R, int variant, float* workspace,
                      size_t workspace_floats, float* y14, void* stream) {
  ARDAE_CHECK_ARG(d != nullptr, "resconv_mid: desc is NULL");
  ARDAE_CHECK_ARG(d->kind == 19, "resconv_mid: kind must be 19 (MNISTResConvAuxVAE), got %d", d->kind);
  ARDAE_TRY(family(d).desc_check(d));
  ARDAE_CHECK_ARG(variant >= 0 && variant <= 2, "resconv_mid: variant must be 0 (the library's choice), 1 (fused) or 2 (unfused), got %d", variant);
  ARDAE_CHECK_ARG(params && packed && y8 && y14, "resconv_mid: null pointer argument");
  ARDAE_CHECK_ARG(R > 0 && R < (1 << 20), "resconv_mid: bad batch (R=%d)", R);
  if (variant == 0) variant = mid_fused_default() ? 1 : 2;
  hipStream_t st = (hipStream_t)stream;
  const auto [P, K, mid_w] = auxresvae_decoder_view(*d);
  if (variant == 1) return mid_fused(P, K, params, packed, packed + mid_w, y8, R, y14, st);
  const size_t need = ardae_resconv_mid_workspace_floats(d, R, 2);
  ARDAE_CHECK_ARG(workspace, "resconv_mid: null pointer argument (the unfused launches need a workspace)");
  ARDAE_CHECK_ARG(workspace_floats >= need, "resconv_mid: workspace too small (%zu < %zu floats)", workspace_floats, need);
  Bump ws(workspace, workspace_floats);
  MidBufs m = mid_carve(P, R, ws);
  ARDAE_TRY(mid_unfused(P, K, params, packed, y8, R, m.c7, m.u14, m.u4, m.u5, st));
  return launch_copy(m.u5.out, (size_t)R * 196 * 16, y14, st);
}

}  // extern "C"

