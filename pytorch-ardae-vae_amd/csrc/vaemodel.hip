// Gaussian-posterior VAE baselines (vae.py; ardae_model_desc.kind 8: models/vae/mnist.py::VAE, 9: models/vae/toy.py::VAE), orchestrated
// from the K1 / K6w kernels like csrc/model.hip, plus the one kernel the family adds: the fused Gaussian head.  Also here, for every Gaussian kind
// (11: csrc/convvae.hip, 12: csrc/resvae.hip): the head's kernels and its one policy (gauss_head_fwd), and the ardae_vae_* entry points, which
// validate and dispatch through the table's row (family(d).gauss); the algorithm they run is csrc/vaemodel.h's, over each family's traits.
//
//   per image (B rows):  xs = 2x - 1 (kind 8) | x (kind 9);  h = MLP_enc(xs)  (n_layers Linear -> act: layers.0 .. n-2, fc)
//                        mu = M h + m;  lv = L h + l;  z = mu + exp(lv / 2) eps;  kld = -0.5 sum_c (1 + lv - mu^2 - exp(lv))   (utils/vae.py:78-92)
//                        decoder: n_layers Linear -> act from z, then logit_fn (kind 8) | mean_fn, logvar_fn (kind 9); row reconstruction loss
//   losses = {mean_b(recon_b + beta kld_b), mean recon, mean kld}    (VAE.forward, vae/mnist.py:131-162, vae/toy.py:122-152)
// Backward (c = loss_scale / B; the reparameterisation in closed form):  dz = the decoder's;  dmu = dz + c beta mu;
//   dlv = dz (z - mu) / 2 + c beta (exp(lv) - 1) / 2;  both heads back into h, the encoder stack, every weight gradient in one batch.
//
// gauss_head_kernel: the head as ONE launch over 8-row tiles - the two [z, h] products (FP32 FMAs, each output element's products summed
// over ascending k from a zero accumulator, the bias added after: DESIGN 0 item 1, so a row's bits do not depend on B), the draw
// (Philox keyed like ardae_philox_normal_at) or the injected eps, the reparameterisation and the row's KL (its terms in double, summed
// over ascending c by one thread).  The unfused form of the same head is five launches (two narrow linears, the draw, the
// reparameterisation, the KL rows) and stays callable: ardae_vae_head's `variant`, or ARDAE_VAE_HEAD_UNFUSED=1 under ARDAE_DEBUG_KNOBS=1.
#include <cmath>

#include <vector>

#include "ardae_hip.h"
#include "auxmodel.h"
#include "common.h"
#include "elementwise.h"
#include "mlp.h"
#include "philox.h"
#include "vaemodel.h"

namespace ardae {
namespace {

struct VaeLayout {
  int kind, D, h, zd, nl, act;
  bool toy;                        // kind 9: no 2x - 1 rescale, Gaussian decoder
  std::vector<Lin> enc, dec;       // encode.main / decode.main: nl Linear each (nl - 1 `layers` + `fc`, all followed by act)
  Lin mean, logvar, heads[2];      // encode.reparam.{mean_fn, logvar_fn}; decode.reparam.logit_fn | {mean_fn, logvar_fn}
  size_t total = 0;
  explicit VaeLayout(const ardae_model_desc& d) : kind(d.kind), D(d.input_dim), h(d.h_dim), zd(d.z_dim), nl(d.n_layers), act(d.act), toy(d.kind == 9) {
    size_t off = 0;
    auto one = [&](int out, int in) { return next_lin(off, out, in); };
    for (int l = 0; l < nl; ++l) enc.push_back(one(h, l == 0 ? D : h));
    mean = one(zd, h); logvar = one(zd, h);
    for (int l = 0; l < nl; ++l) dec.push_back(one(h, l == 0 ? zd : h));
    heads[0] = one(D, h);
    if (toy) heads[1] = one(D, h);
    total = off;
  }
};

struct VaePacked {
  MlpStack enc;
  size_t mean_f, mean_b, logvar_f, logvar_b;
  MlpDecoder dec;
  VaePacked(const VaeLayout& P, PackList& pl) : enc(P.enc.data(), P.nl, pl) {
    pl.pair(P.mean, mean_f, mean_b); pl.pair(P.logvar, logvar_f, logvar_b);
    dec = MlpDecoder(P.dec.data(), P.nl, P.heads, P.toy ? 2 : 1, pl);
  }
  explicit VaePacked(const VaeLayout& P, PackList&& sizing = PackList()) : VaePacked(P, sizing) {}   // offsets only
};

struct VaeWs {
  float *xs, *mu, *lv;                  // mode 0 (encode_stats) ends here
  std::vector<float*> e, de;            // e[l] / de[l] [B, h], l = 1 .. nl
  float *z, *eps, *kld;                 // [B, zd] x 2, [B]
  MlpDecoder::Bufs D;
  float *rec_row, *pri_row;             // pri_row: launch_vae_loss' N(0, I) energy rows, which this family does not use
  float *dmu, *dlv;
};

// mode 0: the encoder up to (mu, lv); 1: + sample, decoder, losses, backward
void carve(const VaeLayout& P, const VaePacked& K, Bump& ws, int B, int mode, VaeWs& W) {
  const size_t b = (size_t)B;
  W.xs = P.toy ? nullptr : ws.take(b * P.D);
  K.enc.carve(ws, b, W.e);
  W.mu = ws.take(b * P.zd); W.lv = ws.take(b * P.zd);
  if (mode == 0) return;
  W.z = ws.take(b * P.zd); W.eps = ws.take(b * P.zd); W.kld = ws.take(b);
  K.dec.carve(ws, b, true, W.D);
  W.rec_row = ws.take(b); W.pri_row = ws.take(b);
  W.dmu = ws.take(b * P.zd); W.dlv = ws.take(b * P.zd);
  K.enc.carve(ws, b, W.de);
}
using VaeEntry = Entry<VaeLayout, VaePacked, VaeWs>;

// every weight-gradient problem of the backward: decoder (heads, layers), the two Gaussian heads, the encoder stack
void vae_wgrads(const VaeLayout& P, const VaePacked& K, const VaeWs& W, const float* x, int B, WgradList& wl, Bump& ws) {
  K.dec.wgrads(wl, B, W.z, W.D);
  wl.push(B, P.zd, P.h, W.dmu, W.e[P.nl], P.h, wl.g(P.mean.w), P.h, wl.g(P.mean.b));
  wl.push(B, P.zd, P.h, W.dlv, W.e[P.nl], P.h, wl.g(P.logvar.w), P.h, wl.g(P.logvar.b));
  K.enc.wgrads(wl, B, P.toy ? x : W.xs, W.e.data(), W.de.data());
  wl.assign(ws, (P.toy ? 2 : 1) + P.nl + 2 + P.nl);
}

size_t workspace_floats(const VaeLayout& P, int B, int mode) {
  const VaePacked K(P);
  Bump ws;
  VaeWs W;
  carve(P, K, ws, B, mode, W);
  if (mode != 0) {
    WgradList wl(nullptr);
    vae_wgrads(P, K, W, nullptr, B, wl, ws);
  }
  return ws.off;
}

// ------------------------------------------------------------------------------------------------ kernels
constexpr int GH_THREADS = 256;    // 4 waves of 64
constexpr int GH_ROWS = 8;         // rows of a tile
constexpr int GH_ZMAX = 64;        // widest latent the fused kernel takes
constexpr int GH_PER = GH_ROWS * GH_ZMAX / GH_THREADS;   // (row, column) outputs per thread at z = GH_ZMAX

// the KL term of one latent element, in double on the fp32 (mu, lv): 1 + lv - mu^2 - exp(lv) cancels to a few 1e-2 at an untrained head
__device__ __forceinline__ double kld_term(float mu, float lv) {
  const double m = (double)mu, l = (double)lv;
  return (l - expm1(l)) - m * m;
}

// element g of the draw (seed, offset): the number ardae_philox_normal_at writes there
__device__ __forceinline__ float philox_normal_element(uint64_t seed, uint64_t offset, uint64_t g) {
  float v[4];
  philox_normal4(seed, offset, g >> 2, v);
  const int u = (int)(g & 3);
  return u == 0 ? v[0] : u == 1 ? v[1] : u == 2 ? v[2] : v[3];
}

// One workgroup per GH_ROWS rows of hid [B, h].  Output o = t + 256 i of the tile is (row o / zd, column o % zd): consecutive lanes hold
// consecutive columns, so a wave's global stores are contiguous and its read of the hidden row is one broadcast address.  Each thread
// walks its two weight rows and the hidden row from global memory in 16-byte pieces (all three are L2 / L1 resident: the head's weights
// are 2 z h floats) with no barrier in the k loop, so the loads of later pieces are in flight under the FMAs of earlier ones; a first
// version that staged 16-wide k panels through LDS spent its time in 2 x h / 16 barriers.  Where h is no multiple
// of 4 or a base is not 16-byte aligned the same products are read one float at a time - the sum is the same chain of FMAs over
// ascending k either way.  Rows past B compute nothing and store nothing.
__global__ __launch_bounds__(GH_THREADS) void gauss_head_kernel(const float* __restrict__ hid, int B, int h, int zd, const float* __restrict__ Wm,
                                                                const float* __restrict__ bm, const float* __restrict__ Wl,
                                                                const float* __restrict__ bl, const float* __restrict__ eps_in, uint64_t seed,
                                                                uint64_t offset, const StepState* __restrict__ state, float* __restrict__ mu_out,
                                                                float* __restrict__ lv_out, float* __restrict__ z_out, float* __restrict__ eps_out,
                                                                float* __restrict__ kld_out) {
  __shared__ double kt[GH_ROWS][GH_ZMAX + 1];
  const int t = threadIdx.x;
  const int r0 = blockIdx.x * GH_ROWS;
  const int nout = GH_ROWS * zd;
  const bool vec = (h & 3) == 0 && ((reinterpret_cast<uintptr_t>(hid) | reinterpret_cast<uintptr_t>(Wm) | reinterpret_cast<uintptr_t>(Wl)) & 15) == 0;
  float am[GH_PER], al[GH_PER];
#pragma unroll
  for (int i = 0; i < GH_PER; ++i) {
    am[i] = al[i] = 0.f;
    const int o = t + i * GH_THREADS;
    const int r = o / zd, c = o - r * zd;
    if (o >= nout || r0 + r >= B) continue;
    const float* __restrict__ hr = hid + (size_t)(r0 + r) * h;
    const float* __restrict__ mr = Wm + (size_t)c * h;
    const float* __restrict__ lr = Wl + (size_t)c * h;
    float a = 0.f, b = 0.f;
    if (vec) {
#pragma unroll 4
      for (int k = 0; k < h; k += 4) {             // ascending k
        const f32x4 hv = *reinterpret_cast<const f32x4*>(hr + k);
        const f32x4 mv = *reinterpret_cast<const f32x4*>(mr + k);
        const f32x4 lw = *reinterpret_cast<const f32x4*>(lr + k);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          a = __builtin_fmaf(hv[u], mv[u], a);
          b = __builtin_fmaf(hv[u], lw[u], b);
        }
      }
    } else {
      for (int k = 0; k < h; ++k) {
        a = __builtin_fmaf(hr[k], mr[k], a);
        b = __builtin_fmaf(hr[k], lr[k], b);
      }
    }
    am[i] = a; al[i] = b;
  }

  if (state) offset += state->rng_offset;
#pragma unroll
  for (int i = 0; i < GH_PER; ++i) {
    const int o = t + i * GH_THREADS;
    if (o < nout) {
      const int r = o / zd, c = o - r * zd, gr = r0 + r;
      double term = 0.0;
      if (gr < B) {
        const float m = am[i] + bm[c], l = al[i] + bl[c];
        const uint64_t g = (uint64_t)gr * zd + c;
        const float e = eps_in ? eps_in[g] : philox_normal_element(seed, offset, g);
        mu_out[g] = m;
        lv_out[g] = l;
        z_out[g] = m + __expf(0.5f * l) * e;
        if (eps_out) eps_out[g] = e;
        term = kld_term(m, l);
      }
      kt[r][c] = term;
    }
  }
  __syncthreads();
  if (t < GH_ROWS && r0 + t < B) {
    double s = 0.0;
    for (int c = 0; c < zd; ++c) s += kt[t][c];      // ascending c
    kld_out[r0 + t] = (float)(-0.5 * s);
  }
}

// The head's tail as ONE launch, for a family whose two products run on the MFMA linears (kind 11, csrc/convvae.hip): from mu, lv [B, zd] the
// draw (keyed like ardae_philox_normal_at) or the injected eps, z and the row's KL - the expressions and the order of the three unfused launches
// (ardae_philox_normal_at, reparam_fwd_kernel, gauss_kld_rows_kernel), so its outputs equal theirs bit for bit.  Tiles and LDS as gauss_head_kernel.
__global__ __launch_bounds__(GH_THREADS) void gauss_head_tail_kernel(const float* __restrict__ mu, const float* __restrict__ lv, int B, int zd,
                                                                     const float* __restrict__ eps_in, uint64_t seed, uint64_t offset,
                                                                     const StepState* __restrict__ state, float* __restrict__ z_out,
                                                                     float* __restrict__ eps_out, float* __restrict__ kld_out) {
  __shared__ double kt[GH_ROWS][GH_ZMAX + 1];
  const int t = threadIdx.x;
  const int r0 = blockIdx.x * GH_ROWS;
  const int nout = GH_ROWS * zd;
  if (state) offset += state->rng_offset;
#pragma unroll
  for (int i = 0; i < GH_PER; ++i) {
    const int o = t + i * GH_THREADS;
    if (o < nout) {
      const int r = o / zd, c = o - r * zd, gr = r0 + r;
      double term = 0.0;
      if (gr < B) {
        const uint64_t g = (uint64_t)gr * zd + c;
        const float m = mu[g], l = lv[g];
        const float e = eps_in ? eps_in[g] : philox_normal_element(seed, offset, g);
        z_out[g] = m + __expf(0.5f * l) * e;
        if (eps_out) eps_out[g] = e;
        term = kld_term(m, l);
      }
      kt[r][c] = term;
    }
  }
  __syncthreads();
  if (t < GH_ROWS && r0 + t < B) {
    double s = 0.0;
    for (int c = 0; c < zd; ++c) s += kt[t][c];      // ascending c
    kld_out[r0 + t] = (float)(-0.5 * s);
  }
}

// the unfused head's last launch: kld[r] from (mu, lv) [B, zd], one thread per row, the same terms in the same order
__global__ void gauss_kld_rows_kernel(const float* __restrict__ mu, const float* __restrict__ lv, int B, int zd, float* __restrict__ kld) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= B) return;
  double s = 0.0;
  for (int c = 0; c < zd; ++c) s += kld_term(mu[(size_t)r * zd + c], lv[(size_t)r * zd + c]);
  kld[r] = (float)(-0.5 * s);
}

// the backward seed at the head, one launch: dmu = dz + c beta mu;  dlv = dz (z - mu) / 2 + c beta (exp(lv) - 1) / 2
__global__ void gauss_head_seed_kernel(const float* __restrict__ dz, const float* __restrict__ z, const float* __restrict__ mu,
                                       const float* __restrict__ lv, int64_t n, float cscale, float beta_v, const float* __restrict__ beta_p,
                                       float* __restrict__ dmu, float* __restrict__ dlv) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float cb = cscale * (beta_p ? *beta_p : beta_v);
  const float g = dz[i], m = mu[i];
  dmu[i] = __builtin_fmaf(cb, m, g);
  dlv[i] = 0.5f * (g * (z[i] - m) + cb * expm1f(lv[i]));
}

// IWAE under the analytic posterior: k samples per image and their log-density.  A workgroup takes IQ_SAMPLES samples; a thread owns
// elements of z (contiguous stores), the terms of a sample meet in LDS and ONE thread adds them over ascending c.
constexpr int IQ_THREADS = 256, IQ_SAMPLES = 64;
__global__ __launch_bounds__(IQ_THREADS) void vae_iwae_draw_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                                   const float* __restrict__ eps_in, int64_t S, int k, int zd, uint64_t seed,
                                                                   uint64_t offset, uint64_t first_element, float* __restrict__ z_out,
                                                                   float* __restrict__ logq, float* __restrict__ eps_out) {
  __shared__ double term[IQ_SAMPLES][GH_ZMAX + 1];
  const int t = threadIdx.x;
  const int64_t s0 = (int64_t)blockIdx.x * IQ_SAMPLES;
  const int ns = (int)((S - s0) < IQ_SAMPLES ? (S - s0) : IQ_SAMPLES);
  for (int p = t; p < ns * zd; p += IQ_THREADS) {
    const int j = p / zd, c = p - j * zd;
    const int64_t s = s0 + j, b = s / k;
    const uint64_t g = (uint64_t)s * zd + c;
    const float m = mu[b * zd + c], l = lv[b * zd + c];
    const float e = eps_in ? eps_in[g] : philox_normal_element(seed, offset, first_element + g);
    const float zv = m + __expf(0.5f * l) * e;
    z_out[g] = zv;
    if (eps_out) eps_out[g] = e;
    const double d = (double)zv - (double)m;
    term[j][c] = d * d / exp((double)l) + (double)l + 1.8378770664093454836;      // utils/stat.py:78
  }
  __syncthreads();
  if (t < ns) {
    double s = 0.0;
    for (int c = 0; c < zd; ++c) s += term[t][c];
    logq[s0 + t] = (float)(-0.5 * s);
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ the head, fused or not (vaemodel.h)
// what the fused forms can compute at all (ardae_vae_head's variant 1) ...
bool gauss_head_fused_can(const GaussHead& H) { return H.zd >= 1 && H.zd <= GH_ZMAX && H.h >= 1; }
// ... and where gauss_head_kernel may be the default: where the rows of both head matrices start on 16 bytes (h a multiple of 4 and both parameter
// offsets multiples of 4 floats - a z that is a multiple of 4, given such an h).  Elsewhere the kernel reads float by float and a narrow head
// leaves most of a workgroup idle: at the toy recipe's z = 2 it only ties with the unfused launches, which run there.
bool gauss_head_fused_ok(const GaussHead& H) { return gauss_head_fused_can(H) && (H.h & 3) == 0 && (H.mean.w & 3) == 0 && (H.logvar.w & 3) == 0; }

// variant 0: the library's choice (fused where H.fused_default, unless the debug knob says otherwise), 1: fused, 2: unfused
int gauss_head_fwd(const GaussHead& H, const float* params, const float* packed, const float* hid, const float* eps, int B, uint64_t seed,
                   uint64_t offset, const void* state, int variant, float* mu, float* lv, float* z, float* eps_out, float* kld, hipStream_t st) {
  if (variant == 0) {
    const char* knob = debug_knob("ARDAE_VAE_HEAD_UNFUSED");
    variant = (H.fused_default && !(knob && knob[0] == '1')) ? 1 : 2;
  }
  if (variant == 1) ARDAE_CHECK_ARG(gauss_head_fused_can(H), "vae_head: the fused head takes 1 <= z_dim <= %d (got %d)", GH_ZMAX, H.zd);
  else ARDAE_CHECK_ARG(eps || eps_out, "vae_head: the unfused head draws into eps_out (null pointer)");
  if (variant == 1 && !H.tail) {
    hipLaunchKernelGGL(gauss_head_kernel, dim3((unsigned)ceil_div(B, GH_ROWS)), dim3(GH_THREADS), 0, st, hid, B, H.h, H.zd, params + H.mean.w,
                       params + H.mean.b, params + H.logvar.w, params + H.logvar.b, eps, seed, offset, (const StepState*)state, mu, lv, z, eps_out, kld);
    ARDAE_LAUNCH_CHECK();
    return 0;
  }
  ARDAE_TRY(dense_fwd(ACT_NONE, B, H.zd, hid, H.h, H.h, packed + H.mean_f, params + H.mean.b, mu, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, B, H.zd, hid, H.h, H.h, packed + H.logvar_f, params + H.logvar.b, lv, st));
  if (variant == 1) {      // the tail form: what is left after the two products, in one launch
    hipLaunchKernelGGL(gauss_head_tail_kernel, dim3((unsigned)ceil_div(B, GH_ROWS)), dim3(GH_THREADS), 0, st, mu, lv, B, H.zd, eps, seed, offset,
                       (const StepState*)state, z, eps_out, kld);
    ARDAE_LAUNCH_CHECK();
    return 0;
  }
  if (!eps) {
    ARDAE_TRY(launch_philox_normal_at(eps_out, (int64_t)B * H.zd, seed, offset, state, 0, st));
    eps = eps_out;
  } else if (eps_out && eps_out != eps) {
    ARDAE_TRY(launch_copy(eps, (int64_t)B * H.zd, eps_out, st));
  }
  ARDAE_TRY(launch_reparam_fwd(mu, lv, eps, H.zd, B, H.zd, 1, z, st));
  hipLaunchKernelGGL(gauss_kld_rows_kernel, dim3(nblk(B)), dim3(256), 0, st, mu, lv, B, H.zd, kld);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

int gauss_head_seed(const float* dz, const float* z, const float* mu, const float* lv, int64_t n, float c, DevFloat beta, float* dmu, float* dlv,
                    hipStream_t st) {
  hipLaunchKernelGGL(gauss_head_seed_kernel, dim3(nblk(n)), dim3(256), 0, st, dz, z, mu, lv, n, c, beta.v, beta.p, dmu, dlv);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

// what ardae_model_encode / ardae_model_vae_* answer for the Gaussian-posterior kinds (Family members)
#define GAUSS_KINDS "kinds 8 / 9 / 11 / 12 / 14 / 15 / 17 / 19"
int vae_no_encode(const ardae_model_desc&, const float*, const float*, const float*, const float*, int, int, float*, size_t, float*, float*, hipStream_t,
                  const float*) {
  set_last_error("model_encode: " GAUSS_KINDS " have an analytic posterior, not a sampler (ardae_vae_encode_stats, ardae_vae_forward)");
  return -1;
}
int vae_no_forward(const ardae_model_desc&, const float*, const float*, const float*, const float*, int, int, DevFloat, float*, size_t, float*, float*,
                   hipStream_t) {
  set_last_error("model_vae_forward: " GAUSS_KINDS " are driven by ardae_vae_forward");
  return -1;
}
int vae_no_backward(const ardae_model_desc&, const float*, const float*, const float*, const float*, int, int, DevFloat, float, const float*, float*,
                    size_t, float*, float, hipStream_t) {
  set_last_error("model_vae_backward: " GAUSS_KINDS " are driven by ardae_vae_backward");
  return -1;
}

namespace {

// ------------------------------------------------------------------------------------------------ kinds 8 / 9: the traits and the family row
struct VaeTraits {
  using Layout = VaeLayout; using Packed = VaePacked; using Entry = VaeEntry;
  struct Grads { float* grads; float beta; };
  static Entry open(const ardae_model_desc& d, float* workspace, size_t wsf, int B, int mode) { return Entry(d, workspace, wsf, B, mode); }
  static GaussHead head_of(const VaeLayout& P, const VaePacked& K) {
    GaussHead H{P.h, P.zd, P.mean, P.logvar, K.mean_f, K.logvar_f, false, false};
    H.fused_default = gauss_head_fused_ok(H);
    return H;
  }
  static const float* hid(const VaeWs& W) { return W.e.back(); }
  static GaussBufs bufs(const VaeWs& W) {
    return {W.mu, W.lv, W.z, W.eps, W.kld, W.rec_row, W.pri_row, W.D.o[0], W.D.o[1], W.D.dox[0], W.D.dox[1], W.D.dzq, W.D.dz, W.dmu, W.dlv};
  }
  // xs (kind 8: 2x - 1) and the encoder stack
  static int encoder_fwd(Entry& e, const float* params, const float* packed, const float* x, int B, hipStream_t st) {
    auto& [P, K, ws, W] = e;
    if (!P.toy) ARDAE_TRY(launch_affine(x, (int64_t)B * P.D, 2.f, -1.f, W.xs, st));      // vae/mnist.py:54
    return K.enc.fwd(params, packed, P.act, B, P.toy ? x : W.xs, W.e.data(), st);
  }
  static int decoder_fwd(Entry& e, const float* params, const float* packed, int B, hipStream_t st) {
    return e.K.dec.fwd(params, packed, e.P.act, B, e.W.z, e.W.D.hid.data(), e.W.D.o, st);
  }
  static Grads grads_of(Entry&, const float*, const float*, float* grads, float grads_beta) { return {grads, grads_beta}; }
  static int decoder_bwd(Entry& e, const float* packed, int B, Grads&, hipStream_t st) { return e.K.dec.bwd(packed, e.P.act, B, e.W.D, st); }
  static int encoder_bwd(Entry& e, const float* packed, const float* x, int B, Grads& g, hipStream_t st) {
    auto& [P, K, ws, W] = e;
    ARDAE_TRY(dense_bwd2(P.act, B, P.h, W.dmu, packed + K.mean_b, W.dlv, packed + K.logvar_b, P.zd, W.e[P.nl], W.de[P.nl], st));
    ARDAE_TRY(K.enc.bwd(packed, P.act, B, W.e.data(), W.de.data(), st));
    WgradList wl(g.grads, g.beta);
    vae_wgrads(P, K, W, x, B, wl, ws);
    ARDAE_CHECK_ARG(ws.ok, "vae_backward: internal workspace accounting error");
    return wl.launch(st);
  }
};

size_t vae_workspace_floats(const ardae_model_desc& d, int B, int nz, int mode) {
  const VaeLayout P(d);
  if (mode == 2) return VaePacked(P).dec.decode_floats((size_t)B * nz);
  if (nz != 1 || mode == 3) return 0;         // one draw per image; there is no sampler pair
  return workspace_floats(P, B, mode);
}
// the descriptor rules of kinds 8 / 9 (noise_dim 0, flags 0, 1 .. 4 layers, any activation but NONE)
int vae_desc_check(const ardae_model_desc* d) {
  ARDAE_CHECK_ARG(d->noise_dim == 0, "model: noise_dim must be 0 for kinds 8 / 9 (the Gaussian posterior takes no noise input), got %d", d->noise_dim);
  ARDAE_CHECK_ARG(d->flags == 0, "model: flags must be 0 for kinds 8 / 9, got %d", d->flags);
  ARDAE_CHECK_ARG(d->input_dim >= 1 && d->h_dim >= 1 && d->z_dim >= 1 && d->n_layers >= 1 && d->n_layers <= 4, "model: bad dimensions");
  ARDAE_CHECK_ARG(d->act > ACT_NONE && d->act <= ACT_LAST, "model: unknown activation %d (relu, softplus, elu, tanh, leaky_relu, swish)", d->act);
  return 0;
}
unsigned vae_caps(const ardae_model_desc& d) { return d.kind == 9 ? CAP_GAUSS_DECODER : 0; }      // ToyVAE: mean and logvar heads
// (host pass only, as in csrc/auxmodel.hip)
#ifndef __HIP_DEVICE_COMPILE__
const GaussFamily VAE_GAUSS = gauss_family<VaeTraits>();
#endif

// ------------------------------------------------------------------------------------------------ the ardae_vae_* entry points, every Gaussian kind
// the kinds they take (the rows of the table that have a GaussFamily), and the kind's descriptor rules
int vae_kind_check(const ardae_model_desc* d, const char* who) {
  ARDAE_CHECK_ARG(d != nullptr, "%s: desc is NULL", who);
  ARDAE_CHECK_ARG(family_of(d->kind) && family(d).gauss,
                  "%s: kind must be 8 (MNISTVAE), 9 (ToyVAE) or 11 (MNISTConvVAE), or 12 (MNISTResConvVAE), or 14 (MNISTAuxVAE) or 15 (ToyAuxVAE), or 17 (MNISTConvAuxVAE), or 19 (MNISTResConvAuxVAE), got %d", who, d->kind);
  return family(d).desc_check(d);
}

// what every ardae_vae_* entry point checks before anything is launched
int vae_common(const ardae_model_desc* d, const float* params, const float* packed, const float* x, int B, float* workspace, size_t wsf, int mode,
               const char* who) {
  ARDAE_TRY(vae_kind_check(d, who));
  ARDAE_CHECK_ARG(params && packed && x && workspace, "%s: null pointer argument", who);
  ARDAE_CHECK_ARG(B > 0 && B < (1 << 24), "%s: bad batch (B=%d)", who, B);
  const size_t need = family(d).workspace_floats(*d, B, 1, mode);
  ARDAE_CHECK_ARG(wsf >= need, "%s: workspace too small (%zu < %zu floats)", who, wsf, need);
  return 0;
}

int vae_forward_entry(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* eps, int B, DevFloat beta,
                      float loss_scale, uint64_t seed, uint64_t offset, const void* state, float* workspace, size_t wsf, float* z_out, float* eps_out,
                      float* losses, void* stream) {
  ARDAE_TRY(vae_common(d, params, packed, x, B, workspace, wsf, 1, "vae_forward"));
  ARDAE_CHECK_ARG(z_out && losses, "vae_forward: null pointer argument (z_out, losses)");
  ARDAE_CHECK_ARG(std::isfinite(loss_scale), "vae_forward: loss_scale must be finite");
  return family(d).gauss->forward(*d, params, packed, x, eps, B, beta, seed, offset, state, workspace, wsf, z_out, eps_out, losses, (hipStream_t)stream);
}

int vae_backward_entry(const ardae_model_desc* d, const float* params, const float* packed, const float* x, int B, DevFloat beta, float loss_scale,
                       float* workspace, size_t wsf, float* grads, float grads_beta, void* stream) {
  ARDAE_TRY(vae_common(d, params, packed, x, B, workspace, wsf, 1, "vae_backward"));
  ARDAE_CHECK_ARG(grads, "vae_backward: null pointer argument (grads)");
  ARDAE_CHECK_ARG(std::isfinite(loss_scale) && std::isfinite(grads_beta), "vae_backward: loss_scale and grads_beta must be finite");
  return family(d).gauss->backward(*d, params, packed, x, B, beta, loss_scale, workspace, wsf, grads, grads_beta, (hipStream_t)stream);
}

}  // namespace

// (host pass only, as in csrc/auxmodel.hip)
#ifndef __HIP_DEVICE_COMPILE__
const Family VAE_FAMILY = {vae_desc_check, vae_caps, family_param_floats<VaeLayout, VaePacked>, family_packed_floats<VaeLayout, VaePacked>, vae_workspace_floats,
                           family_pack<VaeLayout, VaePacked>, vae_no_encode, mlp_decode<VaeLayout, VaePacked>, vae_no_forward, vae_no_backward,
                           &VAE_GAUSS};
#endif

}  // namespace ardae

using namespace ardae;

extern "C" {

int ardae_vae_head_fused_ok(const ardae_model_desc* d) {
  if (!d || vae_kind_check(d, "vae_head_fused_ok") != 0) return 0;
  return family(d).gauss->head_fused_ok(*d) ? 1 : 0;
}

int ardae_vae_kld_rows(const float* mu, const float* lv, int B, int z, float* kld, void* stream) {
  ARDAE_CHECK_ARG(B > 0 && z > 0, "vae_kld_rows: need B > 0 and z > 0 (got B=%d, z=%d)", B, z);
  ARDAE_CHECK_ARG(mu && lv && kld, "vae_kld_rows: null pointer argument");
  hipLaunchKernelGGL(gauss_kld_rows_kernel, dim3(nblk(B)), dim3(256), 0, (hipStream_t)stream, mu, lv, B, z, kld);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

int ardae_vae_head(const ardae_model_desc* d, const float* params, const float* packed, const float* hid, const float* eps, int B, uint64_t seed,
                   uint64_t offset, const void* state, int variant, float* mu, float* lv, float* z_out, float* eps_out, float* kld, void* stream) {
  ARDAE_TRY(vae_kind_check(d, "vae_head"));
  ARDAE_CHECK_ARG(variant >= 0 && variant <= 2, "vae_head: variant must be 0 (the library's choice), 1 (fused) or 2 (unfused), got %d", variant);
  ARDAE_CHECK_ARG(params && packed && hid && mu && lv && z_out && kld, "vae_head: null pointer argument");
  ARDAE_CHECK_ARG(B > 0 && B < (1 << 24), "vae_head: bad batch (B=%d)", B);
  return family(d).gauss->head(*d, params, packed, hid, eps, B, seed, offset, state, variant, mu, lv, z_out, eps_out, kld, (hipStream_t)stream);
}

int ardae_vae_forward(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* eps, int B, float beta,
                      float loss_scale, uint64_t seed, uint64_t offset, const void* state, float* workspace, size_t workspace_floats_, float* z_out,
                      float* eps_out, float* losses, void* stream) {
  return vae_forward_entry(d, params, packed, x, eps, B, beta, loss_scale, seed, offset, state, workspace, workspace_floats_, z_out, eps_out, losses,
                           stream);
}
int ardae_vae_forward_dev(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* eps, int B,
                          const void* beta_state, float loss_scale, uint64_t seed, uint64_t offset, const void* state, float* workspace,
                          size_t workspace_floats_, float* z_out, float* eps_out, float* losses, void* stream) {
  ARDAE_CHECK_ARG(beta_state, "vae_forward_dev: beta_state is NULL");
  return vae_forward_entry(d, params, packed, x, eps, B, train_state_beta(beta_state), loss_scale, seed, offset, state, workspace, workspace_floats_,
                           z_out, eps_out, losses, stream);
}

int ardae_vae_backward(const ardae_model_desc* d, const float* params, const float* packed, const float* x, int B, float beta, float loss_scale,
                       float* workspace, size_t workspace_floats_, float* grads, float grads_beta, void* stream) {
  return vae_backward_entry(d, params, packed, x, B, beta, loss_scale, workspace, workspace_floats_, grads, grads_beta, stream);
}
int ardae_vae_backward_dev(const ardae_model_desc* d, const float* params, const float* packed, const float* x, int B, const void* beta_state,
                           float loss_scale, float* workspace, size_t workspace_floats_, float* grads, float grads_beta, void* stream) {
  ARDAE_CHECK_ARG(beta_state, "vae_backward_dev: beta_state is NULL");
  return vae_backward_entry(d, params, packed, x, B, train_state_beta(beta_state), loss_scale, workspace, workspace_floats_, grads, grads_beta, stream);
}

int ardae_vae_encode_stats(const ardae_model_desc* d, const float* params, const float* packed, const float* x, int B, float* workspace,
                           size_t workspace_floats_, float* mu_out, float* lv_out, void* stream) {
  ARDAE_TRY(vae_common(d, params, packed, x, B, workspace, workspace_floats_, 0, "vae_encode_stats"));
  ARDAE_CHECK_ARG(mu_out && lv_out, "vae_encode_stats: null pointer argument (mu_out, lv_out)");
  return family(d).gauss->encode_stats(*d, params, packed, x, B, workspace, workspace_floats_, mu_out, lv_out, (hipStream_t)stream);
}

int ardae_vae_iwae_draw(const float* mu, const float* lv, const float* eps, int B, int k, int z, uint64_t seed, uint64_t offset,
                        uint64_t first_element, float* z_out, float* logq, float* eps_out, void* stream) {
  ARDAE_CHECK_ARG(B > 0 && k > 0, "vae_iwae_draw: need B > 0 and k > 0 (got B=%d, k=%d)", B, k);
  ARDAE_CHECK_ARG(z >= 1 && z <= GH_ZMAX, "vae_iwae_draw: need 1 <= z <= %d (got z=%d)", GH_ZMAX, z);
  ARDAE_CHECK_ARG((int64_t)B * k <= INT32_MAX, "vae_iwae_draw: B k exceeds 2^31 - 1 rows (B=%d, k=%d)", B, k);
  ARDAE_CHECK_ARG((first_element & 3) == 0, "vae_iwae_draw: first_element must be a multiple of 4 (one Philox counter = 4 normals)");
  ARDAE_CHECK_ARG(mu && lv && z_out && logq, "vae_iwae_draw: null pointer argument (mu, lv, z_out, logq)");
  const int64_t S = (int64_t)B * k;
  hipLaunchKernelGGL(vae_iwae_draw_kernel, dim3((unsigned)ceil_div64(S, IQ_SAMPLES)), dim3(IQ_THREADS), 0, (hipStream_t)stream, mu, lv, eps, S, k, z,
                     seed, offset, first_element, z_out, logq, eps_out);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
