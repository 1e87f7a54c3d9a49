// The auxiliary-variable Gaussian baselines of vae.py (ardae_model_desc.kind 14: models/vae/auxmnist.py::VAE `--model auxmnist`, the "# hierarchical
// mlp" baseline of run_vae_dbmnist.sh; 15: models/vae/auxtoy.py::VAE `--model auxtoy`) - the Gaussian counterparts of kinds 3 / 7, joined from the MLP
// pieces (csrc/mlp.h), the shared Gaussian head (csrc/vaemodel.h) and the kernels the family adds: the KL between two diagonal Gaussians, its backward
// seed, and the row kernel of the three-stage importance-weighted evaluation.
//
//   per image (B rows):  xs = 2x - 1 (kind 14) | x (kind 15);  h0 = MLP_aux(xs);  mu0 = M0 h0 + m0;  lv0 = clip(L0 h0 + l0);  z0 = mu0 + exp(lv0 / 2) eps0
//                        h = MLP_enc([xs | z0]);  mu, lv, z, kld: the Gaussian head on h (no clip);  hr = MLP_auxdec([xs | z]);  mup = Mp hr + mp;
//                        lvp = Lp hr + lp;  aux_kld = -0.5 sum_c (1 - lvp + lv0 - (exp(lv0) + (mu0 - mup)^2) / exp(lvp))   (utils/vae.py:94-114)
//                        decoder and row reconstruction loss as kinds 8 / 9
//   losses = {mean_b(recon_b + beta (kld_b + aux_kld_b)), mean recon, mean (kld + aux_kld)}    (vae/auxmnist.py:313-364)
//   (the first layer of MLP_enc / MLP_auxdec eats cat[xs, .]: its image half enters as a row bias, as in csrc/auxmodel.hip, so the same code serves the
//    evaluation's k rows per image)
// Backward (c = loss_scale / B), every reparameterisation and both KLs in closed form:
//   dmup = c beta (mup - mu0) / exp(lvp);  dlvp = c beta (1 - (exp(lv0) + (mu0 - mup)^2) / exp(lvp)) / 2;  both back through MLP_auxdec into its z columns;
//   dz = the decoder's + the auxiliary decoder's;  dmu, dlv: gauss_head_seed;  back through MLP_enc into its z0 columns: dz0;
//   dmu0 = dz0 + c beta (mu0 - mup) / exp(lvp);  dlv0 = dz0 (z0 - mu0) / 2 + c beta (exp(lv0) / exp(lvp) - 1) / 2, then the clip's derivative;
//   back through MLP_aux; every weight gradient in one problem list.
// logprob (vae/auxmnist.py:381-451, sample_size2 = 1): k z0's per image, one z per z0, and ONE row
//   logq = log q(z0 | x) + log q(z | z0, x) - log r(z0 | z, x)   (ardae_vae_aux_iwae_draw); the prior, the decoder and the log-mean-exp are the other kinds'.
#include <cmath>

#include <vector>

#include "ardae_hip.h"
#include "auxmodel.h"
#include "auxvae.h"
#include "common.h"
#include "elementwise.h"
#include "mlp.h"
#include "philox.h"
#include "vaemodel.h"

namespace ardae {
namespace {

// A stack of Linear -> act layers whose first layer reads cat[xs, s]: xs [B, D] once per image (a row bias, with the layer's bias), s [R, sd] per row
// (R = B rows_per_group).  t[1 .. nl] are the layer outputs [R, h].
struct CondStack {
  Lin first;
  int D = 0, sd = 0, h = 0, nl = 0;
  size_t x_f = 0, s_f = 0, s_b = 0;
  MlpStack rest;     // layers 2 .. nl
  CondStack() {}
  CondStack(const Lin* l, int n, int D_, PackList& pl) : first(l[0]), D(D_), sd(l[0].in - D_), h(l[0].out), nl(n) {
    x_f = pl.panel(first.w, first.in, h, D, false);      // image half: forward only (x takes no gradient)
    pl.pair(first, s_f, s_b, D, sd);
    rest = MlpStack(l + 1, n - 1, pl);
  }
  int fwd(const float* params, const float* packed, int act, int B, int rpg, const float* xs, const float* s, float* rb, float* const* t,
          hipStream_t st) const {
    ARDAE_TRY(cat_fwd(act, B, rpg, h, xs, D, packed + x_f, params + first.b, s, sd, packed + s_f, rb, t[1], st));
    return rest.fwd(params, packed, act, B * rpg, t[1], t + 1, st);
  }
  // from dt[nl] down to dt[1], then ds [R, sd] = dt[1] Ws (+ q: what else arrives at s; ds must not be q)
  int bwd(const float* packed, int act, int R, float* const* t, float* const* dt, float* ds, const float* q, hipStream_t st) const {
    ARDAE_TRY(rest.bwd(packed, act, R, t + 1, dt + 1, st));
    if (nl >= 2) ARDAE_TRY(dense_bwd(act, R, h, dt[2], h, packed + rest.b[0], t[1], dt[1], st));
    return cat_bwd(R, h, dt[1], sd, packed + s_b, q, ds, D, nullptr, nullptr, nullptr, st);
  }
  // layers nl .. 2, the first layer's s half (+ bias), its image half (training: one row per image, so dt[1] is the row bias' gradient too)
  void wgrads(WgradList& wl, int B, const float* xs, const float* s, float* const* t, float* const* dt) const {
    for (int l = nl; l >= 2; --l) {
      const Lin& L = rest.lin[l - 2];
      wl.push(B, h, h, dt[l], t[l - 1], h, wl.g(L.w), h, wl.g(L.b));
    }
    cat_wgrads(wl, B, first, D, dt[1], s, xs);
  }
  void carve(Bump& ws, size_t R, std::vector<float*>& t) const {
    t.assign(nl + 1, nullptr);
    for (int l = 1; l <= nl; ++l) t[l] = ws.take(R * h);
  }
};

struct AuxVaeLayout {
  int kind, D, nd, h, zd, nl, act, clip0;
  bool toy;                                   // kind 15: no 2x - 1 rescale, Gaussian decoder
  std::vector<Lin> am, ef, dec, ad;           // aux_encode.main, encode.fc, decode.main, aux_decode.fc: nl Linear each, all followed by act
  Lin mean0, logvar0, mean, logvar, heads[2], meanp, logvarp;
  size_t total = 0;
  explicit AuxVaeLayout(const ardae_model_desc& d)
      : kind(d.kind), D(d.input_dim), nd(d.noise_dim), h(d.h_dim), zd(d.z_dim), nl(d.n_layers), act(d.act),
        clip0((d.flags >> ARDAE_MODEL_CLIP_Z0_SHIFT) & 15), toy(d.kind == 15) {
    size_t off = 0;
    auto one = [&](int out, int in) { return next_lin(off, out, in); };
    for (int l = 0; l < nl; ++l) am.push_back(one(h, l == 0 ? D : h));
    mean0 = one(nd, h); logvar0 = one(nd, h);
    for (int l = 0; l < nl; ++l) ef.push_back(one(h, l == 0 ? D + nd : h));
    mean = one(zd, h); logvar = one(zd, h);
    for (int l = 0; l < nl; ++l) dec.push_back(one(h, l == 0 ? zd : h));
    heads[0] = one(D, h);
    if (toy) heads[1] = one(D, h);
    for (int l = 0; l < nl; ++l) ad.push_back(one(h, l == 0 ? D + zd : h));
    meanp = one(nd, h); logvarp = one(nd, h);
    total = off;
  }
};

struct AuxVaePacked {
  MlpStack am;
  CondStack ef, ad;
  MlpDecoder dec;
  size_t mean0_f, mean0_b, logvar0_f, logvar0_b, mean_f, mean_b, logvar_f, logvar_b, meanp_f, meanp_b, logvarp_f, logvarp_b;
  AuxVaePacked(const AuxVaeLayout& P, PackList& pl) : am(P.am.data(), P.nl, pl) {
    pl.pair(P.mean0, mean0_f, mean0_b); pl.pair(P.logvar0, logvar0_f, logvar0_b);
    ef = CondStack(P.ef.data(), P.nl, P.D, pl);
    pl.pair(P.mean, mean_f, mean_b); pl.pair(P.logvar, logvar_f, logvar_b);
    dec = MlpDecoder(P.dec.data(), P.nl, P.heads, P.toy ? 2 : 1, pl);
    ad = CondStack(P.ad.data(), P.nl, P.D, pl);
    pl.pair(P.meanp, meanp_f, meanp_b); pl.pair(P.logvarp, logvarp_f, logvarp_b);
  }
  explicit AuxVaePacked(const AuxVaeLayout& P, PackList&& sizing = PackList()) : AuxVaePacked(P, sizing) {}   // offsets only
};

struct AuxVaeWs {
  float *xs, *mu0, *lv0, *lv0r;              // xs: 2x - 1 (kind 14) | a copy of x (kind 15); lv0r: the head's raw output where a clip is on (else lv0 itself); mode 0 (encode_stats) ends here
  std::vector<float*> e, de;                 // aux_encode.main [B, h]
  float *eps0, *epsz, *z0, *rb;              // the two draws [B, nd] / [B, zd], z0 [B, nd], the row bias [B, h]
  std::vector<float*> t, dt;                 // encode.fc
  float *mu, *lv, *z, *eps, *kld;            // the head's (eps: the draw it used, a copy of epsz)
  float *rb2;
  std::vector<float*> u, du;                 // aux_decode.fc
  float *mup, *lvp;
  MlpDecoder::Bufs D;
  float *rec_row, *pri_row;
  float *dmu, *dlv, *dz, *dz0, *dmu0, *dlv0, *dmup, *dlvp;      // dz: the decoder's + the auxiliary decoder's
};

// mode 0: aux_encode up to (mu0, lv0); 1: everything
void carve(const AuxVaeLayout& P, const AuxVaePacked& K, Bump& ws, int B, int mode, AuxVaeWs& W) {
  const size_t b = (size_t)B;
  W.xs = ws.take(b * P.D);
  K.am.carve(ws, b, W.e);
  W.mu0 = ws.take(b * P.nd); W.lv0 = ws.take(b * P.nd);
  W.lv0r = P.clip0 ? ws.take(b * P.nd) : W.lv0;
  if (mode == 0) return;
  W.eps0 = ws.take(b * P.nd); W.epsz = ws.take(b * P.zd); W.z0 = ws.take(b * P.nd); W.rb = ws.take(b * P.h);
  K.ef.carve(ws, b, W.t);
  W.mu = ws.take(b * P.zd); W.lv = ws.take(b * P.zd); W.z = ws.take(b * P.zd); W.eps = ws.take(b * P.zd); W.kld = ws.take(b);
  W.rb2 = ws.take(b * P.h);
  K.ad.carve(ws, b, W.u);
  W.mup = ws.take(b * P.nd); W.lvp = ws.take(b * P.nd);
  K.dec.carve(ws, b, true, W.D);
  W.rec_row = ws.take(b); W.pri_row = ws.take(b);
  W.dmu = ws.take(b * P.zd); W.dlv = ws.take(b * P.zd); W.dz = ws.take(b * P.zd);
  W.dz0 = ws.take(b * P.nd); W.dmu0 = ws.take(b * P.nd); W.dlv0 = ws.take(b * P.nd); W.dmup = ws.take(b * P.nd); W.dlvp = ws.take(b * P.nd);
  K.ef.carve(ws, b, W.dt);
  K.ad.carve(ws, b, W.du);
  K.am.carve(ws, b, W.de);
}
using AuxVaeEntry = Entry<AuxVaeLayout, AuxVaePacked, AuxVaeWs>;

int wgrad_nprob(const AuxVaeLayout& P) { return (P.toy ? 2 : 1) + P.nl + 2 + (P.nl + 1) + 2 + P.nl + 2 + (P.nl + 1); }

// every weight-gradient problem of the backward: decoder, the z head, encode.fc, the z0 head, aux_encode.main, the auxiliary decoder's head and stack
void auxvae_wgrads(const AuxVaeLayout& P, const AuxVaePacked& K, const AuxVaeWs& W, int B, WgradList& wl, Bump& ws) {
  const float* xs = W.xs;
  K.dec.wgrads(wl, B, W.z, W.D);
  wl.push(B, P.zd, P.h, W.dmu, W.t[P.nl], P.h, wl.g(P.mean.w), P.h, wl.g(P.mean.b));
  wl.push(B, P.zd, P.h, W.dlv, W.t[P.nl], P.h, wl.g(P.logvar.w), P.h, wl.g(P.logvar.b));
  K.ef.wgrads(wl, B, xs, W.z0, W.t.data(), W.dt.data());
  wl.push(B, P.nd, P.h, W.dmu0, W.e[P.nl], P.h, wl.g(P.mean0.w), P.h, wl.g(P.mean0.b));
  wl.push(B, P.nd, P.h, W.dlv0, W.e[P.nl], P.h, wl.g(P.logvar0.w), P.h, wl.g(P.logvar0.b));
  K.am.wgrads(wl, B, xs, W.e.data(), W.de.data());
  wl.push(B, P.nd, P.h, W.dmup, W.u[P.nl], P.h, wl.g(P.meanp.w), P.h, wl.g(P.meanp.b));
  wl.push(B, P.nd, P.h, W.dlvp, W.u[P.nl], P.h, wl.g(P.logvarp.w), P.h, wl.g(P.logvarp.b));
  K.ad.wgrads(wl, B, xs, W.z, W.u.data(), W.du.data());
  wl.assign(ws, wgrad_nprob(P));
}

// The evaluation pass (mode 4): xs [B, D] in front of the shared rows
struct AuxEvalWs : AuxEvalRows { float* xs; };

// ------------------------------------------------------------------------------------------------ kernels
constexpr int AV_THREADS = 256;    // 4 waves of 64
constexpr int PK_ROWS = 8;         // rows of a pair-KL tile (the training batch is 128 rows: 16 workgroups)
constexpr int AR_ROWS = 32;        // rows of an evaluation tile

// element g of the draw (seed, offset): the number ardae_philox_normal_at writes there
__device__ __forceinline__ float philox_normal_element(uint64_t seed, uint64_t offset, uint64_t g) {
  float v[4];
  philox_normal4(seed, offset, g >> 2, v);
  const int u = (int)(g & 3);
  return u == 0 ? v[0] : u == 1 ? v[1] : u == 2 ? v[2] : v[3];
}

// loss_kld_gaussian_vs_gaussian (utils/vae.py:94-114), row values: kld[r] = -0.5 sum_c (1 - lv2 + lv1 - (exp(lv1) + (mu1 - mu2)^2) / exp(lv2)) on
// [B, n] statistics, n <= AV_NMAX.  A workgroup takes PK_ROWS rows; a thread owns elements (contiguous loads), the terms - in double, written as
// (d - expm1(d)) - (mu1 - mu2)^2 exp(-lv2) with d = lv1 - lv2, which does not cancel at an untrained head - meet in LDS and ONE thread per row adds
// them over ascending c: a row's bits do not depend on B.  accumulate: kld[r] += (the head's KL row is already there).
__global__ __launch_bounds__(AV_THREADS) void pair_kld_rows_kernel(const float* __restrict__ mu1, const float* __restrict__ lv1,
                                                                   const float* __restrict__ mu2, const float* __restrict__ lv2, int B, int n,
                                                                   float* __restrict__ kld, int accumulate) {
  __shared__ double kt[PK_ROWS][AV_NMAX + 1];
  const int t = threadIdx.x;
  const int r0 = blockIdx.x * PK_ROWS;
  const int rows = B - r0 < PK_ROWS ? B - r0 : PK_ROWS;
  for (int p = t; p < rows * n; p += AV_THREADS) {
    const int r = p / n, c = p - r * n;
    const size_t g = (size_t)(r0 + r) * n + c;
    const double l2 = (double)lv2[g], d = (double)lv1[g] - l2, dm = (double)mu1[g] - (double)mu2[g];
    kt[r][c] = (d - expm1(d)) - dm * dm * exp(-l2);
  }
  __syncthreads();
  if (t < rows) {
    double s = 0.0;
    for (int c = 0; c < n; ++c) s += kt[t][c];      // ascending c
    const float v = (float)(-0.5 * s);
    kld[r0 + t] = accumulate ? kld[r0 + t] + v : v;
  }
}

// the backward seed of the pair KL, one launch on n = B nd elements (cb = c beta):
//   dmup = cb (mup - mu0) / exp(lvp);  dlvp = cb (1 - (exp(lv0) + (mu0 - mup)^2) / exp(lvp)) / 2;  dmu0 = -dmup;  dlv0 = cb (exp(lv0) / exp(lvp) - 1) / 2
__global__ void pair_kld_seed_kernel(const float* __restrict__ mu0, const float* __restrict__ lv0, const float* __restrict__ mup,
                                     const float* __restrict__ lvp, int64_t n, float cscale, float beta_v, const float* __restrict__ beta_p,
                                     float* __restrict__ dmup, float* __restrict__ dlvp, float* __restrict__ dmu0, float* __restrict__ dlv0) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float cb = cscale * (beta_p ? *beta_p : beta_v);
  const float lp = lvp[i], dm = mu0[i] - mup[i];
  const float ip = __expf(-lp), em = expm1f(lv0[i] - lp);      // exp(lv0) / exp(lvp) - 1
  const float gm = cb * dm * ip;
  dmup[i] = -gm;
  dlvp[i] = -0.5f * cb * (em + dm * dm * ip);
  dmu0[i] = gm;
  dlv0[i] = 0.5f * cb * em;
}

// the first reparameterisation's part of the first head's seed: dmu0 += dz0;  dlv0 += dz0 (z0 - mu0) / 2
__global__ void z0_seed_kernel(const float* __restrict__ dz0, const float* __restrict__ z0, const float* __restrict__ mu0, int64_t n,
                               float* __restrict__ dmu0, float* __restrict__ dlv0) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float g = dz0[i];
  dmu0[i] += g;
  dlv0[i] = __builtin_fmaf(0.5f * g, z0[i] - mu0[i], dlv0[i]);
}

// One stage of the evaluation on R rows of width n <= AV_NMAX, statistics (mu, lv) [R / rpg, n] (rpg rows share one: stage 1, the k draws of an
// image).  sample_in null: the row's draw v = mu + exp(lv / 2) e - e injected (eps_in, row stride ld_eps) or element `first + r n + c` of the draw
// (seed, offset), keyed like ardae_philox_normal_at - is written to sample_out (and e to eps_out); else v = sample_in (stage 3: the stored z0 under
// the auxiliary decoder's statistics).  The row's log-density -0.5 sum_c ((v - mu)^2 / exp(lv) + lv + log 2 pi) (utils/stat.py:65-85) is formed
// like vae_iwae_draw_kernel's - terms in double in LDS, ONE thread adds them over ascending c - and enters the row's double accumulator:
// acc_mode 0: acc = lp;  1: acc += lp;  2: logq = (float)(acc - lp).  So logq = (log q(z0|x) + log q(z|z0,x)) - log r(z0|z,x), in that order.
// (RowsArgs: csrc/auxvae.h)
__global__ __launch_bounds__(AV_THREADS) void aux_rows_kernel(const RowsArgs a) {
  __shared__ double term[AR_ROWS][AV_NMAX + 1];
  const int t = threadIdx.x, n = a.n;
  const int64_t r0 = (int64_t)blockIdx.x * AR_ROWS;
  const int rows = (int)(a.R - r0 < AR_ROWS ? a.R - r0 : AR_ROWS);
  for (int p = t; p < rows * n; p += AV_THREADS) {
    const int j = p / n, c = p - j * n;
    const int64_t r = r0 + j;
    const size_t g = (size_t)r * n + c, sg = (size_t)(r / a.rpg) * n + c;
    const float m = a.mu[sg], l = a.lv[sg];
    float v;
    if (a.sample_in) {
      v = a.sample_in[g];
    } else {
      const float e = a.eps_in ? a.eps_in[(size_t)r * a.ld_eps + c] : philox_normal_element(a.seed, a.offset, a.first + g);
      v = m + __expf(0.5f * l) * e;
      a.sample_out[g] = v;
      if (a.eps_out) a.eps_out[(size_t)r * a.ld_eps_out + c] = e;
    }
    const double d = (double)v - (double)m;
    term[j][c] = d * d / exp((double)l) + (double)l + 1.8378770664093454836;
  }
  __syncthreads();
  if (t < rows) {
    double s = 0.0;
    for (int c = 0; c < n; ++c) s += term[t][c];      // ascending c
    const double lp = -0.5 * s;
    const int64_t r = r0 + t;
    if (a.acc_mode == 0) a.acc[r] = lp;
    else if (a.acc_mode == 1) a.acc[r] += lp;
    else a.logq[r] = (float)(a.acc[r] - lp);
  }
}

}  // namespace

// the launchers the auxiliary families share (csrc/auxvae.h)
int launch_pair_kld_rows(const float* mu1, const float* lv1, const float* mu2, const float* lv2, int B, int n, float* kld, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(pair_kld_rows_kernel, dim3((unsigned)ceil_div(B, PK_ROWS)), dim3(AV_THREADS), 0, st, mu1, lv1, mu2, lv2, B, n, kld, accumulate);
  ARDAE_LAUNCH_CHECK();
  return 0;
}
int launch_pair_kld_seed(const float* mu0, const float* lv0, const float* mup, const float* lvp, int64_t n, float c, DevFloat beta, float* dmup, float* dlvp,
                         float* dmu0, float* dlv0, hipStream_t st) {
  hipLaunchKernelGGL(pair_kld_seed_kernel, dim3(nblk(n)), dim3(256), 0, st, mu0, lv0, mup, lvp, n, c, beta.v, beta.p, dmup, dlvp, dmu0, dlv0);
  ARDAE_LAUNCH_CHECK();
  return 0;
}
int launch_z0_seed(const float* dz0, const float* z0, const float* mu0, int64_t n, float* dmu0, float* dlv0, hipStream_t st) {
  hipLaunchKernelGGL(z0_seed_kernel, dim3(nblk(n)), dim3(256), 0, st, dz0, z0, mu0, n, dmu0, dlv0);
  ARDAE_LAUNCH_CHECK();
  return 0;
}
int launch_aux_rows(const RowsArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(aux_rows_kernel, dim3((unsigned)ceil_div64(a.R, AR_ROWS)), dim3(AV_THREADS), 0, st, a);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

namespace {

// ------------------------------------------------------------------------------------------------ kinds 14 / 15: the traits and the family row
struct AuxVaeTraits {
  using Layout = AuxVaeLayout; using Packed = AuxVaePacked; using Entry = AuxVaeEntry;
  static Entry open(const ardae_model_desc& d, float* workspace, size_t wsf, int B, int mode) { return Entry(d, workspace, wsf, B, mode); }
  // encode.reparam on encode.fc's last rows: kinds 8 / 9's head and policy
  static GaussHead head_of(const AuxVaeLayout& P, const AuxVaePacked& K) {
    GaussHead H{P.h, P.zd, P.mean, P.logvar, K.mean_f, K.logvar_f, false, false};
    H.fused_default = gauss_head_fused_ok(H);
    return H;
  }
  static const float* hid(const AuxVaeWs& W) { return W.t.back(); }
  static GaussBufs bufs(const AuxVaeWs& W) {
    return {W.mu, W.lv, W.z, W.eps, W.kld, W.rec_row, W.pri_row, W.D.o[0], W.D.o[1], W.D.dox[0], W.D.dox[1], W.D.dzq, W.D.dz, W.dmu, W.dlv};
  }
  // xs, aux_encode.main and its head: mu0, lv0 (clipped; where a clip is on, W.lv0r keeps the raw values)
  static int stats_fwd(Entry& en, const float* params, const float* packed, const float* x, int B, float* mu0, float* lv0, hipStream_t st) {
    auto& [P, K, ws, W] = en;
    float* lv0r = P.clip0 ? W.lv0r : lv0;
    if (P.toy) ARDAE_TRY(launch_copy(x, (int64_t)B * P.D, W.xs, st));      // no rescale (vae/auxtoy.py); the later stages read xs, not the caller's x
    else ARDAE_TRY(launch_affine(x, (int64_t)B * P.D, 2.f, -1.f, W.xs, st));      // vae/auxmnist.py:56
    ARDAE_TRY(K.am.fwd(params, packed, P.act, B, W.xs, W.e.data(), st));
    ARDAE_TRY(dense_fwd(ACT_NONE, B, P.nd, W.e[P.nl], P.h, P.h, packed + K.mean0_f, params + P.mean0.b, mu0, st));
    ARDAE_TRY(dense_fwd(ACT_NONE, B, P.nd, W.e[P.nl], P.h, P.h, packed + K.logvar0_f, params + P.logvar0.b, lv0r, st));
    return launch_logvar_clip(lv0r, nullptr, lv0, (int64_t)B * P.nd, P.clip0, st);
  }
  // (the two draws are in W.eps0 / W.epsz: aux_vae_forward)  aux_encode, z0, encode.fc
  static int encoder_fwd(Entry& en, const float* params, const float* packed, const float* x, int B, hipStream_t st) {
    auto& [P, K, ws, W] = en;
    ARDAE_TRY(stats_fwd(en, params, packed, x, B, W.mu0, W.lv0, st));
    ARDAE_TRY(launch_reparam_fwd(W.mu0, W.lv0, W.eps0, P.nd, B, P.nd, 1, W.z0, st));
    return K.ef.fwd(params, packed, P.act, B, 1, W.xs, W.z0, W.rb, W.t.data(), st);
  }
  // the auxiliary decoder on [xs | z] and the pair KL, added into the head's KL rows; then the decoder
  static int decoder_fwd(Entry& en, const float* params, const float* packed, int B, hipStream_t st) {
    auto& [P, K, ws, W] = en;
    ARDAE_TRY(K.ad.fwd(params, packed, P.act, B, 1, W.xs, W.z, W.rb2, W.u.data(), st));
    ARDAE_TRY(dense_fwd(ACT_NONE, B, P.nd, W.u[P.nl], P.h, P.h, packed + K.meanp_f, params + P.meanp.b, W.mup, st));
    ARDAE_TRY(dense_fwd(ACT_NONE, B, P.nd, W.u[P.nl], P.h, P.h, packed + K.logvarp_f, params + P.logvarp.b, W.lvp, st));
    ARDAE_TRY(launch_pair_kld_rows(W.mu0, W.lv0, W.mup, W.lvp, B, P.nd, W.kld, 1, st));
    return K.dec.fwd(params, packed, P.act, B, W.z, W.D.hid.data(), W.D.o, st);
  }
  struct Grads { float* grads; float beta; };
  static Grads grads_of(Entry&, const float*, const float*, float* grads, float grads_beta) { return {grads, grads_beta}; }
  static int decoder_bwd(Entry& en, const float* packed, int B, Grads&, hipStream_t st) { return en.K.dec.bwd(packed, en.P.act, B, en.W.D, st); }
  // the auxiliary decoder back into its z columns: dz = D.dz + du_1 Wz (xs takes no gradient)
  static int aux_decoder_bwd(Entry& en, const float* packed, int B, Grads&, hipStream_t st) {
    auto& [P, K, ws, W] = en;
    ARDAE_TRY(dense_bwd2(P.act, B, P.h, W.dmup, packed + K.meanp_b, W.dlvp, packed + K.logvarp_b, P.nd, W.u[P.nl], W.du[P.nl], st));
    return K.ad.bwd(packed, P.act, B, W.u.data(), W.du.data(), W.dz, W.D.dz, st);
  }
  static int encode_fc_bwd(Entry& en, const float* packed, int B, Grads&, hipStream_t st) {
    auto& [P, K, ws, W] = en;
    ARDAE_TRY(dense_bwd2(P.act, B, P.h, W.dmu, packed + K.mean_b, W.dlv, packed + K.logvar_b, P.zd, W.t[P.nl], W.dt[P.nl], st));
    return K.ef.bwd(packed, P.act, B, W.t.data(), W.dt.data(), W.dz0, nullptr, st);
  }
  // the clip's derivative on the raw log-variance, the first head, aux_encode.main; every weight gradient in one list
  static int aux_encoder_bwd(Entry& en, const float* packed, int B, Grads& g, hipStream_t st) {
    auto& [P, K, ws, W] = en;
    ARDAE_TRY(launch_logvar_clip(W.lv0r, W.dlv0, W.dlv0, (int64_t)B * P.nd, P.clip0, st));
    ARDAE_TRY(dense_bwd2(P.act, B, P.h, W.dmu0, packed + K.mean0_b, W.dlv0, packed + K.logvar0_b, P.nd, W.e[P.nl], W.de[P.nl], st));
    ARDAE_TRY(K.am.bwd(packed, P.act, B, W.e.data(), W.de.data(), st));
    WgradList wl(g.grads, g.beta);
    auxvae_wgrads(P, K, W, B, wl, ws);
    ARDAE_CHECK_ARG(ws.ok, "vae_backward: internal workspace accounting error");
    return wl.launch(st);
  }
  // the evaluation pass (aux_vae_iwae_draw, csrc/auxvae.h): the stages read xs
  using EvalWs = AuxEvalWs;
  static void carve_eval(const AuxVaeLayout& P, const AuxVaePacked&, Bump& ws, int B, int k, AuxEvalWs& W) {
    W.xs = ws.take((size_t)B * P.D);
    W.carve_rows(ws, B, k, P.nd, P.zd, P.h, P.nl);
  }
  static int eval_prepare(const AuxVaeLayout& P, const float* x, int B, AuxEvalWs& W, const float*& xs, hipStream_t st) {
    xs = x;
    if (P.toy) return 0;
    xs = W.xs;
    return launch_affine(x, (int64_t)B * P.D, 2.f, -1.f, W.xs, st);
  }
  static int eval_hidden(const AuxVaeLayout& P, const AuxVaePacked& K, const float* params, const float* packed, int stage, const float* xs, const float* s,
                         int B, int k, AuxEvalWs& W, const float*& hid, hipStream_t st) {
    hid = W.t[P.nl];
    return (stage == 2 ? K.ef : K.ad).fwd(params, packed, P.act, B, k, xs, s, W.rb, W.t.data(), st);
  }
};

size_t auxvae_workspace_floats(const ardae_model_desc& d, int B, int nz, int mode) {
  if (mode == 4) return aux_eval_floats<AuxVaeTraits>(d, B, nz);
  const AuxVaeLayout P(d);
  const AuxVaePacked K(P);
  if (mode == 2) return K.dec.decode_floats((size_t)B * nz);
  if (nz != 1 || (mode != 0 && mode != 1)) return 0;      // one draw per image; there is no sampler pair
  Bump ws;
  AuxVaeWs W;
  carve(P, K, ws, B, mode, W);
  if (mode == 1) {
    WgradList wl(nullptr);
    auxvae_wgrads(P, K, W, B, wl, ws);
  }
  return ws.off;
}

// the descriptor rules of kinds 14 / 15: 1 <= noise_dim <= AV_NMAX, flags: only aux_encode's clip_logvar code (0 .. 10), 1 .. 4 layers
int auxvae_desc_check(const ardae_model_desc* d) {
  ARDAE_CHECK_ARG(d->noise_dim >= 1 && d->noise_dim <= AV_NMAX, "model: noise_dim must be 1 .. %d for kinds 14 / 15 (the width of z0), got %d", AV_NMAX,
                  d->noise_dim);
  ARDAE_CHECK_ARG((d->flags & ~(15 << ARDAE_MODEL_CLIP_Z0_SHIFT)) == 0,
                  "model: unknown flags %d for kinds 14 / 15 (only the ARDAE_MODEL_CLIP_Z0 code, aux_encode's clip_logvar, is known)", d->flags);
  ARDAE_CHECK_ARG(((d->flags >> ARDAE_MODEL_CLIP_Z0_SHIFT) & 15) <= 10, "model: unknown log-variance clip code");
  ARDAE_CHECK_ARG(d->input_dim >= 1 && d->h_dim >= 1 && d->z_dim >= 1 && d->n_layers >= 1 && d->n_layers <= 4, "model: bad dimensions");
  ARDAE_CHECK_ARG(d->act > ACT_NONE && d->act <= ACT_LAST, "model: unknown activation %d (relu, softplus, elu, tanh, leaky_relu, swish)", d->act);
  return 0;
}
unsigned auxvae_caps(const ardae_model_desc& d) { return d.kind == 15 ? CAP_GAUSS_DECODER : 0; }      // ToyAuxVAE: mean and logvar heads

// (host pass only, as in csrc/auxmodel.hip)
#ifndef __HIP_DEVICE_COMPILE__
const GaussFamily AUXVAE_GAUSS = aux_gauss_family<AuxVaeTraits>();
#endif

}  // namespace

#ifndef __HIP_DEVICE_COMPILE__
const Family AUXVAE_FAMILY = {auxvae_desc_check, auxvae_caps, family_param_floats<AuxVaeLayout, AuxVaePacked>,
                              family_packed_floats<AuxVaeLayout, AuxVaePacked>, auxvae_workspace_floats, family_pack<AuxVaeLayout, AuxVaePacked>,
                              vae_no_encode, mlp_decode<AuxVaeLayout, AuxVaePacked>, vae_no_forward, vae_no_backward, &AUXVAE_GAUSS};
#endif

}  // namespace ardae

using namespace ardae;

extern "C" {

int ardae_vae_pair_kld_rows(const float* mu1, const float* lv1, const float* mu2, const float* lv2, int B, int n, float* kld, void* stream) {
  ARDAE_CHECK_ARG(B > 0 && n >= 1 && n <= AV_NMAX, "vae_pair_kld_rows: bad batch (need B > 0 and 1 <= n <= %d, got B=%d, n=%d)", AV_NMAX, B, n);
  ARDAE_CHECK_ARG(mu1 && lv1 && mu2 && lv2 && kld, "vae_pair_kld_rows: null pointer argument");
  return launch_pair_kld_rows(mu1, lv1, mu2, lv2, B, n, kld, 0, (hipStream_t)stream);
}

// the kinds the two aux entry points take: the rows of the table whose GaussFamily has the aux bodies; then the kind's descriptor rules
static int aux_kind_check(const ardae_model_desc* d, const char* who) {
  ARDAE_CHECK_ARG(d != nullptr, "%s: desc is NULL", who);
  const Family* f = family_of(d->kind);
  ARDAE_CHECK_ARG(f && f->gauss && f->gauss->aux_elbo_rows, "%s: kind must be 14 (MNISTAuxVAE) or 15 (ToyAuxVAE) or 17 (MNISTConvAuxVAE) or 19 (MNISTResConvAuxVAE), got %d", who, d->kind);
  return f->desc_check(d);
}

int ardae_vae_aux_elbo_rows(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* eps, int B, uint64_t seed,
                            uint64_t offset0, uint64_t offset1, uint64_t first_image, float* workspace, size_t workspace_floats_, float* recon_rows,
                            float* kld_rows, void* stream) {
  ARDAE_TRY(aux_kind_check(d, "vae_aux_elbo_rows"));
  ARDAE_CHECK_ARG(params && packed && x && workspace && recon_rows && kld_rows, "vae_aux_elbo_rows: null pointer argument");
  ARDAE_CHECK_ARG(B > 0 && B < (1 << 24), "vae_aux_elbo_rows: bad batch (B=%d)", B);
  ARDAE_CHECK_ARG(eps || (((first_image * (uint64_t)d->noise_dim) & 3) == 0 && ((first_image * (uint64_t)d->z_dim) & 3) == 0),
                  "vae_aux_elbo_rows: first_image noise_dim and first_image z_dim must be multiples of 4 (one Philox counter = 4 normals)");
  const size_t need = family(d).workspace_floats(*d, B, 1, 1);
  ARDAE_CHECK_ARG(workspace_floats_ >= need, "vae_aux_elbo_rows: workspace too small (%zu < %zu floats)", workspace_floats_, need);
  return family(d).gauss->aux_elbo_rows(*d, params, packed, x, eps, B, seed, offset0, offset1, first_image, workspace, workspace_floats_, recon_rows,
                                        kld_rows, (hipStream_t)stream);
}

int ardae_vae_aux_iwae_draw(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* mu0, const float* lv0,
                            const float* eps, int B, int k, uint64_t seed, uint64_t offset0, uint64_t offset1, uint64_t first_image, float* workspace,
                            size_t workspace_floats_, float* z_out, float* logq, float* eps_out, void* stream) {
  ARDAE_TRY(aux_kind_check(d, "vae_aux_iwae_draw"));
  ARDAE_CHECK_ARG(params && packed && x && mu0 && lv0 && workspace && z_out && logq, "vae_aux_iwae_draw: null pointer argument");
  ARDAE_CHECK_ARG(B > 0 && k > 0 && (int64_t)B * k < (int64_t)1 << 30, "vae_aux_iwae_draw: bad batch (B=%d, k=%d)", B, k);
  ARDAE_CHECK_ARG(d->z_dim <= AV_NMAX, "vae_aux_iwae_draw: need z_dim <= %d (got %d)", AV_NMAX, d->z_dim);
  ARDAE_CHECK_ARG(eps || (((first_image * (uint64_t)k * d->noise_dim) & 3) == 0 && ((first_image * (uint64_t)k * d->z_dim) & 3) == 0),
                  "vae_aux_iwae_draw: first_image k noise_dim and first_image k z_dim must be multiples of 4 (one Philox counter = 4 normals)");
  const size_t need = family(d).workspace_floats(*d, B, k, 4);
  ARDAE_CHECK_ARG(workspace_floats_ >= need, "vae_aux_iwae_draw: workspace too small (%zu < %zu floats)", workspace_floats_, need);
  return family(d).gauss->aux_iwae_draw(*d, params, packed, x, mu0, lv0, eps, B, k, seed, offset0, offset1, first_image, workspace, workspace_floats_,
                                        z_out, logq, eps_out, (hipStream_t)stream);
}

}  // extern "C"
