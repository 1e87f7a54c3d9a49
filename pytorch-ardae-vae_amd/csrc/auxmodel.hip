// MNISTAuxIPVAE (`--model auxmnist`, ardae_model_desc.kind == 3): the hierarchical implicit-posterior VAE of
// models/ivae/auxmnist.py:47-132 (Encoder = AuxEncoder + SimpleEncoder of models/vae/auxmnist.py:31-190 with enc_input = enc_noise =
// False and no log-variance clipping, as in the shipped recipe run_vae_dbmnist.sh) + models/vae/mnist.py Decoder, orchestrated from the
// K1 / K6w kernels like csrc/model.hip.  Oracle: oracle/ardae_oracle.py::aux_encode (pinned against the reference).
//
//   per image (B rows):   xs = 2x - 1;  h0 = MLP_aux(xs);  mu0 = M0 h0 + m0;  lv0 = L0 h0 + l0;  rb = Wx xs + b_1
//   per sample (R = B nz rows):  z0 = mu0[b] + exp(lv0[b] / 2) eps0;   t_1 = act(Wz z0 + rb[b]);  t_i = act(W_i t_{i-1} + b_i);
//                                 h = t_n;  mu = M h + m;  lv = L h + l;  z = mu + exp(lv / 2) eps
//   (the first encoder layer eats cat[xs, z0]: its image half is computed once per image and enters as a row bias - the
//    reference expands xs to R rows, vae/auxmnist.py:138-141)
// Noise layout of this kind: ONE [R, noise_dim + z_dim] tensor per sampler call, row = [eps0 | eps] (already scaled by std).
//
// kind 7, ToyAuxIPVAE (`--model auxmlp`, models/ivae/auxtoy.py:44-292 + models/vae/auxtoy.py + the Gaussian Decoder of models/vae/toy.py): the same
// networks WITHOUT the 2x - 1 rescale, a decoder with mean_fn / logvar_fn heads, and a SQUARE sampling scheme: the model-level calls take nz = q^2
// rows per image and run Encoder._forward with q = int(sqrt(nz)) (:215,230) - q z0's per image, the second stage on R = B q rows, q z's per
// z0: z [B q q, z] = mu[R][.] + exp(lv[R][.] / 2) eps.  Noise layout of kind 7: [eps0: R x noise_dim | eps: R q x z_dim], two blocks.
// Backward (closed form of the two reparameterisations):  dmu = dz, dlv = dz (z - mu) / 2;  dz0 = dt_1 Wz;
//   dmu0[b] = sum_nz dz0, dlv0[b] = sum_nz dz0 (z0 - mu0[b]) / 2.
#include <vector>

#include "auxmodel.h"
#include "ipmodel.h"
#include "elementwise.h"
#include "mlp.h"

namespace ardae {
namespace {

struct AuxLayout {
  int D, nd, h, zd, nl, act;
  int clip0, clip1;               // NormalDistribution.clip_logvar codes of the z0 / z heads (ardae_hip.h: ARDAE_MODEL_CLIP_*), 0 = none
  bool toy;                       // kind 7
  std::vector<Lin> am, ef, dec;   // aux_encode.main, encode.fc, decode.main: nl Linear each (nl - 1 hidden + fc, all followed by act)
  Lin mean0, logvar0, mean, logvar, heads[2];         // heads: decode.reparam.logit_fn, or (toy) mean_fn, logvar_fn
  size_t total = 0;
  // stage rows per image of a call with nz rows per image: nz, or (toy) q = sqrt(nz)
  int stage(int nz) const {
    if (!toy) return nz;
    int q = 1;
    while ((q + 1) * (q + 1) <= nz) ++q;
    return q;
  }
  explicit AuxLayout(const ardae_model_desc& d)
      : D(d.input_dim), nd(d.noise_dim), h(d.h_dim), zd(d.z_dim), nl(d.n_layers), act(d.act),
        clip0((d.flags >> ARDAE_MODEL_CLIP_Z0_SHIFT) & 15), clip1((d.flags >> ARDAE_MODEL_CLIP_Z_SHIFT) & 15), toy(d.kind == 7) {
    size_t off = 0;
    auto one = [&](int out, int in) { return next_lin(off, out, in); };
    for (int l = 0; l < nl; ++l) am.push_back(one(h, l == 0 ? D : h));
    mean0 = one(nd, h); logvar0 = one(nd, h);
    for (int l = 0; l < nl; ++l) ef.push_back(one(h, l == 0 ? D + nd : h));
    mean = one(zd, h); logvar = one(zd, h);
    for (int l = 0; l < nl; ++l) dec.push_back(one(h, l == 0 ? zd : h));
    heads[0] = one(D, h);
    if (toy) heads[1] = one(D, h);
    total = off;
  }
};

struct AuxPacked {
  MlpStack am, ef;   // ef: the encoder's layers 2 .. nl (the first one is a row bias plus its z0 half: efx_f, ef0_f / ef0_b)
  MlpDecoder dec;
  size_t efx_f, ef0_f, ef0_b, mean0_f, mean0_b, logvar0_f, logvar0_b, mean_f, mean_b, logvar_f, logvar_b;
  AuxPacked(const AuxLayout& P, PackList& pl) : am(P.am.data(), P.nl, pl) {
    pl.pair(P.mean0, mean0_f, mean0_b); pl.pair(P.logvar0, logvar0_f, logvar0_b);
    const Lin& e0 = P.ef[0];                                            // [h, D + nd]: image half (forward only) | z0 half
    efx_f = pl.panel(e0.w, e0.in, P.h, P.D, false);
    pl.pair(e0, ef0_f, ef0_b, P.D, P.nd);
    ef = MlpStack(P.ef.data() + 1, P.nl - 1, pl);
    pl.pair(P.mean, mean_f, mean_b); pl.pair(P.logvar, logvar_f, logvar_b);
    dec = MlpDecoder(P.dec.data(), P.nl, P.heads, P.toy ? 2 : 1, pl);
  }
  explicit AuxPacked(const AuxLayout& P, PackList&& sizing = PackList()) : AuxPacked(P, sizing) {}   // offsets only
};

struct AuxWs {
  float *xs, *mu0, *lv0, *rb, *z0, *mu, *lv, *z, *zero;
  float *lv0r, *lvr;                    // the heads' raw outputs when a log-variance clip is on (lv0 / lv then hold the clipped values)
  std::vector<float*> e, t;             // e[l] [B,h] (l = 1..nl), t[l] [R,h]
  MlpDecoder::Bufs D;                   // the decoder's, forward and backward (toy: o[0] = mean, o[1] = logvar)
  float *rec_row, *pri_row;             // row losses
  // backward
  float *dlv, *dz0, *dlv0r, *drb, *dmu0, *dlv0;
  float *dmu_s, *dlv_s;                 // toy: dz / dlv summed over the q z's of a stage row, [R, zd]
  std::vector<float*> dt, de;
};

int wgrad_nprob(const AuxLayout& P) { return 1 + (P.toy ? 1 : 0) + P.nl + 2 + P.nl + 1 + 2 + P.nl; }

// mode 0: sampler only; 1: + decoder, losses, backward, weight gradients
void carve(const AuxLayout& P, const AuxPacked& K, Bump& ws, int B, int nz, int mode, AuxWs& W) {
  const size_t R = (size_t)B * P.stage(nz), N = (size_t)B * nz, h = P.h;
  W.xs = ws.take((size_t)B * P.D);
  K.am.carve(ws, B, W.e);
  W.mu0 = ws.take((size_t)B * P.nd); W.lv0 = ws.take((size_t)B * P.nd); W.rb = ws.take((size_t)B * h);
  W.z0 = ws.take(R * P.nd);
  W.t.assign(P.nl + 1, nullptr);
  for (int l = 1; l <= P.nl; ++l) W.t[l] = ws.take(R * h);
  W.mu = ws.take(R * P.zd); W.lv = ws.take(R * P.zd); W.z = ws.take(N * P.zd);
  W.zero = ws.take(R * P.nd + N * P.zd);
  W.lv0r = P.clip0 ? ws.take((size_t)B * P.nd) : W.lv0;
  W.lvr = P.clip1 ? ws.take(R * P.zd) : W.lv;
  if (mode == 0) return;
  K.dec.carve(ws, N, true, W.D);
  W.rec_row = ws.take(N); W.pri_row = ws.take(N);
  W.dlv = ws.take(N * P.zd);
  W.dmu_s = P.toy ? ws.take(R * P.zd) : nullptr; W.dlv_s = P.toy ? ws.take(R * P.zd) : nullptr;
  W.dz0 = ws.take(R * P.nd); W.dlv0r = ws.take(R * P.nd);
  W.drb = ws.take((size_t)B * h); W.dmu0 = ws.take((size_t)B * P.nd); W.dlv0 = ws.take((size_t)B * P.nd);
  W.dt.assign(P.nl + 1, nullptr);
  for (int l = 1; l <= P.nl; ++l) W.dt[l] = ws.take(R * h);
  K.am.carve(ws, B, W.de);
}
using AuxEntry = Entry<AuxLayout, AuxPacked, AuxWs>;

// out[r][c] = mu[g][c] + exp(lv[g][c] / 2) * eps[r][c],  g = r / rows_per_group  (models/ivae/auxmnist.py:33-41)
__global__ void reparam_fwd_kernel(const float* __restrict__ mu, const float* __restrict__ lv, int ld_stat, const float* __restrict__ eps,
                                   int ld_eps, int64_t rows, int cols, int rows_per_group, float* __restrict__ out, float min_std,
                                   const float* __restrict__ raw, int ld_raw) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * cols; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cols;
    const int c = (int)(i - r * cols);
    const int64_t g = r / rows_per_group;
    const float e = eps[r * ld_eps + c];
    float v = mu[g * ld_stat + c] + __expf(0.5f * lv[g * ld_stat + c]) * e;
    if (min_std != 0.f) v += min_std * (raw ? raw[r * ld_raw + c] : e);
    out[i] = v;
  }
}
// dlv[r][c] = dz[r][c] * (z[r][c] - mu[g][c]) / 2    (z - mu = exp(lv / 2) eps: d z / d lv = (z - mu) / 2; with min_std: z - mu - min_std eps)
__global__ void reparam_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ z, const float* __restrict__ mu, int64_t rows,
                                   int cols, int rows_per_group, float* __restrict__ dlv, float min_std, const float* __restrict__ eps, int ld_eps) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * cols; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cols;
    const int c = (int)(i - r * cols);
    float d = z[i] - mu[(r / rows_per_group) * cols + c];
    if (min_std != 0.f) d -= min_std * eps[r * ld_eps + c];
    dlv[i] = 0.5f * dz[i] * d;
  }
}
int grid_of(int64_t n) {
  const int64_t g = (n + 255) / 256;
  return (int)(g < 4096 ? g : 4096);
}
}  // namespace
// NormalDistribution.clip_logvar (models/reparam.py:17-41) on a head's raw output x: y = c(x), or (dy given) the backward dx = dy c'(x).
// codes: 1 'hard' clamp to [MIN_LOGVAR, MAX_LOGVAR] = [-4, 2] (:7-8; torch.max / torch.min pass the gradient where x is strictly inside),
// 2 'softplus', 3 .. 8 'spmK' = softplus(x + K) - K for K = 10, 6, 5, 4, 3, 2, 9 'tanh', 10 '2tanh'
__global__ void logvar_clip_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ y, int64_t n, int code) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const float v = x[e];
  float f, d;
  if (code == 1) {
    f = fminf(fmaxf(v, -4.f), 2.f);
    d = (v > -4.f && v < 2.f) ? 1.f : ((v == -4.f || v == 2.f) ? 0.5f : 0.f);      // (ties: torch.max / min split the gradient evenly)
  } else if (code <= 8) {
    const float k = code == 2 ? 0.f : code == 3 ? 10.f : code == 4 ? 6.f : code == 5 ? 5.f : code == 6 ? 4.f : code == 7 ? 3.f : 2.f;
    const float u = v + k;
    f = (u > 20.f ? u : log1pf(expf(u))) - k;
    d = 1.f / (1.f + expf(-u));
  } else {
    const float t = tanhf(v), s = code == 9 ? 1.f : 2.f;
    f = s * t;
    d = s * (1.f - t * t);
  }
  y[e] = dy ? dy[e] * d : f;
}
int launch_logvar_clip(const float* x, const float* dy, float* y, int64_t n, int code, hipStream_t st) {
  if (code == 0 || n == 0) return 0;
  hipLaunchKernelGGL(logvar_clip_kernel, dim3(grid_of(n)), dim3(256), 0, st, x, dy, y, n, code);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

int launch_reparam_fwd(const float* mu, const float* lv, const float* eps, int ld_eps, int64_t rows, int cols, int rpg, float* out, hipStream_t st,
                       float min_std, const float* raw, int ld_raw) {
  hipLaunchKernelGGL(reparam_fwd_kernel, dim3(grid_of(rows * cols)), dim3(256), 0, st, mu, lv, cols, eps, ld_eps, rows, cols, rpg, out, min_std, raw, ld_raw);
  ARDAE_LAUNCH_CHECK();
  return 0;
}
int launch_reparam_bwd(const float* dz, const float* z, const float* mu, int64_t rows, int cols, int rpg, float* dlv, hipStream_t st, float min_std,
                       const float* eps, int ld_eps) {
  ARDAE_CHECK_ARG(min_std == 0.f || eps, "reparam_bwd: min_std needs the forward draw");
  hipLaunchKernelGGL(reparam_bwd_kernel, dim3(grid_of(rows * cols)), dim3(256), 0, st, dz, z, mu, rows, cols, rpg, dlv, min_std, eps, ld_eps);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

namespace {
// the sampler on R = B nz rows; noise [R, nd + zd] (never null here); fills every forward field of W
// (toy: R = B q stage rows, z on B q q rows; noise = [eps0: R x nd | eps: R q x zd])
int sampler_fwd(const AuxLayout& P, const AuxPacked& K, const float* params, const float* packed, const float* x, const float* noise, int B,
                int nz_rows, AuxWs& W, hipStream_t st) {
  const int nz = P.stage(nz_rows);               // samples per image at the stage level
  const int R = B * nz, h = P.h, act = P.act, nl = P.nl;
  const int ld0 = P.toy ? P.nd : P.nd + P.zd, lde = P.toy ? P.zd : P.nd + P.zd;
  const float* eps = P.toy ? noise + (size_t)R * P.nd : noise + P.nd;
  if (P.toy) ARDAE_TRY(launch_copy(x, (int64_t)B * P.D, W.xs, st));      // no rescale (models/vae/auxtoy.py: the `x = 2*x - 1` lines are gone)
  else ARDAE_TRY(launch_affine(x, (int64_t)B * P.D, 2.f, -1.f, W.xs, st));
  ARDAE_TRY(K.am.fwd(params, packed, act, B, W.xs, W.e.data(), st));
  ARDAE_TRY(dense_fwd(ACT_NONE, B, P.nd, W.e[nl], h, h, packed + K.mean0_f, params + P.mean0.b, W.mu0, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, B, P.nd, W.e[nl], h, h, packed + K.logvar0_f, params + P.logvar0.b, W.lv0r, st));
  ARDAE_TRY(launch_logvar_clip(W.lv0r, nullptr, W.lv0, (int64_t)B * P.nd, P.clip0, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, B, h, W.xs, P.D, P.D, packed + K.efx_f, params + P.ef[0].b, W.rb, st));   // image half of the first encoder layer (+ its bias)
  ARDAE_TRY(launch_reparam_fwd(W.mu0, W.lv0, noise, ld0, R, P.nd, nz, W.z0, st));
  {  // first encoder layer: the z0 half on the stage rows, the image half as a row bias
    LinArgs A{}; A.Y = W.t[1]; A.ldY = h; A.rowbias = W.rb; A.rowbias_ld = h; A.rows_per_group = nz;
    ARDAE_TRY(lin1(EPI_ACT, act, R, h, W.z0, P.nd, P.nd, packed + K.ef0_f, A, st));
  }
  ARDAE_TRY(K.ef.fwd(params, packed, act, R, W.t[1], W.t.data() + 1, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, R, P.zd, W.t[nl], h, h, packed + K.mean_f, params + P.mean.b, W.mu, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, R, P.zd, W.t[nl], h, h, packed + K.logvar_f, params + P.logvar.b, W.lvr, st));
  ARDAE_TRY(launch_logvar_clip(W.lvr, nullptr, W.lv, (int64_t)R * P.zd, P.clip1, st));
  if (P.toy) return launch_reparam_fwd(W.mu, W.lv, eps, lde, (int64_t)R * nz, P.zd, nz, W.z, st);      // q z's per stage row
  return launch_reparam_fwd(W.mu, W.lv, eps, lde, R, P.zd, 1, W.z, st);
}

// ------------------------------------------------------------------------------------------------ kinds 3 / 7 as a family
// What the shared algorithm (csrc/ipmodel.h) needs to know of the hierarchical MLP models.
struct AuxTraits : IpTraitsBase {
  using Layout = AuxLayout; using Packed = AuxPacked; using Ws = AuxWs; using Entry = AuxEntry;
  [[maybe_unused]] static constexpr bool mlp_decoder = true;
  static int desc_check(const ardae_model_desc* d) { return mlp_desc_check(d, ARDAE_MODEL_CLIP_MASK); }
  static unsigned caps(const ardae_model_desc& d) { return CAP_HIDDEN | (d.kind == 7 ? CAP_GAUSS_DECODER : 0); }
  static IpBufs bufs(const AuxWs& W) { return {W.z, W.D.o[0], W.D.o[1], W.D.dox[0], W.D.dox[1], W.D.dzq, W.D.dz, W.rec_row, W.pri_row}; }
  // every weight-gradient problem of the backward, with its scratch taken from ws
  // (rows: B images, R = B stage(nz) stage rows, N = B nz z / decoder rows; toy: the heads' gradients are the sums over a stage row's q z's)
  static void wgrads(const AuxLayout& P, const AuxPacked& K, const AuxWs& W, const float*, const float*, int B, int nz, WgradList& wl, Bump& ws) {
    const int R = B * P.stage(nz), N = B * nz, h = P.h, nl = P.nl;
    const float* dmu = P.toy ? W.dmu_s : W.D.dz;
    const float* dlv = P.toy ? W.dlv_s : W.dlv;
    K.dec.wgrads(wl, N, W.z, W.D);                                                                     // decoder: head(s), then its layers
    wl.push(R, P.zd, h, dmu, W.t[nl], h, wl.g(P.mean.w), h, wl.g(P.mean.b));
    wl.push(R, P.zd, h, dlv, W.t[nl], h, wl.g(P.logvar.w), h, wl.g(P.logvar.b));
    for (int l = nl; l >= 2; --l) wl.push(R, h, h, W.dt[l], W.t[l - 1], h, wl.g(P.ef[l - 1].w), h, wl.g(P.ef[l - 1].b));   // encoder layers n..2
    wl.push(R, h, P.nd, W.dt[1], W.z0, P.nd, wl.g(P.ef[0].w + P.D), P.ef[0].in, wl.g(P.ef[0].b));        // first encoder layer, z0 half (+ bias)
    wl.push(B, h, P.D, W.drb, W.xs, P.D, wl.g(P.ef[0].w), P.ef[0].in, nullptr);                         // first encoder layer, image half
    wl.push(B, P.nd, h, W.dmu0, W.e[nl], h, wl.g(P.mean0.w), h, wl.g(P.mean0.b));
    wl.push(B, P.nd, h, W.dlv0, W.e[nl], h, wl.g(P.logvar0.w), h, wl.g(P.logvar0.b));
    K.am.wgrads(wl, B, W.xs, W.e.data(), W.de.data());                                                 // aux main
    wl.assign(ws, wgrad_nprob(P));
  }
  static size_t noise_floats(const AuxLayout& P, int B, int nz) { return (size_t)B * P.stage(nz) * P.nd + (size_t)B * nz * P.zd; }
  static float* zero_noise(Entry& e, size_t) { return e.W.zero; }
  static int rows_ok(const AuxLayout& P, int nz, bool encode) {
    if (!P.toy || P.stage(nz) * P.stage(nz) == nz) return 0;
    ARDAE_CHECK_ARG(!encode, "aux_model_encode: ToyAuxIPVAE draws q z0's x q z's per image - nz (%d) must be a square", nz);
    ARDAE_CHECK_ARG(false, "aux_model_vae_forward: ToyAuxIPVAE needs a square nz (got %d)", nz);
    return 0;
  }
  static int sampler_fwd(Entry& e, const float* params, const float* packed, const float* x, const float* noise, int B, int nz, const IpEncodeOut*,
                         hipStream_t st) {
    return ardae::sampler_fwd(e.P, e.K, params, packed, x, noise, B, nz, e.W, st);
  }
  // forward_hidden of the ENCODER (ivae/auxmnist.py:125-132, nz == 1): cat(h0, h)
  static int hidden_copy(Entry& e, float* hidden_out, int B, hipStream_t st) {
    const size_t h = (size_t)e.P.h;
    ARDAE_TRY(launch_copy2d(e.W.e[e.P.nl], h, hidden_out, 2 * h, B, h, st));
    return launch_copy2d(e.W.t[e.P.nl], h, hidden_out + h, 2 * h, B, h, st);
  }
  static int decoder_fwd(Entry& e, const float* params, const float* packed, const float* z, int N, hipStream_t st) {
    return e.K.dec.fwd(params, packed, e.P.act, N, z, e.W.D.hid.data(), e.W.D.o, st);
  }
  static int decoder_bwd(Entry& e, const float* packed, int N, Grads&, hipStream_t st) { return e.K.dec.bwd(packed, e.P.act, N, e.W.D, st); }
  // rows: N = B nz z / decoder rows, R = B nzs stage rows
  static int sampler_bwd(Entry& e, const float*, const float* packed, const float*, const float*, int B, int nz, Grads& g, hipStream_t st) {
    auto& [P, K, ws, W] = e;
    const int N = B * nz;
    const int nzs = P.stage(nz);                            // samples per image at the stage level (toy: q)
    const int R = B * nzs, h = P.h, act = P.act, nl = P.nl;
    // second reparameterisation: dmu = dz, dlv = dz (z - mu) / 2; both heads back into h = t_n
    // (toy: q z's share a stage row's mu / lv: their dz and dlv are summed over the q rows first)
    ARDAE_TRY(launch_reparam_bwd(W.D.dz, W.z, W.mu, N, P.zd, P.toy ? nzs : 1, W.dlv, st));
    const float* dmu = W.D.dz;
    float* dlv = W.dlv;
    if (P.toy) {
      ARDAE_TRY(launch_segment_sum(W.D.dz, P.zd, R, nzs, P.zd, 1.0f, W.dmu_s, P.zd, st));
      ARDAE_TRY(launch_segment_sum(W.dlv, P.zd, R, nzs, P.zd, 1.0f, W.dlv_s, P.zd, st));
      dmu = W.dmu_s; dlv = W.dlv_s;
    }
    // through the z head's log-variance clip: d lv_raw = d lv c'(lv_raw) (in place; one value per stage row)
    ARDAE_TRY(launch_logvar_clip(W.lvr, dlv, dlv, (int64_t)R * P.zd, P.clip1, st));
    ARDAE_TRY(dense_bwd2(act, R, h, dmu, packed + K.mean_b, dlv, packed + K.logvar_b, P.zd, W.t[nl], W.dt[nl], st));
    ARDAE_TRY(K.ef.bwd(packed, act, R, W.t.data() + 1, W.dt.data() + 1, st));                             // dt_n .. dt_2
    if (nl >= 2) ARDAE_TRY(dense_bwd(act, R, h, W.dt[2], h, packed + K.ef.b[0], W.t[1], W.dt[1], st));    // ... and into the first layer's output
    ARDAE_TRY(dense_fwd(ACT_NONE, R, P.nd, W.dt[1], h, h, packed + K.ef0_b, nullptr, W.dz0, st));          // dz0 = dt_1 Wz  (no activation between z0 and the layer)
    ARDAE_TRY(launch_segment_sum(W.dt[1], h, B, nzs, h, 1.0f, W.drb, h, st));
    // first reparameterisation, reduced over the nz samples of each image
    ARDAE_TRY(launch_reparam_bwd(W.dz0, W.z0, W.mu0, R, P.nd, nzs, W.dlv0r, st));
    ARDAE_TRY(launch_segment_sum(W.dz0, P.nd, B, nzs, P.nd, 1.0f, W.dmu0, P.nd, st));
    ARDAE_TRY(launch_segment_sum(W.dlv0r, P.nd, B, nzs, P.nd, 1.0f, W.dlv0, P.nd, st));
    ARDAE_TRY(launch_logvar_clip(W.lv0r, W.dlv0, W.dlv0, (int64_t)B * P.nd, P.clip0, st));      // ... and through the z0 head's
    ARDAE_TRY(dense_bwd2(act, B, h, W.dmu0, packed + K.mean0_b, W.dlv0, packed + K.logvar0_b, P.nd, W.e[nl], W.de[nl], st));
    ARDAE_TRY(K.am.bwd(packed, act, B, W.e.data(), W.de.data(), st));
    // weight gradients: one batched launch
    WgradList wl(g.grads, g.beta);
    wgrads(P, K, W, nullptr, nullptr, B, nz, wl, ws);
    ARDAE_CHECK_ARG(ws.ok, "model_vae_backward: internal workspace accounting error");
    return wl.launch(st);
  }
};

}  // namespace

// (host pass only: a const object with a constant initialiser is otherwise emitted for the device too, where no entry point exists)
#ifndef __HIP_DEVICE_COMPILE__
const Family AUX_FAMILY = ip_family<AuxTraits>();
#endif

}  // namespace ardae
