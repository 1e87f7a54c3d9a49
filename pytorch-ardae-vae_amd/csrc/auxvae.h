// The auxiliary-variable Gaussian baselines of vae.py (ardae_model_desc.kind 14: MNISTAuxVAE `--model auxmnist`, 15: ToyAuxVAE `--model auxtoy`,
// 17: MNISTConvAuxVAE `--model auxconv`, csrc/auxconvvae.hip, 19: MNISTResConvAuxVAE `--model auxresconv`, csrc/auxresvae.hip); csrc/model.hip dispatches
// to the families, the ardae_vae_* entry points of csrc/vaemodel.hip and the two ardae_vae_aux_* entry points of csrc/auxvae.hip through a family's
// GaussFamily row.  What the auxiliary families share is declared here: the row kernels' launchers (csrc/auxvae.hip) and their algorithm - forward,
// backward, encode_stats, the two evaluation passes, the mode-4 workspace - written once over a family's traits.
#pragma once
#include "auxmodel.h"
#include "host_util.h"
#include "vaemodel.h"

namespace ardae {
extern const Family AUXVAE_FAMILY;   // kinds 14 / 15

constexpr int AV_NMAX = 128;       // widest noise_dim (and, in the evaluation, z_dim) the row kernels hold in LDS

// kld[r] (accumulate: +)= KL(N(mu1, exp lv1) || N(mu2, exp lv2)) of row r on [B, n] statistics, n <= AV_NMAX (pair_kld_rows_kernel)
int launch_pair_kld_rows(const float* mu1, const float* lv1, const float* mu2, const float* lv2, int B, int n, float* kld, int accumulate, hipStream_t st);
// the backward seed of the pair KL on n elements (c = loss_scale / B): dmup, dlvp at the auxiliary decoder's head, dmu0, dlv0 at the first head
int launch_pair_kld_seed(const float* mu0, const float* lv0, const float* mup, const float* lvp, int64_t n, float c, DevFloat beta, float* dmup, float* dlvp,
                         float* dmu0, float* dlv0, hipStream_t st);
// the first reparameterisation's part of the first head's seed: dmu0 += dz0;  dlv0 += dz0 (z0 - mu0) / 2
int launch_z0_seed(const float* dz0, const float* z0, const float* mu0, int64_t n, float* dmu0, float* dlv0, hipStream_t st);

// One stage of the evaluation (aux_rows_kernel, csrc/auxvae.hip, where the fields are described)
struct RowsArgs {
  const float *mu, *lv; int rpg;
  const float* eps_in; int ld_eps;
  uint64_t seed, offset, first;
  const float* sample_in;
  int64_t R; int n;
  float *sample_out, *eps_out; int ld_eps_out;
  double* acc; int acc_mode; float* logq;
};
int launch_aux_rows(const RowsArgs& a, hipStream_t st);

inline size_t roundup4(size_t n) { return (n + 3) & ~size_t(3); }

// ------------------------------------------------------------------------------------------------ bodies over an auxiliary family's traits F
// The auxiliary families' algorithm is written once, here; aux_gauss_family<F>() is the family's GaussFamily row.  Beyond what gauss_vae_forward
// needs (csrc/vaemodel.h: open, head_of, hid, bufs, encoder_fwd, decoder_fwd, Grads, grads_of, decoder_bwd), F names
//   P.nd, P.zd, P.h, P.mean / logvar / meanp / logvarp and K.mean_f / logvar_f / meanp_f / logvarp_f      the widths, the z head and the auxiliary decoder's head
//   W.eps0 [B, nd], W.epsz [B, zd], W.kld, W.z, W.rec_row, W.pri_row, out0(W), out1(W)                    the two draws and the rows of a forward
//   W.mu0, lv0, mup, lvp, z0, mu, lv and W.dz0, dmu0, dlv0, dmup, dlvp, dz (the decoder's dz + the auxiliary decoder's)      what the backward's seeds read and write
//   stats_fwd(entry, params, packed, x, B, mu_out, lv_out, st)           x -> (mu0, lv0) of q(z0 | x) on a mode-0 entry (encoder_fwd opens with it on W.mu0, W.lv0)
//   aux_decoder_bwd(entry, packed, B, g, st)                             dmup, dlvp back through the auxiliary decoder: W.dz = the decoder's dz + its z columns', and into the context
//   encode_fc_bwd(entry, packed, B, g, st)                               dmu, dlv back through encode's fc: W.dz0 from its z0 columns, and into the context
//   aux_encoder_bwd(entry, packed, B, g, st)                             dmu0, dlv0 (after any clip's derivative) through the first head, the trunks, and every weight
//                                                                        gradient not launched yet; the families that assign weight-gradient scratch check the arena after it
//   EvalWs : AuxEvalRows, carve_eval(P, K, ws, B, k, W)                  the evaluation pass' buffers (mode 4): the family's own, then W.carve_rows
//   eval_prepare(P, x, B, W, st)                                         what the stages read in place of x
//   eval_hidden(P, K, params, packed, stage, xs, s, B, k, W, st)         stage 2: encode.fc on [. | z0], 3: aux_decode.fc on [. | z]; -> the hidden rows [B k, h]

// the two draws into W.eps0 [B, nd] / W.epsz [B, zd]: the caller's rows [eps0 | eps], or the draws (seed, offset0 [+ state.rng_offset]) from element
// first0 on and (seed, offset1 [+ state.rng_offset]) from element first1 on
template <class Layout, class Ws> int aux_stage_draws(const Layout& P, Ws& W, const float* eps, int B, uint64_t seed, uint64_t offset0, uint64_t first0,
                                                       uint64_t offset1, uint64_t first1, const void* state, hipStream_t st) {
  if (eps) {
    ARDAE_TRY(launch_copy2d(eps, P.nd + P.zd, W.eps0, P.nd, B, P.nd, st));
    return launch_copy2d(eps + P.nd, P.nd + P.zd, W.epsz, P.zd, B, P.zd, st);
  }
  ARDAE_TRY(launch_philox_normal_at(W.eps0, (int64_t)B * P.nd, seed, offset0, state, first0, st));
  return launch_philox_normal_at(W.epsz, (int64_t)B * P.zd, seed, offset1, state, first1, st);
}

// ardae_vae_forward: the two draws go into the workspace first - the caller's rows [eps0 | eps], or elements [0, B nd) and
// [roundup4(B nd), roundup4(B nd) + B zd) of the draw (seed, offset [+ state.rng_offset]) - then the shared algorithm runs on an injected draw.
template <class F> int aux_vae_forward(const ardae_model_desc& d, const float* params, const float* packed, const float* x, const float* eps, int B,
                                       DevFloat beta, uint64_t seed, uint64_t offset, const void* state, float* workspace, size_t wsf, float* z_out,
                                       float* eps_out, float* losses, hipStream_t st) {
  typename F::Entry entry = F::open(d, workspace, wsf, B, 1);
  auto& [P, K, ws, W] = entry;
  ARDAE_CHECK_ARG(ws.ok, "vae_forward: internal workspace accounting error");
  const int ld = P.nd + P.zd;
  ARDAE_TRY(aux_stage_draws(P, W, eps, B, seed, offset, 0, offset, roundup4((size_t)B * P.nd), state, st));
  ARDAE_TRY(gauss_vae_forward<F>(d, params, packed, x, W.epsz, B, beta, seed, offset, state, workspace, wsf, z_out, nullptr, losses, st));
  if (eps_out) {
    ARDAE_TRY(launch_copy2d(W.eps0, P.nd, eps_out, ld, B, P.nd, st));
    ARDAE_TRY(launch_copy2d(W.epsz, P.zd, eps_out + P.nd, ld, B, P.zd, st));
  }
  return 0;
}

// ardae_vae_backward (c = loss_scale / B): every reparameterisation and both KLs in closed form.  The order of the ten steps is written here; what a
// family's networks do between the seeds is in its hooks.
template <class F> int aux_vae_backward(const ardae_model_desc& d, const float* params, const float* packed, const float* x, int B, DevFloat beta,
                                        float loss_scale, float* workspace, size_t wsf, float* grads, float grads_beta, hipStream_t st) {
  typename F::Entry entry = F::open(d, workspace, wsf, B, 1);
  auto& [P, K, ws, W] = entry;
  ARDAE_CHECK_ARG(ws.ok, "vae_backward: internal workspace accounting error");
  const GaussBufs G = F::bufs(W);
  const float c = loss_scale / (float)B;
  const int64_t n0 = (int64_t)B * P.nd;
  typename F::Grads g = F::grads_of(entry, params, packed, grads, grads_beta);
  // reconstruction gradients at the decoder's outputs (beta 0, no seed: dzq gets the zeros of the switched-off energy), the decoder down to G.dz
  ARDAE_TRY(launch_vae_loss(G.out1 ? 1 : 0, G.out0, G.out1, x, W.z, B, 1, d.input_dim, P.zd, 0.f, 1, c, nullptr, G.rec_row, G.pri_row, G.dout0, G.dout1,
                            G.dzq, st));
  ARDAE_TRY(F::decoder_bwd(entry, packed, B, g, st));
  // the pair KL's seed at the auxiliary decoder's head and at the first head; the auxiliary decoder back into its z columns: W.dz = G.dz + its part
  ARDAE_TRY(launch_pair_kld_seed(W.mu0, W.lv0, W.mup, W.lvp, n0, c, beta, W.dmup, W.dlvp, W.dmu0, W.dlv0, st));
  ARDAE_TRY(F::aux_decoder_bwd(entry, packed, B, g, st));
  // the z head's seed, encode's fc back into its z0 columns
  ARDAE_TRY(gauss_head_seed(W.dz, W.z, W.mu, W.lv, (int64_t)B * P.zd, c, beta, G.dmu, G.dlv, st));
  ARDAE_TRY(F::encode_fc_bwd(entry, packed, B, g, st));
  // the first head: the reparameterisation through z0 joins the pair KL's part
  ARDAE_TRY(launch_z0_seed(W.dz0, W.z0, W.mu0, n0, W.dmu0, W.dlv0, st));
  return F::aux_encoder_bwd(entry, packed, B, g, st);
}

// ardae_vae_encode_stats: mu0, lv0 of q(z0 | x), what the evaluation needs first
template <class F> int aux_vae_encode_stats(const ardae_model_desc& d, const float* params, const float* packed, const float* x, int B, float* workspace,
                                            size_t wsf, float* mu_out, float* lv_out, hipStream_t st) {
  typename F::Entry entry = F::open(d, workspace, wsf, B, 0);
  ARDAE_CHECK_ARG(entry.ws.ok, "vae_encode_stats: internal workspace accounting error");
  return F::stats_fwd(entry, params, packed, x, B, mu_out, lv_out, st);
}

// ardae_vae_aux_elbo_rows behind its checks: a forward at beta = 1 that leaves its rows, own draws keyed by the chunk's first image
template <class F> int aux_vae_elbo_rows(const ardae_model_desc& d, const float* params, const float* packed, const float* x, const float* eps, int B,
                                         uint64_t seed, uint64_t offset0, uint64_t offset1, uint64_t first_image, float* workspace, size_t wsf,
                                         float* recon_rows, float* kld_rows, hipStream_t st) {
  typename F::Entry entry = F::open(d, workspace, wsf, B, 1);
  auto& [P, K, ws, W] = entry;
  ARDAE_TRY(aux_stage_draws(P, W, eps, B, seed, offset0, first_image * (uint64_t)P.nd, offset1, first_image * (uint64_t)P.zd, nullptr, st));
  ARDAE_TRY(F::encoder_fwd(entry, params, packed, x, B, st));
  ARDAE_TRY(gauss_head_fwd(F::head_of(P, K), params, packed, F::hid(W), W.epsz, B, seed, 0, nullptr, 0, W.mu, W.lv, W.z, W.eps, kld_rows, st));
  W.kld = kld_rows;      // the pair KL is added into the caller's rows
  ARDAE_TRY(F::decoder_fwd(entry, params, packed, B, st));
  const GaussBufs G = F::bufs(W);
  return launch_vae_loss(G.out1 ? 1 : 0, G.out0, G.out1, x, G.z, B, 1, d.input_dim, P.zd, 0.f, 0, 0.f, nullptr, recon_rows, G.pri_row, nullptr, nullptr, nullptr,
                         st);
}

// The rows every family's evaluation pass (mode 4) ends in, B images x k samples, R = B k: the auxiliary decoder reuses encode.fc's row bias and layer rows
struct AuxEvalRows {
  float *rb, *z0;                            // the row bias [B, h], z0 [R, nd]
  std::vector<float*> t;                     // [1 .. nl]: the layer rows of the stage at hand [R, h]
  float *mu, *lv, *mup, *lvp;
  double* acc;                               // the row's log-density so far [R]
  void carve_rows(Bump& ws, int B, int k, int nd, int zd, int h, int nl) {
    const size_t b = (size_t)B, R = b * (size_t)k;
    rb = ws.take(b * h);
    z0 = ws.take(R * nd);
    t.assign(nl + 1, nullptr);
    for (int l = 1; l <= nl; ++l) t[l] = ws.take(R * h);
    mu = ws.take(R * zd); lv = ws.take(R * zd);
    mup = ws.take(R * nd); lvp = ws.take(R * nd);
    acc = reinterpret_cast<double*>(ws.take(2 * R));
  }
};
// the mode-4 arm of a family's workspace_floats (0: more rows than the row kernels index)
template <class F> size_t aux_eval_floats(const ardae_model_desc& d, int B, int k) {
  if ((int64_t)B * k >= (int64_t)1 << 30) return 0;
  const typename F::Layout P(d);
  Bump ws;
  typename F::EvalWs W;
  F::carve_eval(P, typename F::Packed(P), ws, B, k, W);
  return ws.off;
}
// workspace_floats of a family whose decode-only pass (mode 2, B nz rows) is a mode of its carve - kinds 17 / 19 - as a sizing pass over its entry.
// One draw pair per image; there is no sampler pair.  size_wgrads(entry, B): the weight-gradient scratch the backward assigns after the carve.
template <class F> size_t aux_workspace_floats(const ardae_model_desc& d, int B, int nz, int mode) {
  if (mode == 4) return aux_eval_floats<F>(d, B, nz);
  if (mode != 2 && (nz != 1 || (mode != 0 && mode != 1))) return 0;
  typename F::Entry entry = F::open(d, nullptr, Bump().cap, mode == 2 ? B * nz : B, mode);
  if (mode == 1) F::size_wgrads(entry, B);
  return entry.ws.off;
}

// ardae_vae_aux_iwae_draw behind its checks: the three stochastic stages of logprob on R = B k rows
template <class F> int aux_vae_iwae_draw(const ardae_model_desc& d, const float* params, const float* packed, const float* x, const float* mu0,
                                         const float* lv0, const float* eps, int B, int k, uint64_t seed, uint64_t offset0, uint64_t offset1,
                                         uint64_t first_image, float* workspace, size_t wsf, float* z_out, float* logq, float* eps_out, hipStream_t st) {
  const typename F::Layout P(d);
  const typename F::Packed K(P);
  Bump ws(workspace, wsf);
  typename F::EvalWs W;
  F::carve_eval(P, K, ws, B, k, W);
  ARDAE_CHECK_ARG(ws.ok, "vae_aux_iwae_draw: internal workspace accounting error");
  const int64_t R = (int64_t)B * k;
  const int ld = P.nd + P.zd;
  const float* xs = nullptr;
  ARDAE_TRY(F::eval_prepare(P, x, B, W, xs, st));
  // stage 1: k z0's per image from q(z0 | x), log q(z0 | x)
  RowsArgs a{};
  a.mu = mu0; a.lv = lv0; a.rpg = k; a.eps_in = eps; a.ld_eps = ld; a.seed = seed; a.offset = offset0; a.first = first_image * (uint64_t)k * P.nd;
  a.R = R; a.n = P.nd; a.sample_out = W.z0; a.eps_out = eps_out; a.ld_eps_out = ld; a.acc = W.acc; a.acc_mode = 0;
  ARDAE_TRY(launch_aux_rows(a, st));
  // (the timing tool's per-stage split: ARDAE_AUX_DRAW_STAGES=1 | 2 under ARDAE_DEBUG_KNOBS=1 stops after that stage; logq is then not written)
  int stages = 3;
  if (const char* knob = debug_knob("ARDAE_AUX_DRAW_STAGES")) stages = knob[0] == '1' ? 1 : knob[0] == '2' ? 2 : 3;
  if (stages < 2) return 0;
  // stage 2: encode.fc on [. | z0], one z per row from q(z | z0, x), + log q(z | z0, x)
  const float* hid = nullptr;
  ARDAE_TRY(F::eval_hidden(P, K, params, packed, 2, xs, W.z0, B, k, W, hid, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, (int)R, P.zd, hid, P.h, P.h, packed + K.mean_f, params + P.mean.b, W.mu, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, (int)R, P.zd, hid, P.h, P.h, packed + K.logvar_f, params + P.logvar.b, W.lv, st));
  RowsArgs b{};
  b.mu = W.mu; b.lv = W.lv; b.rpg = 1; b.eps_in = eps ? eps + P.nd : nullptr; b.ld_eps = ld; b.seed = seed; b.offset = offset1;
  b.first = first_image * (uint64_t)k * P.zd; b.R = R; b.n = P.zd; b.sample_out = z_out; b.eps_out = eps_out ? eps_out + P.nd : nullptr;
  b.ld_eps_out = ld; b.acc = W.acc; b.acc_mode = 1;
  ARDAE_TRY(launch_aux_rows(b, st));
  if (stages < 3) return 0;
  // stage 3: aux_decode.fc on [. | z] (in encode.fc's buffers), - log r(z0 | z, x) on the stored z0
  ARDAE_TRY(F::eval_hidden(P, K, params, packed, 3, xs, z_out, B, k, W, hid, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, (int)R, P.nd, hid, P.h, P.h, packed + K.meanp_f, params + P.meanp.b, W.mup, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, (int)R, P.nd, hid, P.h, P.h, packed + K.logvarp_f, params + P.logvarp.b, W.lvp, st));
  RowsArgs r{};
  r.mu = W.mup; r.lv = W.lvp; r.rpg = 1; r.sample_in = W.z0; r.R = R; r.n = P.nd; r.acc = W.acc; r.acc_mode = 2; r.logq = logq;
  return launch_aux_rows(r, st);
}

// the family's row: the bodies above over its traits
template <class F> constexpr GaussFamily aux_gauss_family() {
  return {gauss_vae_head_fused_ok<F>, aux_vae_forward<F>, aux_vae_backward<F>, aux_vae_encode_stats<F>, gauss_vae_head<F>, aux_vae_elbo_rows<F>,
          aux_vae_iwae_draw<F>};
}
}  // namespace ardae
