// The Gaussian-posterior VAE baselines of vae.py (ardae_model_desc.kind 8: MNISTVAE `--model mnist`, 9: ToyVAE `--model toy`, 11: MNISTConvVAE
// `--model conv`, 12: MNISTResConvVAE `--model resconv`).  Their algorithm is written ONCE, here, as templates over a family's traits
// (gauss_vae_forward / _backward / _encode_stats); each family file (csrc/vaemodel.hip: kinds 8 / 9, csrc/convvae.hip, csrc/resvae.hip) supplies
// its traits and one GaussFamily row of the instantiated bodies, which hangs off its Family row (host_util.h).  The ardae_vae_* entry points of
// csrc/vaemodel.hip validate and dispatch through family(d).gauss; they know no family by name.
#pragma once
#include "host_util.h"

namespace ardae {
extern const Family VAE_FAMILY;   // kinds 8 / 9
// encode.reparam.{mean_fn, logvar_fn} [zd, h] on hidden rows [B, h]: the Linears in the parameter buffer, their forward panels, and the family's
// fused form (variant 1) - gauss_head_kernel, or (tail) the two products on the MFMA linears + ONE gauss_head_tail_kernel launch - with
// whether that form is the library's choice (variant 0)
struct GaussHead { int h, zd; Lin mean, logvar; size_t mean_f, logvar_f; bool tail, fused_default; };
// what either fused form can compute at all (1 <= zd <= 64), and where gauss_head_kernel is kinds 8 / 9's default (rows of both matrices on 16 bytes)
bool gauss_head_fused_can(const GaussHead& H);
bool gauss_head_fused_ok(const GaussHead& H);
// mu, lv, z [B, zd], kld [B] (and eps_out: the draw used) from hid [B, h]; variant 0: fused where H.fused_default (unless ARDAE_VAE_HEAD_UNFUSED=1
// under ARDAE_DEBUG_KNOBS=1), 1: H's fused form, 2: the unfused launches.  eps null: element i of the draw (seed, offset [+ state.rng_offset])
int gauss_head_fwd(const GaussHead& H, const float* params, const float* packed, const float* hid, const float* eps, int B, uint64_t seed,
                   uint64_t offset, const void* state, int variant, float* mu, float* lv, float* z, float* eps_out, float* kld, hipStream_t st);
// the backward seed at the head on n = B zd elements: dmu = dz + c beta mu;  dlv = dz (z - mu) / 2 + c beta (exp(lv) - 1) / 2
int gauss_head_seed(const float* dz, const float* z, const float* mu, const float* lv, int64_t n, float c, DevFloat beta, float* dmu, float* dlv,
                    hipStream_t st);
// the Family members that refuse the implicit models' calls (there is no sampler)
int vae_no_encode(const ardae_model_desc&, const float*, const float*, const float*, const float*, int, int, float*, size_t, float*, float*, hipStream_t,
                  const float*);
int vae_no_forward(const ardae_model_desc&, const float*, const float*, const float*, const float*, int, int, DevFloat, float*, size_t, float*, float*,
                   hipStream_t);
int vae_no_backward(const ardae_model_desc&, const float*, const float*, const float*, const float*, int, int, DevFloat, float, const float*, float*,
                    size_t, float*, float, hipStream_t);

// What a Gaussian family adds to its Family row (whose desc_check holds its descriptor rules): the bodies of ardae_vae_head_fused_ok /
// _forward / _backward / _encode_stats / _head, whose arguments the entry points have validated.
struct GaussFamily {
  bool (*head_fused_ok)(const ardae_model_desc& d);
  int (*forward)(const ardae_model_desc& d, const float* params, const float* packed, const float* x, const float* eps, int B, DevFloat beta,
                 uint64_t seed, uint64_t offset, const void* state, float* workspace, size_t wsf, float* z_out, float* eps_out, float* losses,
                 hipStream_t st);
  int (*backward)(const ardae_model_desc& d, const float* params, const float* packed, const float* x, int B, DevFloat beta, float loss_scale,
                  float* workspace, size_t wsf, float* grads, float grads_beta, hipStream_t st);
  int (*encode_stats)(const ardae_model_desc& d, const float* params, const float* packed, const float* x, int B, float* workspace, size_t wsf,
                      float* mu_out, float* lv_out, hipStream_t st);
  int (*head)(const ardae_model_desc& d, const float* params, const float* packed, const float* hid, const float* eps, int B, uint64_t seed,
              uint64_t offset, const void* state, int variant, float* mu, float* lv, float* z, float* eps_out, float* kld, hipStream_t st);
  // the auxiliary-variable families only (kinds 14 / 15 / 17; null elsewhere): the bodies of ardae_vae_aux_elbo_rows / ardae_vae_aux_iwae_draw
  int (*aux_elbo_rows)(const ardae_model_desc& d, const float* params, const float* packed, const float* x, const float* eps, int B, uint64_t seed,
                       uint64_t offset0, uint64_t offset1, uint64_t first_image, float* workspace, size_t wsf, float* recon_rows, float* kld_rows,
                       hipStream_t st);
  int (*aux_iwae_draw)(const ardae_model_desc& d, const float* params, const float* packed, const float* x, const float* mu0, const float* lv0,
                       const float* eps, int B, int k, uint64_t seed, uint64_t offset0, uint64_t offset1, uint64_t first_image, float* workspace,
                       size_t wsf, float* z_out, float* logq, float* eps_out, hipStream_t st);
};

// The buffers of a family's workspace that the shared algorithm names (out1 / dout1: the second head of a Gaussian decoder - kind 9 - else null; dzq: the
// part of dL/dz the loss kernel writes, dz: dL/dz after the decoder's backward - the same buffer where that backward accumulates in place)
struct GaussBufs { float *mu, *lv, *z, *eps, *kld, *rec_row, *pri_row, *out0, *out1, *dout0, *dout1, *dzq, *dz, *dmu, *dlv; };

// A family's traits F:
//   Entry, Layout, Packed    its Entry<Layout, Packed, Ws>; open(d, workspace, wsf, B, mode) carves it (mode 0: the encoder only, 1: everything)
//   head_of(P, K)            the GaussHead;   hid(W): the hidden rows it reads;   bufs(W): the GaussBufs (mode 1)
//   encoder_fwd(entry, params, packed, x, B, st), decoder_fwd(entry, params, packed, B, st): x -> hid, z -> out0 (, out1)
//   Grads, grads_of(entry, params, packed, grads, grads_beta): what its backward halves share (kind 12: the GradMap)
//   decoder_bwd(entry, packed, B, g, st): dout -> dz;   encoder_bwd(entry, packed, x, B, g, st): the head's backward-data from dmu, dlv into the
//                            hidden rows, the encoder's backward, and every weight gradient not launched yet
template <class F> int gauss_vae_forward(const ardae_model_desc& d, const float* params, const float* packed, const float* x, const float* eps, int B,
                                         DevFloat beta, uint64_t seed, uint64_t offset, const void* state, float* workspace, size_t wsf, float* z_out,
                                         float* eps_out, float* losses, hipStream_t st) {
  typename F::Entry entry = F::open(d, workspace, wsf, B, 1);
  auto& [P, K, ws, W] = entry;
  ARDAE_CHECK_ARG(ws.ok, "vae_forward: internal workspace accounting error");
  const GaussBufs G = F::bufs(W);
  const int64_t n = (int64_t)B * d.z_dim;
  ARDAE_TRY(F::encoder_fwd(entry, params, packed, x, B, st));
  ARDAE_TRY(gauss_head_fwd(F::head_of(P, K), params, packed, F::hid(W), eps, B, seed, offset, state, 0, G.mu, G.lv, G.z, G.eps, G.kld, st));
  ARDAE_TRY(F::decoder_fwd(entry, params, packed, B, st));
  // the row reconstruction loss (the N(0, I) energy this kernel also knows is switched off: beta 0; pri_row is its unused output)
  ARDAE_TRY(launch_vae_loss(G.out1 ? 1 : 0, G.out0, G.out1, x, G.z, B, 1, d.input_dim, d.z_dim, 0.f, 0, 0.f, nullptr, G.rec_row, G.pri_row, nullptr,
                            nullptr, nullptr, st));
  ARDAE_TRY(launch_vae_loss_finalize(G.rec_row, G.kld, B, beta, losses, st));
  ARDAE_TRY(launch_copy(G.z, n, z_out, st));
  if (eps_out) ARDAE_TRY(launch_copy(G.eps, n, eps_out, st));
  return 0;
}

// (the arena check sits where each family had it: kind 12, whose scratch is carved up front, checks here and nowhere else; kinds 8 / 9 / 11 check
// again in encoder_bwd, after their weight-gradient scratch is assigned.  For them the check here is new but unobservable: Bump::ok never turns
// true again, so it fails only where the later one fails, with the same message - and the entry point has sized the arena with the same code.)
template <class F> int gauss_vae_backward(const ardae_model_desc& d, const float* params, const float* packed, const float* x, int B, DevFloat beta,
                                          float loss_scale, float* workspace, size_t wsf, float* grads, float grads_beta, hipStream_t st) {
  typename F::Entry entry = F::open(d, workspace, wsf, B, 1);
  auto& [P, K, ws, W] = entry;
  ARDAE_CHECK_ARG(ws.ok, "vae_backward: internal workspace accounting error");
  const GaussBufs G = F::bufs(W);
  const float c = loss_scale / (float)B;
  typename F::Grads g = F::grads_of(entry, params, packed, grads, grads_beta);
  // reconstruction gradients at the decoder's outputs (beta 0, no seed: dzq gets the zeros of the switched-off energy)
  ARDAE_TRY(launch_vae_loss(G.out1 ? 1 : 0, G.out0, G.out1, x, G.z, B, 1, d.input_dim, d.z_dim, 0.f, 1, c, nullptr, G.rec_row, G.pri_row, G.dout0,
                            G.dout1, G.dzq, st));
  ARDAE_TRY(F::decoder_bwd(entry, packed, B, g, st));
  ARDAE_TRY(gauss_head_seed(G.dz, G.z, G.mu, G.lv, (int64_t)B * d.z_dim, c, beta, G.dmu, G.dlv, st));
  return F::encoder_bwd(entry, packed, x, B, g, st);
}

template <class F> int gauss_vae_encode_stats(const ardae_model_desc& d, const float* params, const float* packed, const float* x, int B,
                                              float* workspace, size_t wsf, float* mu_out, float* lv_out, hipStream_t st) {
  typename F::Entry entry = F::open(d, workspace, wsf, B, 0);
  ARDAE_CHECK_ARG(entry.ws.ok, "vae_encode_stats: internal workspace accounting error");
  ARDAE_TRY(F::encoder_fwd(entry, params, packed, x, B, st));
  // the two heads write the caller's buffers themselves: no draw, no sample
  const GaussHead H = F::head_of(entry.P, entry.K);
  ARDAE_TRY(dense_fwd(ACT_NONE, B, H.zd, F::hid(entry.W), H.h, H.h, packed + H.mean_f, params + H.mean.b, mu_out, st));
  return dense_fwd(ACT_NONE, B, H.zd, F::hid(entry.W), H.h, H.h, packed + H.logvar_f, params + H.logvar.b, lv_out, st);
}

template <class F> GaussHead gauss_head_of(const ardae_model_desc& d) {
  const typename F::Layout P(d);
  return F::head_of(P, typename F::Packed(P));
}
template <class F> bool gauss_vae_head_fused_ok(const ardae_model_desc& d) { return gauss_head_of<F>(d).fused_default; }
template <class F> int gauss_vae_head(const ardae_model_desc& d, const float* params, const float* packed, const float* hid, const float* eps, int B,
                                      uint64_t seed, uint64_t offset, const void* state, int variant, float* mu, float* lv, float* z, float* eps_out,
                                      float* kld, hipStream_t st) {
  return gauss_head_fwd(gauss_head_of<F>(d), params, packed, hid, eps, B, seed, offset, state, variant, mu, lv, z, eps_out, kld, st);
}

// the family's row: the bodies above over its traits
template <class F> constexpr GaussFamily gauss_family() {
  return {gauss_vae_head_fused_ok<F>, gauss_vae_forward<F>, gauss_vae_backward<F>, gauss_vae_encode_stats<F>, gauss_vae_head<F>, nullptr, nullptr};
}
}  // namespace ardae
