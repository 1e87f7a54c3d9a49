// The implicit-posterior VAEs (ardae_model_desc.kind 0 - 7: a sampler z = f(x, noise) on R = B nz rows, a decoder, the ELBO pieces).  Their algorithm
// is written ONCE, here, as templates over a family's traits (ip_workspace_floats / ip_encode / ip_decode / ip_vae_forward / ip_vae_backward and its two
// halves); each family file (csrc/model.hip: kinds 0 / 1, csrc/convmodel.hip: 2, csrc/auxconvmodel.hip: 4, csrc/auxmodel.hip: 3 / 7, csrc/resmodel.hip: 5 / 6) supplies
// its traits and exports one Family row (host_util.h) built by ip_family<F>().  csrc/vaemodel.h is the same for the Gaussian-posterior kinds.
//
// The internal arena checks (`ws.ok`) of these bodies carry one text each.  They cannot fire through the ABI: the entry point has sized the arena with
// ip_workspace_floats<F>, which runs the same carve and the same weight-gradient list on a null arena.
#pragma once
#include "host_util.h"
#include "mlp.h"

namespace ardae {

// The buffers of a family's workspace that the shared algorithm names (mode 1).  out1 / dout1: the second head of a Gaussian decoder, else null;
// dzq: the part of dL/dz the loss kernel writes (prior + injected seed); dz: dL/dz after the decoder's backward - dzq itself where that backward
// accumulates in place
struct IpBufs { float *z, *out0, *out1, *dout0, *dout1, *dzq, *dz, *rec_row, *pri_row; };

// What a forward-only sampler pass (ip_encode) hands the family's sampler_fwd; a training forward passes null and keeps every hidden row.
//   z_out       where z goes when the family writes the caller's buffer itself (F::direct_z: one launch less); else z stays in the workspace
//   hidden_out  the hidden context is wanted (ip_encode copies it through F::hidden_copy, unless the family's sampler does so in passing)
//   raw0, std0  kind 6's clipped class: the unscaled eps0 of a std = 0 pass, and whether this is one (the caller's noise was null)
struct IpEncodeOut { float* z_out; float* hidden_out; const float* raw0; bool std0; };

// What a family's traits may leave at these defaults
struct IpTraitsBase {
  static constexpr bool mlp_decoder = false;    // its Packed holds an MlpDecoder `dec`: mode 2 is that decoder's own sizing (mlp.h::mlp_decode)
  static constexpr bool direct_z = false;
  struct Grads { float* grads; float beta; };   // what the two halves of the backward share
  template <class Entry> static Grads grads_of(Entry&, const float*, const float*, float* grads, float grads_beta) { return {grads, grads_beta}; }
  template <class Layout> static size_t extra_floats(const Layout&, int, int, int) { return 0; }
  template <class Layout> static int rows_ok(const Layout&, int, bool) { return 0; }
  template <class Entry> static int hidden_copy(Entry&, float*, int, hipStream_t) { return 0; }
};

// A family's traits F (: IpTraitsBase):
//   Layout, Packed, Ws, Entry  its Entry<Layout, Packed, Ws>, carved by carve(P, K, ws, B, nz, mode, W) (mode 0: the sampler only, 1: everything,
//                              2: decode only on B rows)
//   desc_check(d), caps(d)     the Family row's
//   bufs(W)                    the IpBufs
//   wgrads(P, K, W, x, noise, B, nz, wl, ws)   the weight-gradient list with its scratch assigned (a sizing pass: null buffers), where the family has one
//   extra_floats(P, B, nz, mode)   what the family's arena holds beside the carve (mode as the caller gave it: 3 = encode_pair)
//   noise_floats(P, B, nz), zero_noise(entry, n)   the size of a call's noise, and the n zeros that stand in for a null one
//   rows_ok(P, nz, encode)     the family's rule on nz (kind 7: a square)
//   sampler_fwd(entry, params, packed, x, noise, B, nz, enc, st)   x, noise -> z (enc: the IpEncodeOut of a forward-only pass, else null)
//   hidden_copy(entry, hidden_out, B, st)   the hidden context of an nz = 1 pass
//   decoder_fwd(entry, params, packed, z, R, st)   z -> out0 (, out1), every hidden row kept where the arena has room for it
//   grads_of(entry, params, packed, grads, grads_beta)   F::Grads (kinds 5 / 6: the GradMap)
//   decoder_bwd(entry, packed, R, g, st)   dout0 (, dout1), dzq -> dz
//   sampler_bwd(entry, params, packed, x, noise, B, nz, g, st)   dz -> the sampler's backward, and every weight gradient not launched yet
template <class F> size_t ip_workspace_floats(const ardae_model_desc& d, int B, int nz, int mode) {
  const typename F::Layout P(d);
  const typename F::Packed K(P);
  if constexpr (F::mlp_decoder)
    if (mode == 2) return K.dec.decode_floats((size_t)B * nz);
  const int m = mode == 3 ? 0 : mode;      // encode_pair runs on the sampler's buffers (plus the family's extra)
  Bump ws;
  typename F::Ws W{};
  carve(P, K, ws, B, nz, m, W);
  if (m == 1) {
    WgradList wl(nullptr);
    F::wgrads(P, K, W, nullptr, nullptr, B, nz, wl, ws);
  }
  return ws.off + F::extra_floats(P, B, nz, mode);
}

template <class F> int ip_encode(const ardae_model_desc& d, const float* params, const float* packed, const float* x, const float* noise, int B, int nz,
                                 float* workspace, size_t wsf, float* z_out, float* hidden_out, hipStream_t st, const float* raw0) {
  typename F::Entry entry(d, workspace, wsf, B, nz, 0);
  auto& [P, K, ws, W] = entry;
  const size_t nn = F::noise_floats(P, B, nz);
  float* zero = noise ? nullptr : F::zero_noise(entry, nn);
  ARDAE_CHECK_ARG(ws.ok, "model_encode: internal workspace accounting error");
  ARDAE_TRY(F::rows_ok(P, nz, true));
  ARDAE_CHECK_ARG(!hidden_out || nz == 1, "model_encode: the hidden context is defined for nz == 1");
  const IpEncodeOut enc{z_out, hidden_out, raw0, noise == nullptr};
  ARDAE_TRY(noise_or_zero(noise, zero, nn, st));
  ARDAE_TRY(F::sampler_fwd(entry, params, packed, x, noise, B, nz, &enc, st));
  if (z_out && !F::direct_z) ARDAE_TRY(launch_copy(F::bufs(W).z, (size_t)B * nz * d.z_dim, z_out, st));
  if (hidden_out) ARDAE_TRY(F::hidden_copy(entry, hidden_out, B, st));
  return 0;
}

// out0 (, out1) [R, input_dim] from z [R, z_dim]: the family's decoder forward in a decode-only arena, then its output copied out
template <class F> int ip_decode(const ardae_model_desc& d, const float* params, const float* packed, const float* z, int R, float* workspace, size_t wsf,
                                 float* out0, hipStream_t st, float*) {
  typename F::Entry entry(d, workspace, wsf, R, 1, 2);
  ARDAE_CHECK_ARG(entry.ws.ok, "model_decode: internal workspace accounting error");
  ARDAE_TRY(F::decoder_fwd(entry, params, packed, z, R, st));
  return launch_copy(F::bufs(entry.W).out0, (size_t)R * d.input_dim, out0, st);
}

template <class F> int ip_vae_forward(const ardae_model_desc& d, const float* params, const float* packed, const float* x, const float* noise, int B, int nz,
                                      DevFloat beta, float* workspace, size_t wsf, float* z_out, float* losses, hipStream_t st) {
  typename F::Entry entry(d, workspace, wsf, B, nz, 1);
  auto& [P, K, ws, W] = entry;
  ARDAE_CHECK_ARG(ws.ok, "model_vae_forward: internal workspace accounting error");
  ARDAE_TRY(F::rows_ok(P, nz, false));
  const IpBufs G = F::bufs(W);
  const int R = B * nz;
  ARDAE_TRY(F::sampler_fwd(entry, params, packed, x, noise, B, nz, nullptr, st));
  ARDAE_TRY(launch_copy(G.z, (size_t)R * d.z_dim, z_out, st));
  ARDAE_TRY(F::decoder_fwd(entry, params, packed, G.z, R, st));
  ARDAE_TRY(launch_vae_loss(G.out1 ? 1 : 0, G.out0, G.out1, x, G.z, R, nz, d.input_dim, d.z_dim, beta, 0, 0.f, nullptr, G.rec_row, G.pri_row, nullptr,
                            nullptr, nullptr, st));
  return launch_vae_loss_finalize(G.rec_row, G.pri_row, R, beta, losses, st);
}

// The backward in two halves.  phases & 1: the loss gradients (gscale = dloss / R) and the decoder's backward up to dz - it needs nothing from the cDAE;
// phases & 2: the sampler's backward and the weight gradients.  The entropy seed dz_extra (or null) enters pre-scaled through the loss kernel where one
// call runs both halves (phases 3), and is added to dz as seed_scale * dz_extra where the second half is a call of its own (phases 2).
template <class F> int ip_backward(const ardae_model_desc& d, const float* params, const float* packed, const float* x, const float* noise, int B, int nz,
                                   DevFloat beta, float dloss, const float* dz_extra, DevFloat seed_scale, float* workspace, size_t wsf, float* grads,
                                   float grads_beta, int phases, hipStream_t st) {
  typename F::Entry entry(d, workspace, wsf, B, nz, 1);
  ARDAE_CHECK_ARG(entry.ws.ok, "model_vae_backward: internal workspace accounting error");
  typename F::Grads g = F::grads_of(entry, params, packed, grads, grads_beta);
  const IpBufs G = F::bufs(entry.W);
  const int R = B * nz;
  if (phases & 1) {
    ARDAE_TRY(launch_vae_loss(G.out1 ? 1 : 0, G.out0, G.out1, x, G.z, R, nz, d.input_dim, d.z_dim, beta, 1, dloss / (float)R,
                              phases == 3 ? dz_extra : nullptr, G.rec_row, G.pri_row, G.dout0, G.dout1, G.dzq, st));
    ARDAE_TRY(F::decoder_bwd(entry, packed, R, g, st));
  }
  if (!(phases & 2)) return 0;
  if (phases == 2 && dz_extra) ARDAE_TRY(launch_axpy(dz_extra, (int64_t)R * d.z_dim, seed_scale, G.dz, st));
  return F::sampler_bwd(entry, params, packed, x, noise, B, nz, g, st);
}
// Family::vae_backward, and the halves as Family::vae_backward_decoder / _sampler
template <class F> int ip_vae_backward(const ardae_model_desc& d, const float* params, const float* packed, const float* x, const float* noise, int B,
                                       int nz, DevFloat beta, float dloss, const float* dz_extra, float* workspace, size_t wsf, float* grads,
                                       float grads_beta, hipStream_t st) {
  return ip_backward<F>(d, params, packed, x, noise, B, nz, beta, dloss, dz_extra, 1.f, workspace, wsf, grads, grads_beta, 3, st);
}
template <class F> int ip_vae_backward_decoder(const ardae_model_desc& d, const float* params, const float* packed, const float* x, const float* noise,
                                               int B, int nz, DevFloat beta, float dloss, float* workspace, size_t wsf, hipStream_t st) {
  return ip_backward<F>(d, params, packed, x, noise, B, nz, beta, dloss, nullptr, 0.f, workspace, wsf, nullptr, 0.f, 1, st);
}
template <class F> int ip_vae_backward_sampler(const ardae_model_desc& d, const float* params, const float* packed, const float* x, const float* noise,
                                               int B, int nz, const float* dz_extra, DevFloat seed_scale, float* workspace, size_t wsf, float* grads,
                                               float grads_beta, hipStream_t st) {
  return ip_backward<F>(d, params, packed, x, noise, B, nz, 0.f, 0.f, dz_extra, seed_scale, workspace, wsf, grads, grads_beta, 2, st);
}

// the family's row: its rules and the bodies above over its traits (pack: where the pack launch is not all a family's pack does)
template <class F> constexpr Family ip_family(int (*pack)(const ardae_model_desc&, const float*, float*, hipStream_t) =
                                                  family_pack<typename F::Layout, typename F::Packed>) {
  Family f{};
  f.desc_check = F::desc_check; f.caps = F::caps;
  f.param_floats = family_param_floats<typename F::Layout, typename F::Packed>;
  f.packed_floats = family_packed_floats<typename F::Layout, typename F::Packed>;
  f.workspace_floats = ip_workspace_floats<F>; f.pack = pack; f.encode = ip_encode<F>;
  if constexpr (F::mlp_decoder) f.decode = mlp_decode<typename F::Layout, typename F::Packed>;
  else f.decode = ip_decode<F>;
  f.vae_forward = ip_vae_forward<F>; f.vae_backward = ip_vae_backward<F>;
  return f;
}
}  // namespace ardae
