// The conv Gaussian-posterior baseline (vae.py --model conv; ardae_model_desc.kind 11: models/vae/conv.py::VAE), joined from pieces the other
// families own - no kernel of its own, and of the algorithm only what ConvVaeTraits says (the rest is csrc/vaemodel.h's, shared by every Gaussian kind):
//
//   per image (B rows):  x2 = 2x - 1;  h3 = trunk(x2) (conv 1 -> 16 -> 32 -> 32, k5 s2 p2: csrc/convmodel.hip);  hid = act(F h3 + f)  [B, 800]
//                        mu, lv, z, kld: the Gaussian head on hid - two MFMA linears and one tail launch (gauss_head_fwd's tail form,
//                        csrc/vaemodel.hip: the draw keying and the KL in double of kinds 8 / 9)
//                        logit = Decoder(z) (models/vae/conv.py:79-136, the decoder of kinds 2 / 4);  recon = BCE-with-logits over 784 pixels
//   losses = {mean_b(recon_b + beta kld_b), mean recon, mean kld}    (vae/conv.py:170-201)
// Backward (c = loss_scale / B): the reconstruction seed, the decoder down to dz, the head's closed form (dmu, dlv), both heads back into
// hid, fc, the trunk; every weight gradient - the decoder's eight, the two heads, fc, the three convs - in one batch.
#include "ardae_hip.h"
#include "common.h"
#include "convmodel.h"
#include "convvae.h"
#include "vaemodel.h"

namespace ardae {
namespace {

struct ConvVaeLayout {
  int zd, act;
  Lin conv[3], fc, mean, logvar;   // encode.conv{1,2,3}, encode.fc [800, 512], encode.reparam.{mean_fn, logvar_fn} [zd, 800]
  ConvDecLayout dec;
  size_t total;
  explicit ConvVaeLayout(const ardae_model_desc& d) : zd(d.z_dim), act(d.act) {
    size_t off = 0;
    trunk_lins(off, conv);
    fc = next_lin(off, 800, 512); mean = next_lin(off, zd, 800); logvar = next_lin(off, zd, 800);
    dec = ConvDecLayout(zd, act, off);
    total = off;
  }
};

struct ConvVaePacked {
  size_t conv_f[3], conv_b[3], fc_f, fc_b, mean_f, mean_b, logvar_f, logvar_b;
  ConvDecPacked dec;
  ConvVaePacked(const ConvVaeLayout& P, PackList& pl) {
    trunk_panels(P.conv, pl, conv_f, conv_b);
    pl.pair(P.fc, fc_f, fc_b); pl.pair(P.mean, mean_f, mean_b); pl.pair(P.logvar, logvar_f, logvar_b);
    dec = ConvDecPacked(P.dec, pl);
  }
  explicit ConvVaePacked(const ConvVaeLayout& P, PackList&& sizing = PackList()) : ConvVaePacked(P, sizing) {}   // offsets only
};

struct ConvVaeWs {
  float* x2; TrunkBuf T; TrunkScratch S;
  float *hid, *mu, *lv, *z, *eps, *kld, *dmu, *dlv, *dhid;      // hid [B, 800] = act(fc(h3))
  ConvDecWs D;
};

// mode 0: the encoder up to hid (encode_stats writes mu, lv to the caller); 1: forward + backward; 2: the decoder's forward on B rows of z
void carve(const ConvVaeLayout& P, const ConvVaePacked&, Bump& ws, int B, int mode, ConvVaeWs& W) {
  const size_t b = (size_t)B;
  if (mode == 2) return conv_decoder_carve(ws, b, P.zd, CONV_DEC_DECODE, W.D);
  W.x2 = ws.take(b * 784);
  trunk_carve(ws, b, W.T);
  W.hid = ws.take(b * 800);
  if (mode == 0) return;
  W.mu = ws.take(b * P.zd); W.lv = ws.take(b * P.zd); W.z = ws.take(b * P.zd); W.eps = ws.take(b * P.zd); W.kld = ws.take(b);
  conv_decoder_carve(ws, b, P.zd, CONV_DEC_TRAIN, W.D);
  W.dmu = ws.take(b * P.zd); W.dlv = ws.take(b * P.zd); W.dhid = ws.take(b * 800);
  trunk_bwd_carve(ws, b, W.T, &W.S);
}
using ConvVaeEntry = Entry<ConvVaeLayout, ConvVaePacked, ConvVaeWs>;

// every weight-gradient problem of the backward: the decoder's eight, the two heads, fc, the three convs
void convvae_wgrads(const ConvVaeLayout& P, const ConvVaeWs& W, int B, WgradList& wl, Bump& ws) {
  conv_decoder_wgrads(P.dec, W.D, W.z, B, wl);
  wl.push(B, P.zd, 800, W.dmu, W.hid, 800, wl.g(P.mean.w), 800, wl.g(P.mean.b));
  wl.push(B, P.zd, 800, W.dlv, W.hid, 800, wl.g(P.logvar.w), 800, wl.g(P.logvar.b));
  wl.push(B, 800, 512, W.dhid, W.T.inp, 512, wl.g(P.fc.w), 512, wl.g(P.fc.b));
  conv_trunk_wgrads(P.conv, W.T, B, wl);
  wl.assign(ws, CONV_WGRAD_HINT);
}

size_t convvae_workspace_floats(const ardae_model_desc& d, int B, int nz, int mode) {
  if (mode != 2 && (nz != 1 || mode == 3)) return 0;         // one draw per image; there is no sampler pair
  const ConvVaeLayout P(d);
  Bump ws;
  ConvVaeWs W;
  carve(P, ConvVaePacked(P), ws, mode == 2 ? B * nz : B, mode, W);
  if (mode == 1) {
    WgradList wl(nullptr);
    convvae_wgrads(P, W, B, wl, ws);
  }
  return ws.off;
}

int convvae_decode(const ardae_model_desc& d, const float* params, const float* packed, const float* z, int R, float* workspace, size_t wsf, float* out0,
                   hipStream_t st, float*) {
  ConvVaeEntry entry(d, workspace, wsf, R, 2);
  auto& [P, K, ws, W] = entry;
  ARDAE_CHECK_ARG(ws.ok, "model_decode: workspace too small");
  ARDAE_TRY(conv_decode_fwd(P.dec, K.dec, params, packed, z, R, W.D, st));
  return launch_copy(W.D.logit, (int64_t)R * 784, out0, st);
}

// the descriptor rules of kind 11 (input_dim 784, h_dim 800, n_layers 1, noise_dim 0, flags 0, z_dim >= 1, any activation but NONE)
int convvae_desc_check(const ardae_model_desc* d) {
  ARDAE_CHECK_ARG(d->noise_dim == 0, "model: noise_dim must be 0 for kind 11 (the Gaussian posterior takes no noise input), got %d", d->noise_dim);
  ARDAE_CHECK_ARG(d->flags == 0, "model: flags must be 0 for kind 11, got %d", d->flags);
  return conv_gauss_desc_check(d, "MNISTConvVAE", "the width of encode.fc");
}

// What gauss_vae_forward / _backward / _encode_stats (csrc/vaemodel.h) need to know of this family.
struct ConvVaeTraits {
  using Layout = ConvVaeLayout; using Packed = ConvVaePacked; using Entry = ConvVaeEntry;
  struct Grads { float* grads; float beta; };
  static Entry open(const ardae_model_desc& d, float* workspace, size_t wsf, int B, int mode) { return Entry(d, workspace, wsf, B, mode); }
  // The head at h = 800.  gauss_head_kernel (one serial 800-long FMA chain per output, 16 workgroups at 128 rows) loses here: 51.0 us against
  // 19.8 us for the five unfused launches at 128 x 800 -> 2 x 32.  So this family's fused form is the tail form: the two
  // products stay on the MFMA linears and what is left - the draw, the reparameterisation and the KL rows - is ONE launch: three launches in place
  // of five, and bit for bit the unfused head's outputs, whose launches and expressions it shares.  Where it is the default: z <= 64 (the tail's LDS).
  static GaussHead head_of(const ConvVaeLayout& P, const ConvVaePacked& K) {
    return GaussHead{800, P.zd, P.mean, P.logvar, K.mean_f, K.logvar_f, true, P.zd >= 1 && P.zd <= 64};
  }
  static const float* hid(const ConvVaeWs& W) { return W.hid; }
  static GaussBufs bufs(const ConvVaeWs& W) {
    const ConvDecWs& D = W.D;
    return {W.mu, W.lv, W.z, W.eps, W.kld, D.rec_row, D.pri_row, D.logit, nullptr, D.dlogit, nullptr, D.dzq, D.dz, W.dmu, W.dlv};
  }
  // x2 = 2x - 1, the trunk, hid = act(fc(h3))
  static int encoder_fwd(Entry& e, const float* params, const float* packed, const float* x, int B, hipStream_t st) {
    auto& [P, K, ws, W] = e;
    ARDAE_TRY(launch_affine(x, (int64_t)B * 784, 2.f, -1.f, W.x2, st));           // vae/conv.py:64
    ARDAE_TRY(trunk_fwd(P.conv, K.conv_f, params, packed, W.x2, W.T, B, P.act, st));
    return dense_fwd(P.act, B, 800, W.T.inp, 512, 512, packed + K.fc_f, params + P.fc.b, W.hid, st);
  }
  static int decoder_fwd(Entry& e, const float* params, const float* packed, int B, hipStream_t st) {
    return conv_decode_fwd(e.P.dec, e.K.dec, params, packed, e.W.z, B, e.W.D, st);
  }
  static Grads grads_of(Entry&, const float*, const float*, float* grads, float grads_beta) { return {grads, grads_beta}; }
  static int decoder_bwd(Entry& e, const float* packed, int B, Grads&, hipStream_t st) { return conv_decoder_bwd(e.P.dec, e.K.dec, packed, e.W.D, B, st); }
  static int encoder_bwd(Entry& e, const float* packed, const float*, int B, Grads& g, hipStream_t st) {
    auto& [P, K, ws, W] = e;
    ARDAE_TRY(dense_bwd2(P.act, B, 800, W.dmu, packed + K.mean_b, W.dlv, packed + K.logvar_b, P.zd, W.hid, W.dhid, st));
    ARDAE_TRY(dense_fwd(ACT_NONE, B, 512, W.dhid, 800, 800, packed + K.fc_b, nullptr, W.T.dinp, st));   // fc backward-data; the trunk applies conv3's act'
    ARDAE_TRY(trunk_bwd(K.conv_b, packed, W.T, W.S, B, P.act, st));
    WgradList wl(g.grads, g.beta);
    convvae_wgrads(P, W, B, wl, ws);
    ARDAE_CHECK_ARG(ws.ok, "vae_backward: internal workspace accounting error");
    return wl.launch(st);
  }
};

}  // namespace

// (host pass only, as in csrc/auxmodel.hip)
#ifndef __HIP_DEVICE_COMPILE__
static const GaussFamily CONVVAE_GAUSS = gauss_family<ConvVaeTraits>();
const Family CONVVAE_FAMILY = {convvae_desc_check, no_caps, family_param_floats<ConvVaeLayout, ConvVaePacked>, family_packed_floats<ConvVaeLayout, ConvVaePacked>,
                               convvae_workspace_floats, family_pack<ConvVaeLayout, ConvVaePacked>, vae_no_encode, convvae_decode, vae_no_forward,
                               vae_no_backward, &CONVVAE_GAUSS};
#endif

}  // namespace ardae
