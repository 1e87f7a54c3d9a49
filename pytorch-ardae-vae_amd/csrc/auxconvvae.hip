// The hierarchical conv Gaussian baseline (vae.py --model auxconv; ardae_model_desc.kind 17: models/vae/auxconv.py::VAE, the "# hierarchical conv"
// baseline of run_vae_dbmnist.sh) - the Gaussian counterpart of kind 4, joined from pieces the other families own: the conv trunk and the decoder of
// csrc/convmodel.h, the Gaussian head (csrc/vaemodel.h), the pair KL, its seed and the evaluation's row kernel (csrc/auxvae.hip).
//
//   per image (B rows):  x2 = 2x - 1; three trunks (conv 1 -> 16 -> 32 -> 32, k5 s2 p2) on the SAME x2, each with its own weights, one im2col of x2
//     aux_encode   h3a = trunk_a(x2);  h4a = act(Fa h3a + fa)  [B, 800];  mu0 = M0 h4a + m0;  lv0 = L0 h4a + l0 (no clip);  z0 = mu0 + exp(lv0 / 2) eps0
//     encode       h4 = act(Fe [h3e | z0] + fe);  mu, lv, z, kld: the Gaussian head on h4 (kind 11's policy: the tail form)
//     aux_decode   h4r = act(Fr [h3r | z] + fr);  mup = Mp h4r + mp;  lvp = Lp h4r + lp;  aux_kld = KL(N(mu0, exp lv0) || N(mup, exp lvp)), added into kld
//     decode       kind 11's decoder (models/vae/conv.py::Decoder), Bernoulli reconstruction rows
//   losses = {mean_b(recon_b + beta (kld_b + aux_kld_b)), mean recon, mean (kld + aux_kld)}
//   (the trunk half of Fe / Fr enters as a row bias, computed once per image: the same code serves the evaluation's k rows per image)
// Backward (c = loss_scale / B), every reparameterisation and both KLs in closed form, as csrc/auxvae.hip's: the reconstruction seed and the decoder; the
// pair KL's seed; aux_decode back into its z columns (dz = the decoder's + the auxiliary decoder's) and into h3r; the head's seed; encode back into z0
// and h3e; the first head's seed; aux_encode; the three trunks; every weight gradient - 28 problems - in one list.
// Decode-only (ardae_model_decode: the importance samples, generate, decode_params): the decoder up to u1, then conv_tail_kernel - unless
// ARDAE_CONV_TAIL_UNFUSED=1 under ARDAE_DEBUG_KNOBS=1.  The training forward keeps the unfused launches.
#include <cmath>

#include "ardae_hip.h"
#include "auxconvvae.h"
#include "auxvae.h"
#include "common.h"
#include "convmodel.h"
#include "vaemodel.h"

namespace ardae {
namespace {

enum { TR_A = 0, TR_E = 1, TR_R = 2 };      // the three trunks: aux_encode, encode, aux_decode

struct AuxConvVaeLayout {
  int nd, zd, act, h = 800;
  Lin conv[3][3], afc, mean0, logvar0, efc, mean, logvar, rfc, meanp, logvarp;
  ConvDecLayout dec;
  size_t total;
  explicit AuxConvVaeLayout(const ardae_model_desc& d) : nd(d.noise_dim), zd(d.z_dim), act(d.act) {
    size_t off = 0;
    trunk_lins(off, conv[TR_A]); afc = next_lin(off, 800, 512); mean0 = next_lin(off, nd, 800); logvar0 = next_lin(off, nd, 800);
    trunk_lins(off, conv[TR_E]); efc = next_lin(off, 800, 512 + nd); mean = next_lin(off, zd, 800); logvar = next_lin(off, zd, 800);
    dec = ConvDecLayout(zd, act, off);
    trunk_lins(off, conv[TR_R]); rfc = next_lin(off, 800, 512 + zd); meanp = next_lin(off, nd, 800); logvarp = next_lin(off, nd, 800);
    total = off;
  }
};

// Linear on cat[h3, s] (h3 [B, 512] a trunk's output, FIRST in the concat; s [R, sd]): both halves forward and backward-data - unlike csrc/auxvae.hip's
// CondStack, whose first half is the image and takes no gradient
struct CatLin { size_t i_f, i_b, s_f, s_b; };

struct AuxConvVaePacked {
  size_t conv_f[3][3], conv_b[3][3], afc_f, afc_b, mean0_f, mean0_b, logvar0_f, logvar0_b, mean_f, mean_b, logvar_f, logvar_b, meanp_f, meanp_b, logvarp_f,
      logvarp_b;
  CatLin efc, rfc;
  ConvDecPacked dec;
  size_t tail_w2, tail_w3;         // conv_tail_kernel's weights (launch_conv_tail_pack fills them after the pack launch)
  AuxConvVaePacked(const AuxConvVaeLayout& P, PackList& pl) {
    auto trunk = [&](int k) { trunk_panels(P.conv[k], pl, conv_f[k], conv_b[k]); };
    auto cat = [&](const Lin& l, CatLin& c) { pl.pair(l, c.i_f, c.i_b, 0, 512); pl.pair(l, c.s_f, c.s_b, 512, l.in - 512); };
    trunk(TR_A); pl.pair(P.afc, afc_f, afc_b); pl.pair(P.mean0, mean0_f, mean0_b); pl.pair(P.logvar0, logvar0_f, logvar0_b);
    trunk(TR_E); cat(P.efc, efc); pl.pair(P.mean, mean_f, mean_b); pl.pair(P.logvar, logvar_f, logvar_b);
    dec = ConvDecPacked(P.dec, pl);
    trunk(TR_R); cat(P.rfc, rfc); pl.pair(P.meanp, meanp_f, meanp_b); pl.pair(P.logvarp, logvarp_f, logvarp_b);
    tail_w2 = pl.take(CT_W2); tail_w3 = pl.take(CT_W3);
  }
  explicit AuxConvVaePacked(const AuxConvVaeLayout& P, PackList&& sizing = PackList()) : AuxConvVaePacked(P, sizing) {}   // offsets only
};

struct AuxConvVaeWs {
  float* x2; TrunkBuf T[3]; TrunkScratch S;      // cols[0], the im2col rows of x2, is the same buffer in all three trunks; ONE scratch set
  float *h4a, *mu0, *lv0, *eps0, *epsz, *z0, *rb, *h4, *mu, *lv, *z, *eps, *kld, *rb2, *h4r, *mup, *lvp;
  ConvDecWs D;
  float *dmu, *dlv, *dz, *dz0, *dmu0, *dlv0, *dmup, *dlvp, *dh4r, *dh4, *dh4a;      // dz: the decoder's (D.dz) + the auxiliary decoder's
};

// which tail the decode-only path runs (ardae_conv_tail's variant 0; the mode-2 workspace is sized for the answer): conv_tail_kernel, unless
// ARDAE_CONV_TAIL_UNFUSED=1 under ARDAE_DEBUG_KNOBS=1
bool tail_fused_default() {
  const char* knob = debug_knob("ARDAE_CONV_TAIL_UNFUSED");
  return !(knob && knob[0] == '1');
}

// mode 0: aux_encode up to h4a (encode_stats writes mu0, lv0 to the caller); 1: forward + backward; 2: the decoder's forward on B rows of z
void carve(const AuxConvVaeLayout& P, const AuxConvVaePacked&, Bump& ws, int B, int mode, AuxConvVaeWs& W) {
  const size_t b = (size_t)B;
  if (mode == 2) return conv_decoder_carve(ws, b, P.zd, ConvDecRuns{true, !tail_fused_default(), false, false}, W.D);
  W.x2 = ws.take(b * 784);
  trunk_carve(ws, b, W.T[TR_A]);
  W.h4a = ws.take(b * 800);
  if (mode == 0) return;
  trunk_carve(ws, b, W.T[TR_E], &W.T[TR_A]); trunk_carve(ws, b, W.T[TR_R], &W.T[TR_A]);
  W.mu0 = ws.take(b * P.nd); W.lv0 = ws.take(b * P.nd); W.eps0 = ws.take(b * P.nd); W.epsz = ws.take(b * P.zd); W.z0 = ws.take(b * P.nd);
  W.rb = ws.take(b * 800); W.h4 = ws.take(b * 800);
  W.mu = ws.take(b * P.zd); W.lv = ws.take(b * P.zd); W.z = ws.take(b * P.zd); W.eps = ws.take(b * P.zd); W.kld = ws.take(b);
  W.rb2 = ws.take(b * 800); W.h4r = ws.take(b * 800); W.mup = ws.take(b * P.nd); W.lvp = ws.take(b * P.nd);
  conv_decoder_carve(ws, b, P.zd, CONV_DEC_TRAIN, W.D);
  W.dmu = ws.take(b * P.zd); W.dlv = ws.take(b * P.zd); W.dz = ws.take(b * P.zd);
  W.dz0 = ws.take(b * P.nd); W.dmu0 = ws.take(b * P.nd); W.dlv0 = ws.take(b * P.nd); W.dmup = ws.take(b * P.nd); W.dlvp = ws.take(b * P.nd);
  W.dh4r = ws.take(b * 800); W.dh4 = ws.take(b * 800); W.dh4a = ws.take(b * 800);
  for (int k = 0; k < 3; ++k) trunk_bwd_carve(ws, b, W.T[k], k == 0 ? &W.S : nullptr);
}
using AuxConvVaeEntry = Entry<AuxConvVaeLayout, AuxConvVaePacked, AuxConvVaeWs>;

// wgrad_splits hint of the backward (a tuning value, as CONV_WGRAD_HINT), and the size of its first batch: the 28 problems go out as 14 + 14
constexpr int ACV_WGRAD_HINT = 14;

// every weight-gradient problem of the backward: the decoder's eight, the z head, encode.fc's two halves and trunk, the z0 head, aux_encode.fc and
// trunk, the auxiliary decoder's head, its fc's two halves and trunk
void auxconvvae_wgrads(const AuxConvVaeLayout& P, const AuxConvVaeWs& W, int B, WgradList& wl, Bump& ws) {
  conv_decoder_wgrads(P.dec, W.D, W.z, B, wl);
  wl.push(B, P.zd, 800, W.dmu, W.h4, 800, wl.g(P.mean.w), 800, wl.g(P.mean.b));
  wl.push(B, P.zd, 800, W.dlv, W.h4, 800, wl.g(P.logvar.w), 800, wl.g(P.logvar.b));
  cat_wgrads(wl, B, P.efc, 512, W.dh4, W.z0, W.T[TR_E].inp);
  conv_trunk_wgrads(P.conv[TR_E], W.T[TR_E], B, wl);
  wl.push(B, P.nd, 800, W.dmu0, W.h4a, 800, wl.g(P.mean0.w), 800, wl.g(P.mean0.b));
  wl.push(B, P.nd, 800, W.dlv0, W.h4a, 800, wl.g(P.logvar0.w), 800, wl.g(P.logvar0.b));
  wl.push(B, 800, 512, W.dh4a, W.T[TR_A].inp, 512, wl.g(P.afc.w), 512, wl.g(P.afc.b));
  conv_trunk_wgrads(P.conv[TR_A], W.T[TR_A], B, wl);
  wl.push(B, P.nd, 800, W.dmup, W.h4r, 800, wl.g(P.meanp.w), 800, wl.g(P.meanp.b));
  wl.push(B, P.nd, 800, W.dlvp, W.h4r, 800, wl.g(P.logvarp.w), 800, wl.g(P.logvarp.b));
  cat_wgrads(wl, B, P.rfc, 512, W.dh4r, W.z, W.T[TR_R].inp);
  conv_trunk_wgrads(P.conv[TR_R], W.T[TR_R], B, wl);
  wl.assign(ws, ACV_WGRAD_HINT);
}

// The evaluation pass (mode 4): x2 and ONE trunk's buffers, which serve encode's and aux_decode's trunk in turn, in front of the shared rows
struct AuxConvEvalWs : AuxEvalRows {
  float* x2;
  TrunkBuf T;
};

struct AuxConvVaeTraits {
  using Layout = AuxConvVaeLayout; using Packed = AuxConvVaePacked; using Entry = AuxConvVaeEntry;
  static Entry open(const ardae_model_desc& d, float* workspace, size_t wsf, int B, int mode) { return Entry(d, workspace, wsf, B, mode); }
  // encode.reparam on h4: kind 11's head and policy (the tail form, the default for z <= 64)
  static GaussHead head_of(const AuxConvVaeLayout& P, const AuxConvVaePacked& K) {
    return GaussHead{800, P.zd, P.mean, P.logvar, K.mean_f, K.logvar_f, true, P.zd >= 1 && P.zd <= 64};
  }
  static const float* hid(const AuxConvVaeWs& W) { return W.h4; }
  static GaussBufs bufs(const AuxConvVaeWs& W) {
    const ConvDecWs& D = W.D;
    return {W.mu, W.lv, W.z, W.eps, W.kld, D.rec_row, D.pri_row, D.logit, nullptr, D.dlogit, nullptr, D.dzq, D.dz, W.dmu, W.dlv};
  }
  // x2 and aux_encode up to (mu0, lv0); its trunk fills the im2col rows of x2 the other two read
  static int stats_fwd(Entry& en, const float* params, const float* packed, const float* x, int B, float* mu0, float* lv0, hipStream_t st) {
    auto& [P, K, ws, W] = en;
    const TrunkBuf& T = W.T[TR_A];
    ARDAE_TRY(launch_affine(x, (int64_t)B * 784, 2.f, -1.f, W.x2, st));
    ARDAE_TRY(trunk_fwd(P.conv[TR_A], K.conv_f[TR_A], params, packed, W.x2, T, B, P.act, st));
    ARDAE_TRY(dense_fwd(P.act, B, 800, T.inp, 512, 512, packed + K.afc_f, params + P.afc.b, W.h4a, st));
    ARDAE_TRY(dense_fwd(ACT_NONE, B, P.nd, W.h4a, 800, 800, packed + K.mean0_f, params + P.mean0.b, mu0, st));
    return dense_fwd(ACT_NONE, B, P.nd, W.h4a, 800, 800, packed + K.logvar0_f, params + P.logvar0.b, lv0, st);
  }
  // (the two draws are in W.eps0 / W.epsz: aux_vae_forward)  aux_encode, z0, encode's trunk and fc
  static int encoder_fwd(Entry& en, const float* params, const float* packed, const float* x, int B, hipStream_t st) {
    auto& [P, K, ws, W] = en;
    const TrunkBuf& T = W.T[TR_E];
    ARDAE_TRY(stats_fwd(en, params, packed, x, B, W.mu0, W.lv0, st));
    ARDAE_TRY(launch_reparam_fwd(W.mu0, W.lv0, W.eps0, P.nd, B, P.nd, 1, W.z0, st));
    ARDAE_TRY(trunk_fwd(P.conv[TR_E], K.conv_f[TR_E], params, packed, W.x2, T, B, P.act, st, true));
    return cat_fwd(P.act, B, 1, 800, T.inp, 512, packed + K.efc.i_f, params + P.efc.b, W.z0, P.nd, packed + K.efc.s_f, W.rb, W.h4, st);
  }
  // the auxiliary decoder on [h3r | z] and the pair KL, added into the head's KL rows; then the decoder
  static int decoder_fwd(Entry& en, const float* params, const float* packed, int B, hipStream_t st) {
    auto& [P, K, ws, W] = en;
    const TrunkBuf& T = W.T[TR_R];
    ARDAE_TRY(trunk_fwd(P.conv[TR_R], K.conv_f[TR_R], params, packed, W.x2, T, B, P.act, st, true));
    ARDAE_TRY(cat_fwd(P.act, B, 1, 800, T.inp, 512, packed + K.rfc.i_f, params + P.rfc.b, W.z, P.zd, packed + K.rfc.s_f, W.rb2, W.h4r, st));
    ARDAE_TRY(dense_fwd(ACT_NONE, B, P.nd, W.h4r, 800, 800, packed + K.meanp_f, params + P.meanp.b, W.mup, st));
    ARDAE_TRY(dense_fwd(ACT_NONE, B, P.nd, W.h4r, 800, 800, packed + K.logvarp_f, params + P.logvarp.b, W.lvp, st));
    ARDAE_TRY(launch_pair_kld_rows(W.mu0, W.lv0, W.mup, W.lvp, B, P.nd, W.kld, 1, st));
    return conv_decode_fwd(P.dec, K.dec, params, packed, W.z, B, W.D, st);
  }
  struct Grads { float* grads; float beta; };
  static Grads grads_of(Entry&, const float*, const float*, float* grads, float grads_beta) { return {grads, grads_beta}; }
  static int decoder_bwd(Entry& en, const float* packed, int B, Grads&, hipStream_t st) { return conv_decoder_bwd(en.P.dec, en.K.dec, packed, en.W.D, B, st); }
  // the auxiliary decoder back into its z columns (dz = D.dz + dh4r Wz) and into h3r (the trunk applies conv3's act')
  static int aux_decoder_bwd(Entry& en, const float* packed, int B, Grads&, hipStream_t st) {
    auto& [P, K, ws, W] = en;
    ARDAE_TRY(dense_bwd2(P.act, B, 800, W.dmup, packed + K.meanp_b, W.dlvp, packed + K.logvarp_b, P.nd, W.h4r, W.dh4r, st));
    return cat_bwd(B, 800, W.dh4r, P.zd, packed + K.rfc.s_b, W.D.dz, W.dz, 512, packed + K.rfc.i_b, nullptr, W.T[TR_R].dinp, st);
  }
  // encode.fc back into its z0 columns and into h3e
  static int encode_fc_bwd(Entry& en, const float* packed, int B, Grads&, hipStream_t st) {
    auto& [P, K, ws, W] = en;
    ARDAE_TRY(dense_bwd2(P.act, B, 800, W.dmu, packed + K.mean_b, W.dlv, packed + K.logvar_b, P.zd, W.h4, W.dh4, st));
    return cat_bwd(B, 800, W.dh4, P.nd, packed + K.efc.s_b, nullptr, W.dz0, 512, packed + K.efc.i_b, nullptr, W.T[TR_E].dinp, st);
  }
  // the first head (there is no clip in this family), aux_encode.fc, the three trunks; the 28 weight gradients as two batches
  static int aux_encoder_bwd(Entry& en, const float* packed, int B, Grads& g, hipStream_t st) {
    auto& [P, K, ws, W] = en;
    ARDAE_TRY(dense_bwd2(P.act, B, 800, W.dmu0, packed + K.mean0_b, W.dlv0, packed + K.logvar0_b, P.nd, W.h4a, W.dh4a, st));
    ARDAE_TRY(dense_fwd(ACT_NONE, B, 512, W.dh4a, 800, 800, packed + K.afc_b, nullptr, W.T[TR_A].dinp, st));
    for (int k = 0; k < 3; ++k) ARDAE_TRY(trunk_bwd(K.conv_b[k], packed, W.T[k], W.S, B, P.act, st));
    WgradList wl(g.grads, g.beta);
    auxconvvae_wgrads(P, W, B, wl, ws);
    ARDAE_CHECK_ARG(ws.ok, "vae_backward: internal workspace accounting error");
    ARDAE_TRY(wl.launch(st, ACV_WGRAD_HINT));
    return wl.launch(st);
  }
  static void size_wgrads(Entry& en, int B) {
    WgradList wl(nullptr);
    auxconvvae_wgrads(en.P, en.W, B, wl, en.ws);
  }
  // the evaluation pass (aux_vae_iwae_draw, csrc/auxvae.h)
  using EvalWs = AuxConvEvalWs;
  static void carve_eval(const AuxConvVaeLayout& P, const AuxConvVaePacked&, Bump& ws, int B, int k, AuxConvEvalWs& W) {
    const size_t b = (size_t)B;
    W.x2 = ws.take(b * 784);
    trunk_carve(ws, b, W.T);
    W.carve_rows(ws, B, k, P.nd, P.zd, 800, 1);
  }
  static int eval_prepare(const AuxConvVaeLayout&, const float* x, int B, AuxConvEvalWs& W, const float*& xs, hipStream_t st) {
    xs = W.x2;
    return launch_affine(x, (int64_t)B * 784, 2.f, -1.f, W.x2, st);
  }
  static int eval_hidden(const AuxConvVaeLayout& P, const AuxConvVaePacked& K, const float* params, const float* packed, int stage, const float* xs,
                         const float* s, int B, int k, AuxConvEvalWs& W, const float*& hid, hipStream_t st) {
    const int tr = stage == 2 ? TR_E : TR_R;
    const Lin& l = stage == 2 ? P.efc : P.rfc;
    const CatLin& c = stage == 2 ? K.efc : K.rfc;
    hid = W.t[1];
    ARDAE_TRY(trunk_fwd(P.conv[tr], K.conv_f[tr], params, packed, xs, W.T, B, P.act, st, stage == 3));
    return cat_fwd(P.act, B, k, 800, W.T.inp, 512, packed + c.i_f, params + l.b, s, l.in - 512, packed + c.s_f, W.rb, W.t[1], st);
  }
};

// u1 [R, 8, 8, 32] -> logits [R, 784]; fused: conv_tail_kernel, else the four unfused launches on c2 / u2 / c3 / logit (then copied out)
int tail_fwd(const AuxConvVaeLayout& P, const AuxConvVaePacked& K, const float* params, const float* packed, const float* u1, int R, bool fused, ConvDecWs& C,
             float* logits, hipStream_t st) {
  if (fused)
    return launch_conv_tail(u1, packed + K.tail_w2, params + P.dec.dcv[1].b, packed + K.tail_w3, params + P.dec.dcv[2].b, R, P.act, logits, st);
  ARDAE_TRY(conv_decode_tail_fwd(P.dec, K.dec, params, packed, u1, R, C, st));
  return launch_copy(C.logit, (int64_t)R * 784, logits, st);
}

int auxconvvae_decode(const ardae_model_desc& d, const float* params, const float* packed, const float* z, int R, float* workspace, size_t wsf,
                      float* out0, hipStream_t st, float*) {
  AuxConvVaeEntry entry(d, workspace, wsf, R, 2);
  auto& [P, K, ws, W] = entry;
  ARDAE_CHECK_ARG(ws.ok, "model_decode: workspace too small");
  ARDAE_TRY(conv_decode_head_fwd(P.dec, K.dec, params, packed, z, R, W.D, st));
  return tail_fwd(P, K, params, packed, W.D.u1, R, tail_fused_default(), W.D, out0, st);
}

// the pack launch, then the fused tail's two weights
int auxconvvae_pack(const ardae_model_desc& d, const float* params, float* packed, hipStream_t st) {
  const AuxConvVaeLayout P(d);
  PackList pl(params, packed);
  const AuxConvVaePacked K(P, pl);
  ARDAE_TRY(pl.launch(st));
  return launch_conv_tail_pack(params + P.dec.dcv[1].w, params + P.dec.dcv[2].w, packed + K.tail_w2, packed + K.tail_w3, st);
}

// the descriptor rules of kind 17 (input_dim 784, h_dim 800, n_layers 1, 1 <= noise_dim <= AV_NMAX, flags 0, z_dim >= 1, any activation but NONE)
int auxconvvae_desc_check(const ardae_model_desc* d) {
  ARDAE_CHECK_ARG(d->noise_dim >= 1 && d->noise_dim <= AV_NMAX, "model: noise_dim must be 1 .. %d for kind 17 (the width of z0), got %d", AV_NMAX,
                  d->noise_dim);
  ARDAE_CHECK_ARG(d->flags == 0, "model: flags must be 0 for kind 17, got %d", d->flags);
  return conv_gauss_desc_check(d, "MNISTConvAuxVAE", "the width of the three fc layers");
}

// (host pass only, as in csrc/auxmodel.hip)
#ifndef __HIP_DEVICE_COMPILE__
const GaussFamily AUXCONVVAE_GAUSS = aux_gauss_family<AuxConvVaeTraits>();
#endif

}  // namespace

#ifndef __HIP_DEVICE_COMPILE__
const Family AUXCONVVAE_FAMILY = {auxconvvae_desc_check, no_caps, family_param_floats<AuxConvVaeLayout, AuxConvVaePacked>,
                                  family_packed_floats<AuxConvVaeLayout, AuxConvVaePacked>, aux_workspace_floats<AuxConvVaeTraits>,
                                  auxconvvae_pack, vae_no_encode, auxconvvae_decode, vae_no_forward, vae_no_backward,
                                  &AUXCONVVAE_GAUSS};
#endif

}  // namespace ardae

using namespace ardae;

extern "C" {

// floats of the buffers the unfused launches keep: c2, u2, c3 and the logits
size_t ardae_conv_tail_workspace_floats(const ardae_model_desc* d, int R, int variant) {
  if (!d || d->kind != 17 || auxconvvae_desc_check(d) || R <= 0 || R >= (1 << 20) || variant < 0 || variant > 2) return 0;
  if (variant == 1 || (variant == 0 && tail_fused_default())) return 0;
  Bump ws; ConvDecWs C;
  conv_decoder_carve(ws, (size_t)R, d->z_dim, CONV_DEC_TAIL, C);
  return ws.off;
}

int ardae_conv_tail(const ardae_model_desc* d, const float* params, const float* packed, const float* u1, int R, int variant, float* workspace,
                    size_t workspace_floats, float* logits, void* stream) {
  ARDAE_CHECK_ARG(d != nullptr, "conv_tail: desc is NULL");
  ARDAE_CHECK_ARG(d->kind == 17, "conv_tail: kind must be 17 (MNISTConvAuxVAE), got %d", d->kind);
  ARDAE_TRY(auxconvvae_desc_check(d));
  ARDAE_CHECK_ARG(variant >= 0 && variant <= 2, "conv_tail: variant must be 0 (the library's choice), 1 (fused) or 2 (unfused), got %d", variant);
  ARDAE_CHECK_ARG(params && packed && u1 && logits, "conv_tail: null pointer argument");
  ARDAE_CHECK_ARG(R > 0 && R < (1 << 20), "conv_tail: bad batch (R=%d)", R);
  if (variant == 0) variant = tail_fused_default() ? 1 : 2;
  const AuxConvVaeLayout P(*d);
  const AuxConvVaePacked K(P);
  ConvDecWs C{};
  if (variant == 2) {
    const size_t need = ardae_conv_tail_workspace_floats(d, R, 2);
    ARDAE_CHECK_ARG(workspace, "conv_tail: null pointer argument (the unfused launches need a workspace)");
    ARDAE_CHECK_ARG(workspace_floats >= need, "conv_tail: workspace too small (%zu < %zu floats)", workspace_floats, need);
    Bump ws(workspace, workspace_floats);
    conv_decoder_carve(ws, (size_t)R, d->z_dim, CONV_DEC_TAIL, C);
  }
  return tail_fwd(P, K, params, packed, u1, R, variant == 1, C, logits, (hipStream_t)stream);
}

}  // extern "C"
