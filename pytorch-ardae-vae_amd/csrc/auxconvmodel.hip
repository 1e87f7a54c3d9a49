// MNISTConvAuxIPVAE (`--model auxconv`, ardae_model_desc.kind 4): models/ivae/auxconv.py:48-126 - the hierarchical sampler of csrc/auxmodel.hip with
// conv trunks in place of the MLPs (models/vae/auxconv.py:32-140) and ConvIPVAE's decoder (models/vae/conv.py:79-136), both csrc/convmodel.h's:
//   per image:   h3a = trunk_a(2x-1); h4a = act(Fa h3a + fa); mu0 = M0 h4a + m0; lv0 = L0 h4a + l0;  h3 = trunk_e(2x-1); rb = Fi h3 + f
//   per sample:  z0 = mu0[b] + exp(lv0[b]/2) eps0;  h4 = act(Fn z0 + rb[b]);  mu = M h4 + m; lv = L h4 + l;  z = mu + exp(lv/2) eps
// Noise layout as for kind 3: one [R, noise_dim + z_dim] tensor per sampler call.  hidden1a context = cat(h4a, h4) [B, 1600].  No kernel of its own.
#include "ardae_hip.h"
#include "common.h"
#include "auxmodel.h"
#include "convmodel.h"
#include "ipmodel.h"

namespace ardae {
namespace {

enum { TR_A = 0, TR_E = 1 };      // the two trunks: aux encoder, encoder

struct AuxConvLayout {
  int nd, zd, act;
  Lin aconv[3], afc, mean0, logvar0, econv[3], efc, mean, logvar;
  ConvDecLayout dec;
  size_t total;
  explicit AuxConvLayout(const ardae_model_desc& d) : nd(d.noise_dim), zd(d.z_dim), act(d.act) {
    size_t off = 0;
    trunk_lins(off, aconv); afc = next_lin(off, 800, 512); mean0 = next_lin(off, nd, 800); logvar0 = next_lin(off, nd, 800);
    trunk_lins(off, econv); efc = next_lin(off, 800, 512 + nd); mean = next_lin(off, zd, 800); logvar = next_lin(off, zd, 800);
    dec = ConvDecLayout(zd, act, off);
    total = off;
  }
};

struct AuxConvPacked {
  size_t aconv_f[3], aconv_b[3], afc_f, afc_b, mean0_f, mean0_b, logvar0_f, logvar0_b, econv_f[3], econv_b[3], efci_f, efci_b, efcn_f, efcn_b,
      mean_f, mean_b, logvar_f, logvar_b;
  ConvDecPacked dec;
  AuxConvPacked(const AuxConvLayout& P, PackList& pl) {
    trunk_panels(P.aconv, pl, aconv_f, aconv_b);
    pl.pair(P.afc, afc_f, afc_b); pl.pair(P.mean0, mean0_f, mean0_b); pl.pair(P.logvar0, logvar0_f, logvar0_b);
    trunk_panels(P.econv, pl, econv_f, econv_b);
    pl.pair(P.efc, efci_f, efci_b, 0, 512);                            // [800, 512 + nd]: image half | z0 half
    pl.pair(P.efc, efcn_f, efcn_b, 512, P.nd);
    pl.pair(P.mean, mean_f, mean_b); pl.pair(P.logvar, logvar_f, logvar_b);
    dec = ConvDecPacked(P.dec, pl);
  }
  explicit AuxConvPacked(const AuxConvLayout& P, PackList&& sizing = PackList()) : AuxConvPacked(P, sizing) {}   // offsets only
};

struct AuxConvWs {
  float* x2; TrunkBuf T[2]; TrunkScratch S[2];      // each trunk its own im2col rows of x2 and its own scratch set; ONE dinp_t
  float *h4a, *mu0, *lv0, *z0, *rb, *h4, *mu, *lv, *z, *zero;
  ConvDecWs D;
  float *dlv, *dh4, *dz0, *dlv0r, *drb, *dmu0, *dlv0, *dh4a;      // backward
};

void carve(const AuxConvLayout& P, const AuxConvPacked&, Bump& ws, int B, int nz, int mode, AuxConvWs& W) {
  const size_t R = (size_t)B * nz, b = (size_t)B;
  W.x2 = ws.take(b * 784);
  for (TrunkBuf& T : W.T) trunk_carve(ws, b, T);
  W.h4a = ws.take(b * 800); W.mu0 = ws.take(b * P.nd); W.lv0 = ws.take(b * P.nd); W.rb = ws.take(b * 800);
  W.z0 = ws.take(R * P.nd); W.h4 = ws.take(R * 800); W.mu = ws.take(R * P.zd); W.lv = ws.take(R * P.zd); W.z = ws.take(R * P.zd); W.zero = ws.take(R * (P.nd + P.zd));
  if (mode == 0) return;
  conv_decoder_carve(ws, R, P.zd, mode == 2 ? CONV_DEC_DECODE : CONV_DEC_TRAIN, W.D);
  if (mode == 2) return;
  W.dlv = ws.take(R * P.zd); W.dh4 = ws.take(R * 800); W.dz0 = ws.take(R * P.nd); W.dlv0r = ws.take(R * P.nd);
  W.drb = ws.take(b * 800); W.dmu0 = ws.take(b * P.nd); W.dlv0 = ws.take(b * P.nd); W.dh4a = ws.take(b * 800);
  trunk_bwd_carve(ws, b, W.T[TR_A], &W.S[TR_A]); trunk_bwd_carve(ws, b, W.T[TR_E], &W.S[TR_E], &W.S[TR_A]);
}
using AuxConvEntry = Entry<AuxConvLayout, AuxConvPacked, AuxConvWs>;

// wgrad_splits hint of the hierarchical conv backward, and the size of its first batch: the 21 problems go out as 10 + 11
constexpr int AUX_WGRAD_HINT = 10;

// keep_hidden = false (forward-only encodes of the cDAE phase): the [R, 800] hidden rows need not exist
int aux_sampler_fwd(const AuxConvLayout& P, const AuxConvPacked& K, const float* params, const float* packed, const float* x, const float* noise,
                    int B, int nz, AuxConvWs& W, bool keep_hidden, hipStream_t st) {
  const int R = B * nz, act = P.act, ldn = P.nd + P.zd;
  const TrunkBuf &Ta = W.T[TR_A], &Te = W.T[TR_E];
  ARDAE_TRY(launch_affine(x, (int64_t)B * 784, 2.f, -1.f, W.x2, st));
  ARDAE_TRY(trunk_fwd(P.aconv, K.aconv_f, params, packed, W.x2, Ta, B, act, st));
  ARDAE_TRY(dense_fwd(act, B, 800, Ta.inp, 512, 512, packed + K.afc_f, params + P.afc.b, W.h4a, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, B, P.nd, W.h4a, 800, 800, packed + K.mean0_f, params + P.mean0.b, W.mu0, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, B, P.nd, W.h4a, 800, 800, packed + K.logvar0_f, params + P.logvar0.b, W.lv0, st));
  ARDAE_TRY(launch_reparam_fwd(W.mu0, W.lv0, noise, ldn, R, P.nd, nz, W.z0, st));
  ARDAE_TRY(trunk_fwd(P.econv, K.econv_f, params, packed, W.x2, Te, B, act, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, B, 800, Te.inp, 512, 512, packed + K.efci_f, params + P.efc.b, W.rb, st));   // image half of the encoder's fc, once per image
  if (!keep_hidden) {    // z0 -> 800 -> (mean | logvar) in one launch, hidden rows on chip (linear_shortk.hip::sampler_tail_kernel)
    LinArgs A{}; A.M = R; A.Nout = 800; A.act = act; A.nsrc = 1; A.rowbias = W.rb; A.rowbias_ld = 800; A.rows_per_group = nz;
    A.src[0].x = W.z0; A.src[0].ld = P.nd; A.src[0].K = P.nd; A.src[0].wp = packed + K.efcn_f;
    if (sampler_tail_eligible(A, P.zd)) {
      ARDAE_TRY(launch_sampler_tail(A, packed + K.mean_f, params + P.mean.b, W.mu, P.zd, P.zd, st, packed + K.logvar_f, params + P.logvar.b, W.lv, P.zd));
      return launch_reparam_fwd(W.mu, W.lv, noise + P.nd, ldn, R, P.zd, 1, W.z, st);
    }
  }
  { LinArgs A{}; A.rowbias = W.rb; A.rowbias_ld = 800; A.rows_per_group = nz; A.Y = W.h4; A.ldY = 800;
    ARDAE_TRY(lin1(EPI_ACT, act, R, 800, W.z0, P.nd, P.nd, packed + K.efcn_f, A, st)); }
  ARDAE_TRY(dense_fwd(ACT_NONE, R, P.zd, W.h4, 800, 800, packed + K.mean_f, params + P.mean.b, W.mu, st));
  ARDAE_TRY(dense_fwd(ACT_NONE, R, P.zd, W.h4, 800, 800, packed + K.logvar_f, params + P.logvar.b, W.lv, st));
  return launch_reparam_fwd(W.mu, W.lv, noise + P.nd, ldn, R, P.zd, 1, W.z, st);
}

// What the shared algorithm (csrc/ipmodel.h) needs to know of MNISTConvAuxIPVAE.
struct AuxConvTraits : IpTraitsBase {
  using Layout = AuxConvLayout; using Packed = AuxConvPacked; using Ws = AuxConvWs; using Entry = AuxConvEntry;
  static int desc_check(const ardae_model_desc* d) { return conv_desc_check(d); }
  static unsigned caps(const ardae_model_desc&) { return CAP_HIDDEN; }
  static IpBufs bufs(const AuxConvWs& W) { return {W.z, W.D.logit, nullptr, W.D.dlogit, nullptr, W.D.dzq, W.D.dz, W.D.rec_row, W.D.pri_row}; }
  // every weight-gradient problem of the backward, with its scratch taken from ws
  static void wgrads(const AuxConvLayout& P, const AuxConvPacked&, const AuxConvWs& W, const float*, const float*, int B, int nz, WgradList& wl, Bump& ws) {
    const int R = B * nz;
    conv_decoder_wgrads(P.dec, W.D, W.z, R, wl);                                                      // decoder (as ConvIPVAE)
    wl.push(R, P.zd, 800, W.D.dz, W.h4, 800, wl.g(P.mean.w), 800, wl.g(P.mean.b));
    wl.push(R, P.zd, 800, W.dlv, W.h4, 800, wl.g(P.logvar.w), 800, wl.g(P.logvar.b));
    wl.push(R, 800, P.nd, W.dh4, W.z0, P.nd, wl.g(P.efc.w + 512), 512 + P.nd, wl.g(P.efc.b));         // fc z0 half (+ bias)
    wl.push(B, 800, 512, W.drb, W.T[TR_E].inp, 512, wl.g(P.efc.w), 512 + P.nd, nullptr);              // fc image half
    conv_trunk_wgrads(P.econv, W.T[TR_E], B, wl);                                                     // encoder trunk
    wl.push(B, P.nd, 800, W.dmu0, W.h4a, 800, wl.g(P.mean0.w), 800, wl.g(P.mean0.b));
    wl.push(B, P.nd, 800, W.dlv0, W.h4a, 800, wl.g(P.logvar0.w), 800, wl.g(P.logvar0.b));
    wl.push(B, 800, 512, W.dh4a, W.T[TR_A].inp, 512, wl.g(P.afc.w), 512, wl.g(P.afc.b));
    conv_trunk_wgrads(P.aconv, W.T[TR_A], B, wl);                                                     // aux trunk
    wl.assign(ws, AUX_WGRAD_HINT);
  }
  static size_t noise_floats(const AuxConvLayout& P, int B, int nz) { return (size_t)B * nz * (P.nd + P.zd); }
  static float* zero_noise(Entry& e, size_t) { return e.W.zero; }
  // a forward-only pass keeps the [R, 800] hidden rows only where the hidden context is wanted
  static int sampler_fwd(Entry& e, const float* params, const float* packed, const float* x, const float* noise, int B, int nz, const IpEncodeOut* enc,
                         hipStream_t st) {
    return aux_sampler_fwd(e.P, e.K, params, packed, x, noise, B, nz, e.W, !enc || enc->hidden_out != nullptr, st);
  }
  static int hidden_copy(Entry& e, float* hidden_out, int B, hipStream_t st) {      // cat(h4a, h4)
    ARDAE_TRY(launch_copy2d(e.W.h4a, 800, hidden_out, 1600, B, 800, st));
    return launch_copy2d(e.W.h4, 800, hidden_out + 800, 1600, B, 800, st);
  }
  static int decoder_fwd(Entry& e, const float* params, const float* packed, const float* z, int R, hipStream_t st) {
    return conv_decode_fwd(e.P.dec, e.K.dec, params, packed, z, R, e.W.D, st);
  }
  static int decoder_bwd(Entry& e, const float* packed, int R, Grads&, hipStream_t st) { return conv_decoder_bwd(e.P.dec, e.K.dec, packed, e.W.D, R, st); }
  static int sampler_bwd(Entry& e, const float*, const float* packed, const float*, const float*, int B, int nz, Grads& g, hipStream_t st) {
    auto& [P, K, ws, W] = e;
    const int R = B * nz, act = P.act;
    // second reparameterisation and the encoder's fc
    ARDAE_TRY(launch_reparam_bwd(W.D.dz, W.z, W.mu, R, P.zd, 1, W.dlv, st));
    ARDAE_TRY(dense_bwd2(act, R, 800, W.D.dz, packed + K.mean_b, W.dlv, packed + K.logvar_b, P.zd, W.h4, W.dh4, st));
    ARDAE_TRY(dense_fwd(ACT_NONE, R, P.nd, W.dh4, 800, 800, packed + K.efcn_b, nullptr, W.dz0, st));
    ARDAE_TRY(launch_segment_sum(W.dh4, 800, B, nz, 800, 1.0f, W.drb, 800, st));
    ARDAE_TRY(dense_fwd(ACT_NONE, B, 512, W.drb, 800, 800, packed + K.efci_b, nullptr, W.T[TR_E].dinp, st));
    ARDAE_TRY(trunk_bwd(K.econv_b, packed, W.T[TR_E], W.S[TR_E], B, act, st));
    // first reparameterisation, reduced over the nz samples of each image, and the aux encoder
    ARDAE_TRY(launch_reparam_bwd(W.dz0, W.z0, W.mu0, R, P.nd, nz, W.dlv0r, st));
    ARDAE_TRY(launch_segment_sum(W.dz0, P.nd, B, nz, P.nd, 1.0f, W.dmu0, P.nd, st));
    ARDAE_TRY(launch_segment_sum(W.dlv0r, P.nd, B, nz, P.nd, 1.0f, W.dlv0, P.nd, st));
    ARDAE_TRY(dense_bwd2(act, B, 800, W.dmu0, packed + K.mean0_b, W.dlv0, packed + K.logvar0_b, P.nd, W.h4a, W.dh4a, st));
    ARDAE_TRY(dense_fwd(ACT_NONE, B, 512, W.dh4a, 800, 800, packed + K.afc_b, nullptr, W.T[TR_A].dinp, st));
    ARDAE_TRY(trunk_bwd(K.aconv_b, packed, W.T[TR_A], W.S[TR_A], B, act, st));
    // ---- weight gradients, launched as two batches
    WgradList wl(g.grads, g.beta);
    wgrads(P, K, W, nullptr, nullptr, B, nz, wl, ws);
    ARDAE_CHECK_ARG(ws.ok, "model_vae_backward: internal workspace accounting error");
    ARDAE_TRY(wl.launch(st, AUX_WGRAD_HINT));
    return wl.launch(st);
  }
};

}  // namespace

// (host pass only, as in csrc/convmodel.hip)
#ifndef __HIP_DEVICE_COMPILE__
const Family AUXCONV_FAMILY = ip_family<AuxConvTraits>();
#endif

}  // namespace ardae
