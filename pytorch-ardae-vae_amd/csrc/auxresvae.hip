// The hierarchical resconv Gaussian baseline (vae.py --model auxresconv / auxresconvct; ardae_model_desc.kind 19: MNISTResConvAuxVAE,
// models/vae/auxresconv.py:254-424): the Gaussian counterpart of kind 6, joined from the residual-conv pieces of csrc/resmodel.h (kind 12's trunk, head
// policy, decoder and weight-norm backward) and the pair KL, seeds and evaluation bodies of csrc/auxvae.h - no kernel of its own.
//   per image (B rows):  ctx = trunk(x or 2x - 1)  [B, c]  - ONE trunk, read by the three networks
//     aux_encode   mu0 = M0 ctx + m0;  lv0 = L0 ctx + l0 (no clip);  z0 = mu0 + exp(lv0 / 2) eps0
//     encode       h = ELU(Fe [ctx | z0] + fe);  mu, lv, z, kld: the Gaussian head on h (kind 12's policy: the unfused launches)
//     aux_decode   hr = ELU(Fr [ctx | z] + fr);  mup = Mp hr + mp;  lvp = Lp hr + lp;  aux_kld = KL(N(mu0, exp lv0) || N(mup, exp lvp)), added into kld
//     decode       kind 12's decoder, Bernoulli reconstruction rows
//   losses = {mean_b(recon_b + beta (kld_b + aux_kld_b)), mean recon, mean (kld + aux_kld)}
//   (the ctx half of Fe / Fr enters as a row bias, computed once per image: the same code serves the evaluation's k rows per image)
// Forward, backward, encode_stats, the evaluation passes and the workspace sizes are csrc/auxvae.h's bodies over AuxResVaeTraits; the backward's seeds
// and their order are aux_vae_backward's, and the traits' three hooks carry d ctx between them: aux_decode back into its z columns and into ctx, encode
// back into z0 and ctx, aux_encode back into ctx - d ctx is the SUM of the three, made before the trunk's backward.  The ten plain-Linear weight
// gradients go out as one list; the weight-normalised operators' block by block through wn_backward_kernel, as kind 12's.  The decode-only path runs
// the decoder's 14 x 14 stage as resconv_mid_kernel and its last stage as resconv_tail_kernel (csrc/resmodel.hip).
#include "ardae_hip.h"
#include "auxvae.h"
#include "common.h"
#include "resmodel.h"
#include "vaemodel.h"

namespace ardae {
namespace {

// (h, mean .. logvarp, mean_f .. logvarp_f: the names csrc/auxvae.h's bodies read)
struct AuxResLayout : ResLayout {
  Lin mu0{}, lv0{}, efc{}, mean{}, logvar{};   // aux_encode.reparam.{mean,logvar}_fn, encode.fc.0, encode.reparam.{mean,logvar}_fn
  Lin rfc{}, meanp{}, logvarp{};               // aux_decode.fc.0 on cat[ctx, z], aux_decode.reparam.{mean,logvar}_fn (behind the decoder)
  int h;
  explicit AuxResLayout(const ardae_model_desc& d) : ResLayout(d, d.h_dim), h(cdim) {
    ResWalk w;
    trunk_blocks(w);
    mu0 = w.lin(nd, cdim); lv0 = w.lin(nd, cdim); efc = w.lin(cdim, cdim + nd); mean = w.lin(zd, cdim); logvar = w.lin(zd, cdim);
    decoder_blocks(w);
    rfc = w.lin(cdim, cdim + zd); meanp = w.lin(nd, cdim); logvarp = w.lin(nd, cdim);
    total = w.off;
  }
};
struct AuxResPacked : ResPacked {
  LinPk mu0{}, lv0{}, efc{}, mean{}, logvar{}, rfc{}, meanp{}, logvarp{};
  size_t mid_w = 0;              // resconv_mid_kernel's weights (auxresvae_pack fills them after the pack launch)
  size_t mean_f, logvar_f, meanp_f, logvarp_f;
  AuxResPacked(const AuxResLayout& P, PackList& pl) {
    ResPackWalk w{pl};
    trunk_panels(P, w);
    mu0 = w.lin(P.mu0, 0); lv0 = w.lin(P.lv0, 0); efc = w.lin(P.efc, P.cdim); mean = w.lin(P.mean, 0); logvar = w.lin(P.logvar, 0);
    decoder_panels(P, w);
    rfc = w.lin(P.rfc, P.cdim); meanp = w.lin(P.meanp, 0); logvarp = w.lin(P.logvarp, 0); mid_w = pl.take(RM_WTOTAL);
    mean_f = mean.f; logvar_f = logvar.f; meanp_f = meanp.f; logvarp_f = logvarp.f;
  }
  explicit AuxResPacked(const AuxResLayout& P, PackList&& sizing = PackList()) : AuxResPacked(P, sizing) {}   // offsets only
};
// the rows of a training pass beside the shared buffers (B rows): the two heads, the two draws, encode.fc's and aux_decode.fc's row bias and rows,
// the auxiliary decoder's head, and the backward's seeds
struct AuxResWs : ResWs {
  float *mu0, *lv0, *eps0, *epsz, *z0, *rbh, *hh, *mu, *lv, *z, *eps, *kld, *rb2, *hr, *mup, *lvp;
  float *dmu, *dlv, *dz, *dz0, *dmu0, *dlv0, *dmup, *dlvp, *dhr, *dhh;
};

// mode 0: the trunk (encode_stats writes the caller's mu0, lv0); 1: forward + backward, one draw pair per image; 2: decode only on B rows with
// resconv_mid_kernel and resconv_tail_kernel (unless the knobs switch back)
void carve(const AuxResLayout& P, const AuxResPacked&, Bump& ws, int B, int mode, AuxResWs& W) {
  const size_t b = (size_t)B;
  if (mode == 2) return res_decoder_carve(P, ws, b, DecRuns{!mid_fused_default(), !tail_fused_default(), false}, W);
  res_trunk_carve(P, ws, B, W);
  if (mode == 0) return;
  W.mu0 = ws.take(b * P.nd); W.lv0 = ws.take(b * P.nd); W.eps0 = ws.take(b * P.nd); W.epsz = ws.take(b * P.zd); W.z0 = ws.take(b * P.nd);
  W.rbh = ws.take(b * P.cdim); W.hh = ws.take(b * P.cdim);
  W.mu = ws.take(b * P.zd); W.lv = ws.take(b * P.zd); W.z = ws.take(b * P.zd); W.eps = ws.take(b * P.zd); W.kld = ws.take(b);
  W.rb2 = ws.take(b * P.cdim); W.hr = ws.take(b * P.cdim); W.mup = ws.take(b * P.nd); W.lvp = ws.take(b * P.nd);
  W.dmu = ws.take(b * P.zd); W.dlv = ws.take(b * P.zd); W.dz = ws.take(b * P.zd);
  W.dz0 = ws.take(b * P.nd); W.dmu0 = ws.take(b * P.nd); W.dlv0 = ws.take(b * P.nd); W.dmup = ws.take(b * P.nd); W.dlvp = ws.take(b * P.nd);
  W.dhr = ws.take(b * P.cdim); W.dhh = ws.take(b * P.cdim);
  res_decoder_carve(P, ws, b, DecRuns{true, true, true}, W);
  // the ten plain-Linear problems, one list
  res_bwd_carve(P, ws, B, b, 2 * wgrad_scratch_floats(B, P.zd, P.cdim) + 4 * wgrad_scratch_floats(B, P.nd, P.cdim) +
                2 * wgrad_scratch_floats(B, P.cdim, P.cdim) + wgrad_scratch_floats(B, P.cdim, P.nd) + wgrad_scratch_floats(B, P.cdim, P.zd), W);
}
using AuxResEntry = Entry<AuxResLayout, AuxResPacked, AuxResWs>;

// the descriptor rules of kind 19 (1 <= noise_dim <= AV_NMAX, and the shared ones)
int auxresvae_desc_check(const ardae_model_desc* d) {
  ARDAE_CHECK_ARG(d->noise_dim >= 1 && d->noise_dim <= AV_NMAX, "model: noise_dim must be 1 .. %d for kind 19 (the width of z0), got %d", AV_NMAX,
                  d->noise_dim);
  return res_gauss_desc_check(d, "MNISTResConvAuxVAE", "models/vae/auxresconv.py:278");
}

// ardae_model_pack: the shared compose and pack launches, then resconv_mid_kernel's B operands from the effective weights they have written
int auxresvae_pack(const ardae_model_desc& d, const float* params, float* packed, hipStream_t st) {
  const AuxResLayout P(d);
  PackList pl(params, packed);
  const AuxResPacked K(P, pl);
  ARDAE_TRY(res_pack(P, K, {}, pl, st));
  return launch_mid_pack(K, packed, K.mid_w, st);
}

// The evaluation pass (mode 4): the trunk's buffers in front of the shared rows; the trunk runs once, in stage 2
struct AuxResEvalWs : AuxEvalRows {
  ResWs T;                                   // x2, the trunk's block buffers, flat; T.inp = ctx [B, c]
};

// What the bodies of csrc/auxvae.h need to know of kind 19.  Linear on cat[ctx | s]: cat_fwd / cat_bwd / cat_wgrads (host_util.h) at width c.
struct AuxResVaeTraits {
  using Layout = AuxResLayout; using Packed = AuxResPacked; using Entry = AuxResEntry;
  using Grads = GradMap;      // built before the decoder's backward, used again by the trunk's
  static Entry open(const ardae_model_desc& d, float* workspace, size_t wsf, int B, int mode) { return Entry(d, workspace, wsf, B, mode); }
  // encode.reparam on h [B, c]: kind 12's head and policy
  static GaussHead head_of(const AuxResLayout& P, const AuxResPacked& K) { return GaussHead{P.cdim, P.zd, P.mean, P.logvar, K.mean.f, K.logvar.f, false, false}; }
  static const float* hid(const AuxResWs& W) { return W.hh; }
  static GaussBufs bufs(const AuxResWs& W) {
    return {W.mu, W.lv, W.z, W.eps, W.kld, W.rec_row, W.pri_row, W.db[6].out, nullptr, W.dlogit, nullptr, W.dzq, W.dz, W.dmu, W.dlv};
  }
  // the trunk and aux_encode's two Linears on ctx: mu0, lv0 (no clip)
  static int stats_fwd(Entry& e, const float* params, const float* packed, const float* x, int B, float* mu0, float* lv0, hipStream_t st) {
    auto& [P, K, ws, W] = e;
    ARDAE_TRY(res_trunk_fwd(P, K, params, packed, x, B, W, st));
    ARDAE_TRY(dense_fwd(ACT_NONE, B, P.nd, W.inp, P.cdim, P.cdim, packed + K.mu0.f, params + P.mu0.b, mu0, st));
    return dense_fwd(ACT_NONE, B, P.nd, W.inp, P.cdim, P.cdim, packed + K.lv0.f, params + P.lv0.b, lv0, st);
  }
  // (the two draws are in W.eps0 / W.epsz: aux_vae_forward)  the trunk, aux_encode, z0, encode.fc
  static int encoder_fwd(Entry& e, const float* params, const float* packed, const float* x, int B, hipStream_t st) {
    auto& [P, K, ws, W] = e;
    ARDAE_TRY(stats_fwd(e, params, packed, x, B, W.mu0, W.lv0, st));
    ARDAE_TRY(launch_reparam_fwd(W.mu0, W.lv0, W.eps0, P.nd, B, P.nd, 1, W.z0, st));
    return cat_fwd(ACT_ELU, B, 1, P.cdim, W.inp, P.cdim, packed + K.efc.fi, params + P.efc.b, W.z0, P.nd, packed + K.efc.fn, W.rbh, W.hh, st);
  }
  // the auxiliary decoder on [ctx | z] and the pair KL, added into the head's KL rows; then the decoder (unfused: the backward reads its columns)
  static int decoder_fwd(Entry& e, const float* params, const float* packed, int B, hipStream_t st) {
    auto& [P, K, ws, W] = e;
    ARDAE_TRY(cat_fwd(ACT_ELU, B, 1, P.cdim, W.inp, P.cdim, packed + K.rfc.fi, params + P.rfc.b, W.z, P.zd, packed + K.rfc.fn, W.rb2, W.hr, st));
    ARDAE_TRY(dense_fwd(ACT_NONE, B, P.nd, W.hr, P.cdim, P.cdim, packed + K.meanp.f, params + P.meanp.b, W.mup, st));
    ARDAE_TRY(dense_fwd(ACT_NONE, B, P.nd, W.hr, P.cdim, P.cdim, packed + K.logvarp.f, params + P.logvarp.b, W.lvp, st));
    ARDAE_TRY(launch_pair_kld_rows(W.mu0, W.lv0, W.mup, W.lvp, B, P.nd, W.kld, 1, st));
    return res_decoder_fwd(P, K, params, packed, W.z, B, W, nullptr, st);
  }
  static GradMap grads_of(Entry& e, const float* params, const float* packed, float* g, float beta) { return grad_map(e.W, params, packed, g, beta); }
  static int decoder_bwd(Entry& e, const float* packed, int B, GradMap& gm, hipStream_t st) { return res_decoder_bwd(e.P, e.K, packed, e.W.z, e.W, B, gm, st); }
  // d ctx is the SUM of the three networks' parts, made before the trunk's backward: the auxiliary decoder's goes to dB0 (and dz = W.dzq + dhr Wz) ...
  static int aux_decoder_bwd(Entry& e, const float* packed, int B, GradMap&, hipStream_t st) {
    auto& [P, K, ws, W] = e;
    ARDAE_TRY(dense_bwd2(ACT_ELU, B, P.cdim, W.dmup, packed + K.meanp.b, W.dlvp, packed + K.logvarp.b, P.nd, W.hr, W.dhr, st));
    return cat_bwd(B, P.cdim, W.dhr, P.zd, packed + K.rfc.bn, W.dzq, W.dz, P.cdim, packed + K.rfc.bi, nullptr, W.dB0, st);
  }
  // ... encode.fc's joins it: dB1 = dB0 + dhh Wc ...
  static int encode_fc_bwd(Entry& e, const float* packed, int B, GradMap&, hipStream_t st) {
    auto& [P, K, ws, W] = e;
    ARDAE_TRY(dense_bwd2(ACT_ELU, B, P.cdim, W.dmu, packed + K.mean.b, W.dlv, packed + K.logvar.b, P.zd, W.hh, W.dhh, st));
    return cat_bwd(B, P.cdim, W.dhh, P.nd, packed + K.efc.bn, nullptr, W.dz0, P.cdim, packed + K.efc.bi, W.dB0, W.dB1, st);
  }
  // ... and the first head's two Linears (there is no clip in this family) go straight back into ctx.  The ten plain-Linear weight gradients, written
  // in place (no weight norm), go out as one list; the weight-normalised operators' block by block in the trunk's backward.
  static int aux_encoder_bwd(Entry& e, const float* packed, int B, GradMap& gm, hipStream_t st) {
    auto& [P, K, ws, W] = e;
    const int cd = P.cdim;
    { LinArgs A{}; A.Y = W.dinp; A.ldY = cd;
      ARDAE_TRY(lin2(EPI_ACT, ACT_NONE, B, cd, W.dmu0, P.nd, P.nd, packed + K.mu0.b, W.dlv0, P.nd, P.nd, packed + K.lv0.b, A, st)); }
    ARDAE_TRY(launch_axpy(W.dB1, (int64_t)B * cd, 1.f, W.dinp, st));
    WgradList wl(gm.grads, gm.grads_beta);
    wl.push(B, P.zd, cd, W.dmu, W.hh, cd, wl.g(P.mean.w), cd, wl.g(P.mean.b));
    wl.push(B, P.zd, cd, W.dlv, W.hh, cd, wl.g(P.logvar.w), cd, wl.g(P.logvar.b));
    cat_wgrads(wl, B, P.efc, cd, W.dhh, W.z0, W.inp);
    wl.push(B, P.nd, cd, W.dmu0, W.inp, cd, wl.g(P.mu0.w), cd, wl.g(P.mu0.b));
    wl.push(B, P.nd, cd, W.dlv0, W.inp, cd, wl.g(P.lv0.w), cd, wl.g(P.lv0.b));
    wl.push(B, P.nd, cd, W.dmup, W.hr, cd, wl.g(P.meanp.w), cd, wl.g(P.meanp.b));
    wl.push(B, P.nd, cd, W.dlvp, W.hr, cd, wl.g(P.logvarp.w), cd, wl.g(P.logvarp.b));
    cat_wgrads(wl, B, P.rfc, cd, W.dhr, W.z, W.inp);
    ARDAE_TRY(flush_wgrad(wl, W.wscratch, W.wscratch_floats, st));
    return res_trunk_wn_bwd(P, K, packed, W, B, gm, gm.grads_beta, st);
  }
  static void size_wgrads(Entry&, int) {}      // the carve has taken the weight-gradient scratch
  // the evaluation pass (aux_vae_iwae_draw, csrc/auxvae.h)
  using EvalWs = AuxResEvalWs;
  static void carve_eval(const AuxResLayout& P, const AuxResPacked&, Bump& ws, int B, int k, AuxResEvalWs& W) {
    res_trunk_carve(P, ws, B, W.T);
    W.carve_rows(ws, B, k, P.nd, P.zd, P.cdim, 1);
  }
  static int eval_prepare(const AuxResLayout&, const float* x, int, AuxResEvalWs&, const float*& xs, hipStream_t) {
    xs = x;
    return 0;
  }
  // stage 2 runs the trunk (params and packed are first at hand here); stage 3 reads its ctx again
  static int eval_hidden(const AuxResLayout& P, const AuxResPacked& K, const float* params, const float* packed, int stage, const float* xs, const float* s,
                         int B, int k, AuxResEvalWs& W, const float*& hid, hipStream_t st) {
    const Lin& l = stage == 2 ? P.efc : P.rfc;
    const LinPk& c = stage == 2 ? K.efc : K.rfc;
    hid = W.t[1];
    if (stage == 2) ARDAE_TRY(res_trunk_fwd(P, K, params, packed, xs, B, W.T, st));
    return cat_fwd(ACT_ELU, B, k, P.cdim, W.T.inp, P.cdim, packed + c.fi, params + l.b, s, l.in - P.cdim, packed + c.fn, W.rb, W.t[1], st);
  }
};

int auxresvae_decode(const ardae_model_desc& d, const float* params, const float* packed, const float* z, int R, float* workspace, size_t wsf, float* out0,
                     hipStream_t st, float*) {
  AuxResEntry entry(d, workspace, wsf, R, 2);
  auto& [P, K, ws, W] = entry;
  ARDAE_CHECK_ARG(ws.ok, "model_decode: workspace too small");
  return res_decoder_fwd(P, K, params, packed, z, R, W, out0, st, tail_fused_default(), mid_fused_default() ? packed + K.mid_w : nullptr);
}

}  // namespace

ResDecoderView auxresvae_decoder_view(const ardae_model_desc& d) {
  const AuxResLayout P(d);
  const AuxResPacked K(P);
  return {P, K, K.mid_w};
}

// (host pass only, as in csrc/resmodel.hip)
#ifndef __HIP_DEVICE_COMPILE__
static const GaussFamily AUXRESVAE_GAUSS = aux_gauss_family<AuxResVaeTraits>();
const Family AUXRESVAE_FAMILY = {auxresvae_desc_check, no_caps, family_param_floats<AuxResLayout, AuxResPacked>,
                                 family_packed_floats<AuxResLayout, AuxResPacked>, aux_workspace_floats<AuxResVaeTraits>, auxresvae_pack, vae_no_encode,
                                 auxresvae_decode, vae_no_forward, vae_no_backward, &AUXRESVAE_GAUSS};
#endif

}  // namespace ardae
