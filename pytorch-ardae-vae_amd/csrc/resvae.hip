// The resconv Gaussian-posterior baseline (vae.py --model resconv; ardae_model_desc.kind 12: MNISTResConvVAE, models/vae/resconv.py:26-241), joined
// from the residual-conv pieces of csrc/resmodel.h - no kernel of its own, and of the algorithm only what ResVaeTraits says (the rest is
// csrc/vaemodel.h's, shared by every Gaussian kind):
//   per image (B rows):  ctx = trunk(x or 2x - 1)  [B, c = h_dim];  mu, lv, z, kld: the plain Gaussian head encode.reparam.{mean_fn, logvar_fn} on it
//                        (no clip, one draw per image, the analytic KL of kinds 8 / 9 / 11);  logit = decoder(z);  recon = BCE-with-logits
// driven by the ardae_vae_* entry points (csrc/vaemodel.hip dispatches here), not by the sampler calls.  The decode-only path runs the decoder's last
// stage as resconv_tail_kernel (csrc/resmodel.hip).
#include "ardae_hip.h"
#include "common.h"
#include "resmodel.h"
#include "vaemodel.h"

namespace ardae {
namespace {

struct ResVaeLayout : ResLayout {
  Lin mu{}, lv{};                // encode.reparam.{mean,logvar}_fn on the trunk's output
  explicit ResVaeLayout(const ardae_model_desc& d) : ResLayout(d, d.h_dim) {
    ResWalk w;
    trunk_blocks(w);
    mu = w.lin(zd, cdim); lv = w.lin(zd, cdim);
    decoder_blocks(w);
    total = w.off;
  }
};
struct ResVaePacked : ResPacked {
  LinPk mu{}, lv{};
  ResVaePacked(const ResVaeLayout& P, PackList& pl) {
    ResPackWalk w{pl};
    trunk_panels(P, w);
    mu = w.lin(P.mu, 0); lv = w.lin(P.lv, 0);
    decoder_panels(P, w);
  }
  explicit ResVaePacked(const ResVaeLayout& P, PackList&& sizing = PackList()) : ResVaePacked(P, sizing) {}   // offsets only
};
struct ResVaeWs : ResWs {
  float *mu, *lv, *z, *eps, *kld, *dmu, *dlv;      // [B, zd]: the head's rows, the draw used, the KL rows [B], the head's backward seed
};

// mode 0: the trunk (encode_stats writes the caller's mu, lv); 1: forward + backward, one draw per image; 2: decode only on B rows - nothing is saved
// for a backward, and with the fused tail neither u28 nor dec[6]'s buffers exist
void carve(const ResVaeLayout& P, const ResVaePacked&, Bump& ws, int B, int mode, ResVaeWs& W) {
  const size_t b = (size_t)B;
  if (mode == 2) return res_decoder_carve(P, ws, b, DecRuns{true, !tail_fused_default(), false}, W);
  res_trunk_carve(P, ws, B, W);
  if (mode == 0) return;
  W.mu = ws.take(b * P.zd); W.lv = ws.take(b * P.zd); W.z = ws.take(b * P.zd); W.eps = ws.take(b * P.zd); W.kld = ws.take(b);
  W.dmu = ws.take(b * P.zd); W.dlv = ws.take(b * P.zd);
  res_decoder_carve(P, ws, b, DecRuns{true, true, true}, W);
  res_bwd_carve(P, ws, B, b, 2 * wgrad_scratch_floats(B, P.zd, P.cdim), W);      // the two heads, one batch
}
using ResVaeEntry = Entry<ResVaeLayout, ResVaePacked, ResVaeWs>;

// the descriptor rules of kind 12 (noise_dim 0, and the shared ones)
int resvae_desc_check(const ardae_model_desc* d) {
  ARDAE_CHECK_ARG(d->noise_dim == 0, "model: noise_dim must be 0 for kind 12 (the Gaussian posterior takes no noise input), got %d", d->noise_dim);
  return res_gauss_desc_check(d, "MNISTResConvVAE", "models/vae/resconv.py:145");
}

// one draw per image; there is no sampler pair.  mode 2: B * nz decoded rows
size_t resvae_workspace_floats(const ardae_model_desc& d, int B, int nz, int mode) {
  if (mode != 2 && (nz != 1 || mode == 3)) return 0;
  const ResVaeLayout P(d);
  Bump ws;
  ResVaeWs W;
  carve(P, ResVaePacked(P), ws, mode == 2 ? B * nz : B, mode, W);
  return ws.off;
}

int resvae_decode(const ardae_model_desc& d, const float* params, const float* packed, const float* z, int R, float* workspace, size_t wsf, float* out0,
                  hipStream_t st, float*) {
  ResVaeEntry entry(d, workspace, wsf, R, 2);
  auto& [P, K, ws, W] = entry;
  ARDAE_CHECK_ARG(ws.ok, "model_decode: workspace too small");
  return res_decoder_fwd(P, K, params, packed, z, R, W, out0, st, tail_fused_default());
}

// What gauss_vae_forward / _backward / _encode_stats (csrc/vaemodel.h) need to know of kind 12.
struct ResVaeTraits {
  using Layout = ResVaeLayout; using Packed = ResVaePacked; using Entry = ResVaeEntry;
  using Grads = GradMap;      // built before the decoder's backward, used again by the trunk's
  static Entry open(const ardae_model_desc& d, float* workspace, size_t wsf, int B, int mode) { return Entry(d, workspace, wsf, B, mode); }
  // The head at h = c_dim.  The recipe's 450 is no multiple of 4, so gauss_head_kernel reads its rows float by float there: measured at
  // 128 x 450 -> 2 x 32 it loses to the unfused launches (README), which are this kind's default; variant 1 stays callable.
  static GaussHead head_of(const ResVaeLayout& P, const ResVaePacked& K) { return GaussHead{P.cdim, P.zd, P.mu, P.lv, K.mu.f, K.lv.f, false, false}; }
  static const float* hid(const ResVaeWs& W) { return W.inp; }
  static GaussBufs bufs(const ResVaeWs& W) {      // the decoder's backward adds its dz to what the loss kernel left in dzq
    return {W.mu, W.lv, W.z, W.eps, W.kld, W.rec_row, W.pri_row, W.db[6].out, nullptr, W.dlogit, nullptr, W.dzq, W.dzq, W.dmu, W.dlv};
  }
  static int encoder_fwd(Entry& e, const float* params, const float* packed, const float* x, int B, hipStream_t st) {
    return res_trunk_fwd(e.P, e.K, params, packed, x, B, e.W, st);
  }
  // the training forward keeps the unfused tail: the backward reads the columns it saves
  static int decoder_fwd(Entry& e, const float* params, const float* packed, int B, hipStream_t st) {
    return res_decoder_fwd(e.P, e.K, params, packed, e.W.z, B, e.W, nullptr, st);
  }
  static GradMap grads_of(Entry& e, const float* params, const float* packed, float* g, float beta) { return grad_map(e.W, params, packed, g, beta); }
  static int decoder_bwd(Entry& e, const float* packed, int B, GradMap& gm, hipStream_t st) { return res_decoder_bwd(e.P, e.K, packed, e.W.z, e.W, B, gm, st); }
  static int encoder_bwd(Entry& e, const float* packed, const float*, int B, GradMap& gm, hipStream_t st) {
    auto& [P, K, ws, W] = e;
    // the two heads: plain Linears, their gradients go to the gradient buffer itself; then both back into the trunk's output rows
    WgradList wl(gm.grads, gm.grads_beta);
    wl.push(B, P.zd, P.cdim, W.dmu, W.inp, P.cdim, gm.grads + P.mu.w, P.cdim, gm.grads + P.mu.b);
    wl.push(B, P.zd, P.cdim, W.dlv, W.inp, P.cdim, gm.grads + P.lv.w, P.cdim, gm.grads + P.lv.b);
    ARDAE_TRY(flush_wgrad(wl, W.wscratch, W.wscratch_floats, st));
    { LinArgs A{}; A.Y = W.dinp; A.ldY = P.cdim;
      ARDAE_TRY(lin2(EPI_ACT, ACT_NONE, B, P.cdim, W.dmu, P.zd, P.zd, packed + K.mu.b, W.dlv, P.zd, P.zd, packed + K.lv.b, A, st)); }
    return res_trunk_wn_bwd(P, K, packed, W, B, gm, gm.grads_beta, st);
  }
};

}  // namespace

ResDecoderView resvae_decoder_view(const ardae_model_desc& d) {
  const ResVaeLayout P(d);
  return {P, ResVaePacked(P), 0};
}

// (host pass only, as in csrc/resmodel.hip)
#ifndef __HIP_DEVICE_COMPILE__
static const GaussFamily RESVAE_GAUSS = gauss_family<ResVaeTraits>();
const Family RESVAE_FAMILY = {resvae_desc_check, no_caps, family_param_floats<ResVaeLayout, ResVaePacked>, family_packed_floats<ResVaeLayout, ResVaePacked>,
                              resvae_workspace_floats, res_family_pack<ResVaeLayout, ResVaePacked>, vae_no_encode, resvae_decode, vae_no_forward,
                              vae_no_backward, &RESVAE_GAUSS};
#endif

}  // namespace ardae
