// Implicit-posterior VAE (sampler + decoder + ELBO pieces) on gfx950, orchestrated from the K1 / K6w kernels.
//
// Reference: models/ivae/mnist.py (kind 0) and models/ivae/toy.py with enc_type='concat' (kind 1).  Both are
// described by one structure:
//   inp  MLP : n_inp Linear->act on B rows                     (mnist: input is 2x-1, n_inp = n_layers+2; toy: n_layers)
//   stack    : n_stack Linear over [hidden | noise] on R = B*nz rows, act on all but the last; the FIRST one's hidden
//              part is the per-image `inp` (computed once per image and added as a row bias - the reference expands it to
//              R rows, ivae/mnist.py:115-116), the noise part is missing where the reference does not concatenate
//              (mnist: stack = [h <- h|noise, z <- h];  toy: every layer h|noise, models/layers.py:717-722)
//   decoder  : n_dec Linear->act from z, then 1 (logits) or 2 (mean, logvar) linear heads
#include <vector>

#include "ardae_hip.h"
#include "common.h"
#include "auxmodel.h"
#include "convmodel.h"
#include "convvae.h"
#include "resmodel.h"
#include "vaemodel.h"
#include "elementwise.h"
#include "mlp.h"

namespace ardae {
namespace {

struct ModelLayout {
  int kind, D, nd, h, zd, nl, act;
  std::vector<Lin> inp, stack, dec, heads;
  std::vector<bool> stack_noise;   // does stack[i] take the noise concat?
  size_t total = 0;
  explicit ModelLayout(const ardae_model_desc& d)
      : kind(d.kind), D(d.input_dim), nd(d.noise_dim), h(d.h_dim), zd(d.z_dim), nl(d.n_layers), act(d.act) {
    size_t off = 0;
    auto add = [&](std::vector<Lin>& v, int out, int in) { v.push_back(next_lin(off, out, in)); };
    const int n_inp = kind == 0 ? nl + 2 : nl;
    for (int l = 0; l < n_inp; ++l) add(inp, h, l == 0 ? D : h);
    if (kind == 0) {
      add(stack, h, h + nd); stack_noise.push_back(true);
      add(stack, zd, h); stack_noise.push_back(false);
    } else {
      for (int l = 0; l < nl; ++l) { add(stack, h, h + nd); stack_noise.push_back(true); }
      add(stack, zd, h + nd); stack_noise.push_back(true);
    }
    const int n_dec = kind == 0 ? nl + 1 : nl;
    for (int l = 0; l < n_dec; ++l) add(dec, h, l == 0 ? zd : h);
    add(heads, D, h);
    if (kind == 1) add(heads, D, h);
    total = off;
  }
};

// offsets into the packed buffer, reserved (and, over a real PackList, filled) in this order
struct ModelPacked {
  MlpStack inp;
  std::vector<size_t> sh_f, sh_b, sn_f;
  MlpDecoder dec;
  ModelPacked(const ModelLayout& P, PackList& pl) : inp(P.inp.data(), P.inp.size(), pl) {
    const size_t ns = P.stack.size();
    sh_f.resize(ns); sh_b.resize(ns); sn_f.assign(ns, 0);
    for (size_t i = 0; i < ns; ++i) {           // [out, h | nd]: hidden columns both ways, noise columns forward
      const Lin& l = P.stack[i];
      pl.pair(l, sh_f[i], sh_b[i], 0, P.h);
      if (P.stack_noise[i]) sn_f[i] = pl.panel(l.w + P.h, l.in, l.out, P.nd, false);
    }
    dec = MlpDecoder(P.dec.data(), P.dec.size(), P.heads.data(), (int)P.heads.size(), pl);
  }
  explicit ModelPacked(const ModelLayout& P, PackList&& sizing = PackList()) : ModelPacked(P, sizing) {}   // offsets only
};

int desc_ok(const ardae_model_desc* d) {
  ARDAE_CHECK_ARG(d != nullptr, "model: desc is NULL");
  ARDAE_CHECK_ARG(family_of(d->kind) != nullptr,
                  "model: kind must be 0 (MNISTIPVAE), 1 (ToyIPVAE concat), 2 (ConvIPVAE), 3 (MNISTAuxIPVAE), 4 (MNISTConvAuxIPVAE), 5 (ResConvIPVAE), "
                  "6 (MNISTResConvAuxIPVAE), 7 (ToyAuxIPVAE), 8 (MNISTVAE), 9 (ToyVAE), 11 (MNISTConvVAE) or 12 (MNISTResConvVAE)");
  if (family(d).gauss) return family(d).gauss->desc_check(d);      // the Gaussian-posterior baselines: no noise input, their own rules
  ARDAE_CHECK_ARG((d->flags & ~(ARDAE_MODEL_NO_CENTER | ARDAE_MODEL_HEAD_MASK | ARDAE_MODEL_CLIPPED | ARDAE_MODEL_CLIP_MASK)) == 0 &&
                      ((d->kind == 5 || d->kind == 6) ? (d->flags & ARDAE_MODEL_CLIP_MASK) == 0
                                                      : ((d->kind == 3 || d->kind == 7) ? (d->flags & ~ARDAE_MODEL_CLIP_MASK) == 0 : d->flags == 0)),
                  "model: unknown flags %d (ARDAE_MODEL_NO_CENTER / the sampler-head bits / ARDAE_MODEL_CLIPPED: residual-conv kinds 5 / 6 only; "
                  "the log-variance clip codes: kinds 3 / 7 only)", d->flags);
  ARDAE_CHECK_ARG(((d->flags >> ARDAE_MODEL_CLIP_Z0_SHIFT) & 15) <= 10 && ((d->flags >> ARDAE_MODEL_CLIP_Z_SHIFT) & 15) <= 10, "model: unknown log-variance clip code");
  if ((d->kind == 5 || d->kind == 6)) {
    ARDAE_CHECK_ARG(d->input_dim == 784 && d->noise_dim >= 1 && d->z_dim >= 1 && d->h_dim >= 1 && d->act == ACT_ELU && (d->kind == 6 || (d->n_layers >= 1 && d->n_layers <= 4)),
                    "model: the residual-conv models are 28x28x1, ELU, and (kind 5) 1 .. 4 hidden layers in the sampler head");
    return 0;
  }
  if (d->kind == 2 || d->kind == 4) {
    ARDAE_CHECK_ARG(d->input_dim == 784 && d->noise_dim >= 1 && d->z_dim >= 1, "model: ConvIPVAE is hard-wired to 28x28x1 inputs (input_dim 784)");
    ARDAE_CHECK_ARG(d->act > ACT_NONE && d->act <= ACT_LAST, "model: unknown activation %d (relu, softplus, elu, tanh, leaky_relu, swish)", d->act);
    return 0;
  }
  ARDAE_CHECK_ARG(d->input_dim >= 1 && d->noise_dim >= 1 && d->h_dim >= 1 && d->z_dim >= 1 && d->n_layers >= 1 && d->n_layers <= 4,
                  "model: bad dimensions");
  ARDAE_CHECK_ARG(d->act > ACT_NONE && d->act <= ACT_LAST, "model: unknown activation %d (relu, softplus, elu, tanh, leaky_relu, swish)", d->act);
  return 0;
}

// saved activations (in `workspace`, same carving in forward and backward)
struct ModelWs {
  float* x2;
  std::vector<float*> e;    // e[l], l = 1..n_inp        [B,h]
  float* rb;                // per-image part of the first stack layer (+ its bias) [B,h]
  std::vector<float*> t;    // t[i], i = 1..n_stack-1    [R,h]
  float* z;                 // sampler output            [R,zd]
  MlpDecoder::Bufs D;       // the decoder's, forward and backward
  float *rec_row, *pri_row;
  // backward only
  std::vector<float*> dt, de;
  float* drb;
};

void carve(const ModelLayout& P, const ModelPacked& K, Bump& ws, int B, int nz, int mode, ModelWs& W) {
  const size_t R = (size_t)B * nz, h = P.h;
  W.x2 = ws.take((size_t)B * P.D);
  K.inp.carve(ws, B, W.e);
  W.rb = ws.take((size_t)B * h);
  W.t.assign(P.stack.size(), nullptr);
  for (size_t i = 1; i < P.stack.size(); ++i) W.t[i] = ws.take(R * h);
  W.z = ws.take(R * P.zd);
  if (mode == 0) return;
  K.dec.carve(ws, R, true, W.D);
  W.rec_row = ws.take(R); W.pri_row = ws.take(R);
  W.dt.assign(P.stack.size(), nullptr);
  for (size_t i = 1; i < P.stack.size(); ++i) W.dt[i] = ws.take(R * h);
  K.inp.carve(ws, B, W.de);
  W.drb = ws.take((size_t)B * h);
}
using MlpEntry = Entry<ModelLayout, ModelPacked, ModelWs>;

// every weight-gradient problem of the backward, with its scratch taken from ws (x: the images; noise: the sampler's draw)
void model_wgrads(const ModelLayout& P, const ModelPacked& K, const ModelWs& W, const float* x, const float* noise, int B, int R, WgradList& wl, Bump& ws) {
  const int h = P.h;
  const size_t ns = P.stack.size();
  K.dec.wgrads(wl, R, W.z, W.D);
  for (size_t i = 0; i < ns; ++i) {
    const Lin& L = P.stack[i];
    const float* G = (i == ns - 1) ? W.D.dz : W.dt[i + 1];
    if (i == 0) wl.push(B, L.out, h, W.drb, W.e[P.inp.size()], h, wl.g(L.w), L.in, nullptr);        // per-image hidden part
    else wl.push(R, L.out, h, G, W.t[i], h, wl.g(L.w), L.in, P.stack_noise[i] ? nullptr : wl.g(L.b));
    if (P.stack_noise[i]) wl.push(R, L.out, P.nd, G, noise, P.nd, wl.g(L.w + h), L.in, wl.g(L.b));   // noise part (+ bias)
  }
  K.inp.wgrads(wl, B, P.kind == 0 ? W.x2 : x, W.e.data(), W.de.data());
  wl.assign(ws, (int)(P.heads.size() + P.dec.size() + 2 * ns + P.inp.size()));   // the hint counts a noise part for every stack layer
}

// dry run of carve() and the weight-gradient list on a null arena (mode 0: the sampler's buffers only)
size_t workspace_floats(const ModelLayout& P, int B, int nz, int mode) {
  const ModelPacked K(P);
  Bump ws;
  ModelWs W;
  carve(P, K, ws, B, nz, mode, W);
  if (mode != 0) {
    WgradList wl(nullptr);
    model_wgrads(P, K, W, nullptr, nullptr, B, B * nz, wl, ws);
  }
  return ws.off;
}

// sampler trunk (once per image): inp_encode on B rows, then rb = inp . S_1[:, :h]^T + b_S1.  Fills W.e, W.rb.
int encode_trunk(const ModelLayout& P, const ModelPacked& K, const float* params, const float* packed, const float* x, int B,
                 ModelWs& W, hipStream_t st) {
  const int h = P.h;
  const float* x_in = x;
  if (P.kind == 0) {
    ARDAE_TRY(launch_affine(x, (int64_t)B * P.D, 2.f, -1.f, W.x2, st));
    x_in = W.x2;
  }
  ARDAE_TRY(K.inp.fwd(params, packed, P.act, B, x_in, W.e.data(), st));
  return dense_fwd(ACT_NONE, B, h, W.e[P.inp.size()], h, h, packed + K.sh_f[0], params + P.stack[0].b, W.rb, st);
}

// sampler stack on R = B*nz rows: layer 0 takes the per-image rb plus its noise part, the last layer writes zdst [R, zd]
// keep_hidden = false (encode / forward_hidden calls, which run under no_grad in the reference): the hidden rows t[] need not exist
int encode_stack(const ModelLayout& P, const ModelPacked& K, const float* params, const float* packed, const float* noise,
                 int B, int nz, const float* rb, const std::vector<float*>& t, float* zdst, bool keep_hidden, hipStream_t st) {
  const int R = B * nz, h = P.h, act = P.act;
  const size_t ns = P.stack.size();
  if (!keep_hidden && ns == 2 && P.stack_noise[0] && !P.stack_noise[1] && P.stack[0].out == h) {
    // noise -> h -> z with nothing else reading the hidden rows: one launch (linear_shortk.hip::sampler_tail_kernel)
    LinArgs A{}; A.M = R; A.Nout = h; A.act = act; A.nsrc = 1;
    A.rowbias = rb; A.rowbias_ld = h; A.rows_per_group = nz;
    A.src[0].x = noise; A.src[0].ld = P.nd; A.src[0].K = P.nd; A.src[0].wp = packed + K.sn_f[0];
    if (sampler_tail_eligible(A, P.stack[1].out))
      return launch_sampler_tail(A, packed + K.sh_f[1], params + P.stack[1].b, zdst, P.stack[1].out, P.stack[1].out, st);
  }
  for (size_t i = 0; i < ns; ++i) {
    const bool last = i + 1 == ns;
    const int out = P.stack[i].out;
    LinArgs A{}; A.Y = last ? zdst : t[i + 1]; A.ldY = out; A.M = R; A.Nout = out; A.act = last ? ACT_NONE : act;
    int n = 0;
    if (i == 0) {
      A.rowbias = rb; A.rowbias_ld = h; A.rows_per_group = nz;
    } else {
      A.bias = params + P.stack[i].b;
      A.src[n].x = t[i]; A.src[n].ld = h; A.src[n].K = h; A.src[n].wp = packed + K.sh_f[i]; ++n;
    }
    if (P.stack_noise[i]) {
      A.src[n].x = noise; A.src[n].ld = P.nd; A.src[n].K = P.nd; A.src[n].wp = packed + K.sn_f[i]; ++n;
    }
    A.nsrc = n;
    ARDAE_TRY(launch_linear(A, EPI_ACT, st));
  }
  return 0;
}

// sampler forward: fills W.e, W.rb, W.t, W.z (and copies z to z_out when given)
int encode_fwd(const ModelLayout& P, const ModelPacked& K, const float* params, const float* packed, const float* x,
               const float* noise, int B, int nz, ModelWs& W, float* z_out, bool keep_hidden, hipStream_t st) {
  ARDAE_TRY(encode_trunk(P, K, params, packed, x, B, W, st));
  if (z_out && !keep_hidden)     // forward-only: the last layer writes the caller's buffer itself (one launch less per encode)
    return encode_stack(P, K, params, packed, noise, B, nz, W.rb, W.t, z_out, false, st);
  ARDAE_TRY(encode_stack(P, K, params, packed, noise, B, nz, W.rb, W.t, W.z, keep_hidden, st));
  if (z_out) {
    ARDAE_TRY(launch_copy(W.z, (size_t)B * nz * P.zd, z_out, st));
  }
  return 0;
}

// extra floats of the encode_pair workspace: the zero-noise stack's hidden rows and its zero noise block (B rows each)
size_t encode_pair_extra(const ModelLayout& P, int B) {
  return (P.stack.size() - 1) * al64((size_t)B * P.h) + al64((size_t)B * P.nd);
}

// ------------------------------------------------------------------------------------------------ kinds 0 / 1 as a family
size_t mlp_workspace_floats(const ardae_model_desc& d, int B, int nz, int mode) {
  const ModelLayout P(d);
  if (mode == 2) return ModelPacked(P).dec.decode_floats((size_t)B * nz);
  if (mode == 3) return workspace_floats(P, B, nz, 0) + encode_pair_extra(P, B);   // ardae_model_encode_pair
  return workspace_floats(P, B, nz, mode) + (size_t)al64((size_t)B * nz * P.nd);   // + a zero-noise buffer for encode(std=0)
}

int mlp_encode(const ardae_model_desc& d, const float* params, const float* packed, const float* x, const float* noise, int B, int nz,
               float* workspace, size_t wsf, float* z_out, float*, hipStream_t st, const float*) {
  MlpEntry entry(d, workspace, wsf, B, nz, 0);
  auto& [P, K, ws, W] = entry;
  float* zero = noise ? nullptr : ws.take((size_t)B * nz * P.nd);
  ARDAE_CHECK_ARG(ws.ok, "model_encode: internal workspace accounting error");
  ARDAE_TRY(noise_or_zero(noise, zero, (size_t)B * nz * P.nd, st));
  return encode_fwd(P, K, params, packed, x, noise, B, nz, W, z_out, false, st);
}

int mlp_vae_forward(const ardae_model_desc& d, const float* params, const float* packed, const float* x, const float* noise, int B, int nz,
                    DevFloat beta, float* workspace, size_t wsf, float* z_out, float* losses, hipStream_t st) {
  MlpEntry entry(d, workspace, wsf, B, nz, 1);
  auto& [P, K, ws, W] = entry;
  ARDAE_CHECK_ARG(ws.ok, "model_vae_forward: internal workspace accounting error");
  const int R = B * nz;
  ARDAE_TRY(encode_fwd(P, K, params, packed, x, noise, B, nz, W, z_out, true, st));
  ARDAE_TRY(K.dec.fwd(params, packed, P.act, R, W.z, W.D.hid.data(), W.D.o, st));
  ARDAE_TRY(launch_vae_loss(P.kind, W.D.o[0], W.D.o[1], x, W.z, R, nz, P.D, P.zd, beta, 0, 0.f, nullptr, W.rec_row, W.pri_row, nullptr, nullptr, nullptr, st));
  return launch_vae_loss_finalize(W.rec_row, W.pri_row, R, beta, losses, st);
}

// phases: 1 = loss gradients + decoder backward up to dz (needs nothing from the cDAE), 2 = entropy seed + sampler backward +
// weight gradients, 3 = both.  With phases == 3 the (pre-scaled) seed enters through the loss kernel; with phases == 2 it is
// added to dz as seed_scale * dz_extra.
int vae_backward_impl(const ardae_model_desc& d, const float* params, const float* packed, const float* x, const float* noise,
                      int B, int nz, DevFloat beta, float dloss, const float* dz_extra, DevFloat seed_scale, float* workspace,
                      size_t workspace_floats_, float* grads, float grads_beta, int phases, hipStream_t st) {
  MlpEntry entry(d, workspace, workspace_floats_, B, nz, 1);
  auto& [P, K, ws, W] = entry;
  const int R = B * nz, h = P.h, act = P.act;
  const size_t ns = P.stack.size(), ninp = P.inp.size();
  const float gscale = dloss / (float)R;
  if (phases & 1) {
    ARDAE_TRY(launch_vae_loss(P.kind, W.D.o[0], W.D.o[1], x, W.z, R, nz, P.D, P.zd, beta, 1, gscale, phases == 3 ? dz_extra : nullptr, W.rec_row, W.pri_row,
                              W.D.dox[0], W.D.dox[1], W.D.dzq, st));
    ARDAE_TRY(K.dec.bwd(packed, act, R, W.D, st));
  }
  if (!(phases & 2)) return 0;
  if (phases == 2 && dz_extra) ARDAE_TRY(launch_axpy(dz_extra, (int64_t)R * P.zd, seed_scale, W.D.dz, st));   // + the entropy seed
  // sampler backward
  for (size_t i = ns - 1; i >= 1; --i)
    ARDAE_TRY(dense_bwd(act, R, h, (i == ns - 1) ? W.D.dz : W.dt[i + 1], P.stack[i].out, packed + K.sh_b[i], W.t[i], W.dt[i], st));
  ARDAE_TRY(launch_segment_sum(W.dt[1], h, B, nz, h, 1.0f, W.drb, h, st));
  ARDAE_TRY(dense_bwd(act, B, h, W.drb, h, packed + K.sh_b[0], W.e[ninp], W.de[ninp], st));
  ARDAE_TRY(K.inp.bwd(packed, act, B, W.e.data(), W.de.data(), st));
  // weight gradients: one batched launch
  WgradList wl(grads, grads_beta);
  model_wgrads(P, K, W, x, noise, B, R, wl, ws);
  ARDAE_CHECK_ARG(ws.ok, "model_vae_backward: internal workspace accounting error");
  return wl.launch(st);
}

int mlp_vae_backward(const ardae_model_desc& d, const float* params, const float* packed, const float* x, const float* noise, int B, int nz,
                     DevFloat beta, float dloss, const float* dz_extra, float* workspace, size_t wsf, float* grads, float grads_beta,
                     hipStream_t st) {
  return vae_backward_impl(d, params, packed, x, noise, B, nz, beta, dloss, dz_extra, 1.f, workspace, wsf, grads, grads_beta, 3, st);
}

const Family MLP_FAMILY = {family_param_floats<ModelLayout, ModelPacked>, family_packed_floats<ModelLayout, ModelPacked>, mlp_workspace_floats,
                           family_pack<ModelLayout, ModelPacked>, mlp_encode, mlp_decode<ModelLayout, ModelPacked>, mlp_vae_forward, mlp_vae_backward};

// ------------------------------------------------------------------------------------------------ the families, by kind
}  // namespace

// (host_util.h) the one table by kind; desc_ok() checks the kind against it
const Family* family_of(int kind) {
  static const Family* const by_kind[13] = {&MLP_FAMILY, &MLP_FAMILY, &CONV_FAMILY, &AUX_FAMILY, &AUXCONV_FAMILY, &RES_FAMILY, &RES_FAMILY, &AUX_FAMILY,
                                            &VAE_FAMILY, &VAE_FAMILY, nullptr, &CONVVAE_FAMILY, &RESVAE_FAMILY};      // 10 is not a kind
  return kind >= 0 && kind <= 12 ? by_kind[kind] : nullptr;
}

}  // namespace ardae

using namespace ardae;

extern "C" {

size_t ardae_model_param_floats(const ardae_model_desc* d) { return desc_ok(d) ? 0 : family(d).param_floats(*d); }
size_t ardae_model_packed_floats(const ardae_model_desc* d) { return desc_ok(d) ? 0 : family(d).packed_floats(*d); }
size_t ardae_model_workspace_floats(const ardae_model_desc* d, int B, int nz, int mode) {
  if (desc_ok(d) || B <= 0 || nz <= 0) return 0;
  return family(d).workspace_floats(*d, B, nz, mode);
}

int ardae_model_pack(const ardae_model_desc* d, const float* params, float* packed, void* stream) {
  ARDAE_TRY(desc_ok(d));
  ARDAE_CHECK_ARG(params && packed, "model_pack: null pointer");
  return family(d).pack(*d, params, packed, (hipStream_t)stream);
}

static int model_common(const ardae_model_desc* d, const float* params, const float* packed, const float* x, int B, int nz,
                        float* workspace, size_t wsf, int mode) {
  ARDAE_TRY(desc_ok(d));
  ARDAE_CHECK_ARG(params && packed && x && workspace, "model: null pointer argument");
  ARDAE_CHECK_ARG(B > 0 && nz > 0 && (int64_t)B * nz < (int64_t)1 << 30, "model: bad batch (B=%d nz=%d)", B, nz);
  const size_t need = ardae_model_workspace_floats(d, B, nz, mode);
  ARDAE_CHECK_ARG(wsf >= need, "model: workspace too small (%zu < %zu floats)", wsf, need);
  return 0;
}

int ardae_model_encode(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* noise,
                       int B, int nz, float* workspace, size_t workspace_floats_, float* z_out, void* stream) {
  ARDAE_TRY(model_common(d, params, packed, x, B, nz, workspace, workspace_floats_, 0));
  ARDAE_CHECK_ARG(z_out, "model_encode: z_out is NULL");
  return family(d).encode(*d, params, packed, x, noise, B, nz, workspace, workspace_floats_, z_out, nullptr, (hipStream_t)stream, nullptr);
}

int ardae_model_encode_pair(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* noise,
                            int B, int nz, float* workspace, size_t workspace_floats_, float* z0_out, float* z_out, int phase,
                            void* stream) {
  ARDAE_TRY(desc_ok(d));
  ARDAE_CHECK_ARG(phase >= 0 && phase <= 2, "model_encode_pair: phase must be 0 (all), 1 (trunk + z0) or 2 (N-row stack)");
  ARDAE_CHECK_ARG(params && packed && x && (noise || phase == 1) && workspace && z0_out && z_out, "model_encode_pair: null pointer argument");
  ARDAE_CHECK_ARG(B > 0 && nz > 0 && (int64_t)B * nz < (int64_t)1 << 30, "model_encode_pair: bad batch (B=%d nz=%d)", B, nz);
  ARDAE_CHECK_ARG(workspace_floats_ >= ardae_model_workspace_floats(d, B, nz, 3), "model_encode_pair: workspace too small");
  if (d->kind >= 2) {   // conv / aux samplers: two passes over the same workspace
    if (phase != 2) ARDAE_TRY(ardae_model_encode(d, params, packed, x, nullptr, B, 1, workspace, workspace_floats_, z0_out, stream));
    if (phase == 1) return 0;
    return ardae_model_encode(d, params, packed, x, noise, B, nz, workspace, workspace_floats_, z_out, stream);
  }
  hipStream_t st = (hipStream_t)stream;
  MlpEntry entry(*d, workspace, workspace_floats_, B, nz, 0);
  auto& [P, K, ws, W] = entry;
  std::vector<float*> t0(P.stack.size(), nullptr);
  for (size_t i = 1; i < P.stack.size(); ++i) t0[i] = ws.take((size_t)B * P.h);
  float* zero = ws.take((size_t)B * P.nd);
  ARDAE_CHECK_ARG(ws.ok, "model_encode_pair: internal workspace accounting error");
  if (phase != 2) {
    ARDAE_TRY(launch_fill(zero, (size_t)B * P.nd, 0.f, st));
    ARDAE_TRY(encode_trunk(P, K, params, packed, x, B, W, st));
    ARDAE_TRY(encode_stack(P, K, params, packed, zero, B, 1, W.rb, t0, z0_out, false, st));    // encode(x, std=0): the draw is multiplied by 0
  }
  if (phase != 1) ARDAE_TRY(encode_stack(P, K, params, packed, noise, B, nz, W.rb, W.t, z_out, false, st));   // forward_hidden(x, nz); W.rb from phase 1
  return 0;
}

int ardae_model_encode_hidden_raw(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* raw0, int B,
                                  float* workspace, size_t workspace_floats_, float* z0_out, float* hidden_out, void* stream) {
  ARDAE_TRY(model_common(d, params, packed, x, B, 1, workspace, workspace_floats_, 0));
  ARDAE_CHECK_ARG(d->kind == 6 && (d->flags & ARDAE_MODEL_CLIPPED), "model_encode_hidden_raw: the clipped aux-resconv class only (kind 6 + ARDAE_MODEL_CLIPPED)");
  ARDAE_CHECK_ARG(z0_out || hidden_out, "model_encode_hidden_raw: nothing to return");
  return family(d).encode(*d, params, packed, x, nullptr, B, 1, workspace, workspace_floats_, z0_out, hidden_out, (hipStream_t)stream, raw0);
}
int ardae_model_encode_hidden(const ardae_model_desc* d, const float* params, const float* packed, const float* x, int B, float* workspace,
                              size_t workspace_floats_, float* z0_out, float* hidden_out, void* stream) {
  ARDAE_TRY(model_common(d, params, packed, x, B, 1, workspace, workspace_floats_, 0));
  ARDAE_CHECK_ARG((d->kind == 3 || d->kind == 7) || d->kind == 4 || d->kind == 6, "model_encode_hidden: the hidden1a context exists for the aux models only (kinds 3, 4, 6, 7)");
  ARDAE_CHECK_ARG(hidden_out, "model_encode_hidden: hidden_out is NULL");
  return family(d).encode(*d, params, packed, x, nullptr, B, 1, workspace, workspace_floats_, z0_out, hidden_out, (hipStream_t)stream, nullptr);   // z0_out may be NULL
}

int ardae_model_decode(const ardae_model_desc* d, const float* params, const float* packed, const float* z, int R, float* workspace,
                       size_t workspace_floats_, float* out0, float* out1, void* stream) {
  ARDAE_TRY(desc_ok(d));
  ARDAE_CHECK_ARG(params && packed && z && workspace && out0 && R > 0, "model_decode: bad arguments");
  ARDAE_CHECK_ARG(d->kind != 1 || out1, "model_decode: the Gaussian decoder needs out1 (logvar)");
  ARDAE_CHECK_ARG(workspace_floats_ >= family(d).workspace_floats(*d, R, 1, 2), "model_decode: workspace too small");
  return family(d).decode(*d, params, packed, z, R, workspace, workspace_floats_, out0, (hipStream_t)stream, out1);
}

int ardae_model_loss_rows(const ardae_model_desc* d, const float* out0, const float* out1, const float* x, const float* z, int rows,
                          int nz, float* recon_row, float* prior_row, void* stream) {
  ARDAE_TRY(desc_ok(d));
  return launch_vae_loss(d->kind == 1 || d->kind == 7 || d->kind == 9 ? 1 : 0, out0, out1, x, z, rows, nz, d->input_dim, d->z_dim, 1.f, 0, 0.f, nullptr, recon_row, prior_row, nullptr,
                         nullptr, nullptr, (hipStream_t)stream);
}

// The four entry points that take beta or the seed factor, each written once: the ABI's value form passes the float, its _dev twin
// the train state's slot (DevFloat).
static int vae_forward_entry(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* noise, int B,
                             int nz, DevFloat beta, float* workspace, size_t workspace_floats_, float* z_out, float* losses, void* stream) {
  ARDAE_TRY(model_common(d, params, packed, x, B, nz, workspace, workspace_floats_, 1));
  ARDAE_CHECK_ARG(noise && z_out && losses, "model_vae_forward: null pointer argument");
  return family(d).vae_forward(*d, params, packed, x, noise, B, nz, beta, workspace, workspace_floats_, z_out, losses, (hipStream_t)stream);
}

static int vae_backward_entry(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* noise, int B,
                              int nz, DevFloat beta, float dloss, const float* dz_extra, float* workspace, size_t workspace_floats_,
                              float* grads, float grads_beta, void* stream) {
  ARDAE_TRY(model_common(d, params, packed, x, B, nz, workspace, workspace_floats_, 1));
  ARDAE_CHECK_ARG(noise && grads, "model_vae_backward: null pointer argument");
  return family(d).vae_backward(*d, params, packed, x, noise, B, nz, beta, dloss, dz_extra, workspace, workspace_floats_, grads, grads_beta,
                                (hipStream_t)stream);
}

static int vae_backward_decoder_entry(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* noise,
                                      int B, int nz, DevFloat beta, float dloss, float* workspace, size_t workspace_floats_, void* stream) {
  ARDAE_TRY(model_common(d, params, packed, x, B, nz, workspace, workspace_floats_, 1));
  ARDAE_CHECK_ARG(noise, "model_vae_backward_decoder: null pointer argument");
  ARDAE_CHECK_ARG(d->kind < 2, "model_vae_backward_decoder: the conv model and the aux model have no split backward (use ardae_model_vae_backward)");
  return vae_backward_impl(*d, params, packed, x, noise, B, nz, beta, dloss, nullptr, 0.f, workspace, workspace_floats_, nullptr, 0.f, 1,
                           (hipStream_t)stream);
}

static int vae_backward_sampler_entry(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* noise,
                                      int B, int nz, const float* dz_extra, DevFloat seed_scale, float* workspace, size_t workspace_floats_,
                                      float* grads, float grads_beta, void* stream) {
  ARDAE_TRY(model_common(d, params, packed, x, B, nz, workspace, workspace_floats_, 1));
  ARDAE_CHECK_ARG(noise && grads, "model_vae_backward_sampler: null pointer argument");
  ARDAE_CHECK_ARG(d->kind < 2, "model_vae_backward_sampler: the conv model and the aux model have no split backward (use ardae_model_vae_backward)");
  return vae_backward_impl(*d, params, packed, x, noise, B, nz, 0.f, 0.f, dz_extra, seed_scale, workspace, workspace_floats_, grads,
                           grads_beta, 2, (hipStream_t)stream);
}

int ardae_model_vae_forward(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* noise,
                            int B, int nz, float beta, float* workspace, size_t workspace_floats_, float* z_out, float* losses,
                            void* stream) {
  return vae_forward_entry(d, params, packed, x, noise, B, nz, beta, workspace, workspace_floats_, z_out, losses, stream);
}
int ardae_model_vae_forward_dev(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* noise,
                                int B, int nz, const void* state, float* workspace, size_t workspace_floats_, float* z_out, float* losses,
                                void* stream) {
  ARDAE_CHECK_ARG(state, "model_vae_forward_dev: state is NULL");
  return vae_forward_entry(d, params, packed, x, noise, B, nz, train_state_beta(state), workspace, workspace_floats_, z_out, losses, stream);
}

int ardae_model_vae_backward(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* noise,
                             int B, int nz, float beta, float dloss, const float* dz_extra, float* workspace,
                             size_t workspace_floats_, float* grads, float grads_beta, void* stream) {
  return vae_backward_entry(d, params, packed, x, noise, B, nz, beta, dloss, dz_extra, workspace, workspace_floats_, grads, grads_beta, stream);
}
int ardae_model_vae_backward_dev(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* noise,
                                 int B, int nz, const void* state, float dloss, const float* dz_extra, float* workspace,
                                 size_t workspace_floats_, float* grads, float grads_beta, void* stream) {
  ARDAE_CHECK_ARG(state, "model_vae_backward_dev: state is NULL");
  return vae_backward_entry(d, params, packed, x, noise, B, nz, train_state_beta(state), dloss, dz_extra, workspace, workspace_floats_, grads,
                            grads_beta, stream);
}

int ardae_model_vae_backward_decoder(const ardae_model_desc* d, const float* params, const float* packed, const float* x,
                                     const float* noise, int B, int nz, float beta, float dloss, float* workspace,
                                     size_t workspace_floats_, void* stream) {
  return vae_backward_decoder_entry(d, params, packed, x, noise, B, nz, beta, dloss, workspace, workspace_floats_, stream);
}
int ardae_model_vae_backward_decoder_dev(const ardae_model_desc* d, const float* params, const float* packed, const float* x,
                                         const float* noise, int B, int nz, const void* state, float dloss, float* workspace,
                                         size_t workspace_floats_, void* stream) {
  ARDAE_CHECK_ARG(state, "model_vae_backward_decoder_dev: state is NULL");
  return vae_backward_decoder_entry(d, params, packed, x, noise, B, nz, train_state_beta(state), dloss, workspace, workspace_floats_, stream);
}

int ardae_model_vae_backward_sampler(const ardae_model_desc* d, const float* params, const float* packed, const float* x,
                                     const float* noise, int B, int nz, const float* dz_extra, float seed_scale, float* workspace,
                                     size_t workspace_floats_, float* grads, float grads_beta, void* stream) {
  return vae_backward_sampler_entry(d, params, packed, x, noise, B, nz, dz_extra, seed_scale, workspace, workspace_floats_, grads, grads_beta,
                                    stream);
}
int ardae_model_vae_backward_sampler_dev(const ardae_model_desc* d, const float* params, const float* packed, const float* x,
                                         const float* noise, int B, int nz, const float* dz_extra, const void* state, float* workspace,
                                         size_t workspace_floats_, float* grads, float grads_beta, void* stream) {
  ARDAE_CHECK_ARG(state, "model_vae_backward_sampler_dev: state is NULL");
  return vae_backward_sampler_entry(d, params, packed, x, noise, B, nz, dz_extra, train_state_seed_scale(state), workspace, workspace_floats_,
                                    grads, grads_beta, stream);
}

}  // extern "C"
