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
#include "auxconvvae.h"
#include "auxmodel.h"
#include "auxvae.h"
#include "convmodel.h"
#include "convvae.h"
#include "resmodel.h"
#include "vaemodel.h"
#include "ipmodel.h"
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

// ------------------------------------------------------------------------------------------------ kinds 0 / 1 as a family
// What the shared algorithm (csrc/ipmodel.h) needs to know of the MLP models: one trunk, two stacks.
struct MlpTraits : IpTraitsBase {
  using Layout = ModelLayout; using Packed = ModelPacked; using Ws = ModelWs; using Entry = MlpEntry;
  static constexpr bool mlp_decoder = true;
  static constexpr bool direct_z = true;      // a forward-only encode: the last stack layer writes the caller's buffer itself (one launch less)
  static int desc_check(const ardae_model_desc* d) { return mlp_desc_check(d, 0); }
  static unsigned caps(const ardae_model_desc& d) { return d.kind == 1 ? CAP_GAUSS_DECODER : 0; }
  static IpBufs bufs(const ModelWs& W) { return {W.z, W.D.o[0], W.D.o[1], W.D.dox[0], W.D.dox[1], W.D.dzq, W.D.dz, W.rec_row, W.pri_row}; }
  // every weight-gradient problem of the backward, with its scratch taken from ws (x: the images; noise: the sampler's draw)
  static void wgrads(const ModelLayout& P, const ModelPacked& K, const ModelWs& W, const float* x, const float* noise, int B, int nz, WgradList& wl, Bump& ws) {
    const int R = B * nz, h = P.h;
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
  // beside the carve: a zero-noise buffer for encode(std=0), or (encode_pair) the zero-noise stack's hidden rows and its zero noise block (B rows each)
  static size_t extra_floats(const ModelLayout& P, int B, int nz, int mode) {
    if (mode == 3) return (P.stack.size() - 1) * al64((size_t)B * P.h) + al64((size_t)B * P.nd);
    return al64((size_t)B * nz * P.nd);
  }
  static size_t noise_floats(const ModelLayout& P, int B, int nz) { return (size_t)B * nz * P.nd; }
  static float* zero_noise(Entry& e, size_t n) { return e.ws.take(n); }
  // fills W.e, W.rb, and (training forward) W.t, W.z
  static int sampler_fwd(Entry& e, const float* params, const float* packed, const float* x, const float* noise, int B, int nz, const IpEncodeOut* enc,
                         hipStream_t st) {
    ARDAE_TRY(encode_trunk(e.P, e.K, params, packed, x, B, e.W, st));
    return encode_stack(e.P, e.K, params, packed, noise, B, nz, e.W.rb, e.W.t, enc && enc->z_out ? enc->z_out : e.W.z, enc == nullptr, st);
  }
  static int decoder_fwd(Entry& e, const float* params, const float* packed, const float* z, int R, hipStream_t st) {
    return e.K.dec.fwd(params, packed, e.P.act, R, z, e.W.D.hid.data(), e.W.D.o, st);
  }
  static int decoder_bwd(Entry& e, const float* packed, int R, Grads&, hipStream_t st) { return e.K.dec.bwd(packed, e.P.act, R, e.W.D, st); }
  static int sampler_bwd(Entry& e, const float*, const float* packed, const float* x, const float* noise, int B, int nz, Grads& g, hipStream_t st) {
    auto& [P, K, ws, W] = e;
    const int R = B * nz, h = P.h, act = P.act;
    const size_t ns = P.stack.size(), ninp = P.inp.size();
    for (size_t i = ns - 1; i >= 1; --i)
      ARDAE_TRY(dense_bwd(act, R, h, (i == ns - 1) ? W.D.dz : W.dt[i + 1], P.stack[i].out, packed + K.sh_b[i], W.t[i], W.dt[i], st));
    ARDAE_TRY(launch_segment_sum(W.dt[1], h, B, nz, h, 1.0f, W.drb, h, st));
    ARDAE_TRY(dense_bwd(act, B, h, W.drb, h, packed + K.sh_b[0], W.e[ninp], W.de[ninp], st));
    ARDAE_TRY(K.inp.bwd(packed, act, B, W.e.data(), W.de.data(), st));
    // weight gradients: one batched launch
    WgradList wl(g.grads, g.beta);
    wgrads(P, K, W, x, noise, B, nz, wl, ws);
    ARDAE_CHECK_ARG(ws.ok, "model_vae_backward: internal workspace accounting error");
    return wl.launch(st);
  }
};

// ardae_model_encode_pair in one pass: z0 = encode(x, std=0) and z = forward_hidden(x, nz) share the per-image trunk
int mlp_encode_pair(const ardae_model_desc& d, const float* params, const float* packed, const float* x, const float* noise, int B, int nz,
                    float* workspace, size_t wsf, float* z0_out, float* z_out, int phase, hipStream_t st) {
  MlpEntry entry(d, workspace, wsf, B, nz, 0);
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

constexpr Family mlp_family() {
  Family f = ip_family<MlpTraits>();
  f.encode_pair = mlp_encode_pair;
  f.vae_backward_decoder = ip_vae_backward_decoder<MlpTraits>;
  f.vae_backward_sampler = ip_vae_backward_sampler<MlpTraits>;
  return f;
}
const Family MLP_FAMILY = mlp_family();

}  // namespace

// ------------------------------------------------------------------------------------------------ the families, by kind
// (host_util.h) the one table by kind; desc_ok() checks the kind against it
const Family* family_of(int kind) {
  static const Family* const by_kind[20] = {&MLP_FAMILY, &MLP_FAMILY, &CONV_FAMILY, &AUX_FAMILY, &AUXCONV_FAMILY, &RES_FAMILY, &RES_FAMILY, &AUX_FAMILY,
                                            &VAE_FAMILY, &VAE_FAMILY, nullptr, &CONVVAE_FAMILY, &RESVAE_FAMILY, nullptr, &AUXVAE_FAMILY,
                                            &AUXVAE_FAMILY, nullptr, &AUXCONVVAE_FAMILY, nullptr, &AUXRESVAE_FAMILY};      // 10, 13, 16 and 18 are not kinds
  return kind >= 0 && kind <= 19 ? by_kind[kind] : nullptr;
}

}  // namespace ardae

using namespace ardae;

// the number is a kind, then the family's own rules
static int desc_ok(const ardae_model_desc* d) {
  ARDAE_CHECK_ARG(d != nullptr, "model: desc is NULL");
  ARDAE_CHECK_ARG(family_of(d->kind) != nullptr,
                  "model: kind must be 0 (MNISTIPVAE), 1 (ToyIPVAE concat), 2 (ConvIPVAE), 3 (MNISTAuxIPVAE), 4 (MNISTConvAuxIPVAE), 5 (ResConvIPVAE), "
                  "6 (MNISTResConvAuxIPVAE), 7 (ToyAuxIPVAE), 8 (MNISTVAE), 9 (ToyVAE), 11 (MNISTConvVAE) or 12 (MNISTResConvVAE), or 14 (MNISTAuxVAE) or 15 (ToyAuxVAE), or 17 (MNISTConvAuxVAE), or 19 (MNISTResConvAuxVAE)");
  return family(d).desc_check(d);
}

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
  if (family(d).encode_pair)
    return family(d).encode_pair(*d, params, packed, x, noise, B, nz, workspace, workspace_floats_, z0_out, z_out, phase, (hipStream_t)stream);
  // no fused pair (conv / aux samplers): two passes over the same workspace
  if (phase != 2) ARDAE_TRY(ardae_model_encode(d, params, packed, x, nullptr, B, 1, workspace, workspace_floats_, z0_out, stream));
  if (phase == 1) return 0;
  return ardae_model_encode(d, params, packed, x, noise, B, nz, workspace, workspace_floats_, z_out, stream);
}

int ardae_model_encode_hidden_raw(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* raw0, int B,
                                  float* workspace, size_t workspace_floats_, float* z0_out, float* hidden_out, void* stream) {
  ARDAE_TRY(model_common(d, params, packed, x, B, 1, workspace, workspace_floats_, 0));
  ARDAE_CHECK_ARG(family(d).caps(*d) & CAP_HIDDEN_RAW, "model_encode_hidden_raw: the clipped aux-resconv class only (kind 6 + ARDAE_MODEL_CLIPPED)");
  ARDAE_CHECK_ARG(z0_out || hidden_out, "model_encode_hidden_raw: nothing to return");
  return family(d).encode(*d, params, packed, x, nullptr, B, 1, workspace, workspace_floats_, z0_out, hidden_out, (hipStream_t)stream, raw0);
}
int ardae_model_encode_hidden(const ardae_model_desc* d, const float* params, const float* packed, const float* x, int B, float* workspace,
                              size_t workspace_floats_, float* z0_out, float* hidden_out, void* stream) {
  ARDAE_TRY(model_common(d, params, packed, x, B, 1, workspace, workspace_floats_, 0));
  ARDAE_CHECK_ARG(family(d).caps(*d) & CAP_HIDDEN, "model_encode_hidden: the hidden1a context exists for the aux models only (kinds 3, 4, 6, 7)");
  ARDAE_CHECK_ARG(hidden_out, "model_encode_hidden: hidden_out is NULL");
  return family(d).encode(*d, params, packed, x, nullptr, B, 1, workspace, workspace_floats_, z0_out, hidden_out, (hipStream_t)stream, nullptr);   // z0_out may be NULL
}

int ardae_model_decode(const ardae_model_desc* d, const float* params, const float* packed, const float* z, int R, float* workspace,
                       size_t workspace_floats_, float* out0, float* out1, void* stream) {
  ARDAE_TRY(desc_ok(d));
  ARDAE_CHECK_ARG(params && packed && z && workspace && out0 && R > 0, "model_decode: bad arguments");
  ARDAE_CHECK_ARG(!(family(d).caps(*d) & CAP_GAUSS_DECODER) || out1, "model_decode: the Gaussian decoder needs out1 (logvar)");
  ARDAE_CHECK_ARG(workspace_floats_ >= family(d).workspace_floats(*d, R, 1, 2), "model_decode: workspace too small");
  return family(d).decode(*d, params, packed, z, R, workspace, workspace_floats_, out0, (hipStream_t)stream, out1);
}

int ardae_model_loss_rows(const ardae_model_desc* d, const float* out0, const float* out1, const float* x, const float* z, int rows,
                          int nz, float* recon_row, float* prior_row, void* stream) {
  ARDAE_TRY(desc_ok(d));
  return launch_vae_loss(family(d).caps(*d) & CAP_GAUSS_DECODER ? 1 : 0, out0, out1, x, z, rows, nz, d->input_dim, d->z_dim, 1.f, 0, 0.f, nullptr, recon_row, prior_row, nullptr,
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
  ARDAE_CHECK_ARG(family(d).vae_backward_decoder, "model_vae_backward_decoder: the conv model and the aux model have no split backward (use ardae_model_vae_backward)");
  return family(d).vae_backward_decoder(*d, params, packed, x, noise, B, nz, beta, dloss, workspace, workspace_floats_, (hipStream_t)stream);
}

static int vae_backward_sampler_entry(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* noise,
                                      int B, int nz, const float* dz_extra, DevFloat seed_scale, float* workspace, size_t workspace_floats_,
                                      float* grads, float grads_beta, void* stream) {
  ARDAE_TRY(model_common(d, params, packed, x, B, nz, workspace, workspace_floats_, 1));
  ARDAE_CHECK_ARG(noise && grads, "model_vae_backward_sampler: null pointer argument");
  ARDAE_CHECK_ARG(family(d).vae_backward_sampler, "model_vae_backward_sampler: the conv model and the aux model have no split backward (use ardae_model_vae_backward)");
  return family(d).vae_backward_sampler(*d, params, packed, x, noise, B, nz, dz_extra, seed_scale, workspace, workspace_floats_, grads, grads_beta,
                                        (hipStream_t)stream);
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
