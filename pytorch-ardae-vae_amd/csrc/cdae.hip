// AR-DAE update on gfx950, conditional (ardae_cdae_desc.kind 0 / 1; 16 / 17 without an input encoder), unconditional (kind 2 / 3), plain DAE (kind 6 / 7) and plain conditional DAE
// (kind 10 / 11 / 13): forward, score pass, DAE loss, double backward and weight gradients, orchestrated on the host from the K1 (linear.hip) / K6w (wgrad.hip) kernels.
//
// Maths: SURVEY.md Appendix A (closed form of models/graddae/mlp.py:400-444 under autograd), notation below.
//   rows i=1..N (N = B*S), image b(i) = i / S
//   inp_encode : a_0 = xbar, a_l = sp(A_l a_{l-1} + b_l)                      l = 1..L        (N rows)
//   ctx_encode : c_0 = ctx,  c_l = sp(C_l c_{l-1} + bc_l)                     l = 1..L        (B rows, ONCE per image)
//   energy MLP : h_1 = sp(W1a a_L + [W1c c_L + d_1](b) + sigma w1s), h_l = sp(W_l h_{l-1} + d_l), E = w.h_L + d_f
//   score      : e_L = -w (.) s(h_L); e_{l-1} = (e_l W_l) (.) s(h_{l-1}); r_L = (e_1 W1a) (.) s(a_L);
//                r_{l-1} = (r_l A_l) (.) s(a_{l-1});  g = r_1 A_1          [s(.) = softplus' rebuilt from the saved output]
//   loss       : rho = sigma g + eps; loss = sum rho^2 / (N z); gbar = 2 sigma rho / (N z)
//   forward-mode chain (the create_graph half of the double backward):
//                rb_1 = gbar A_1^T; tau_l = rb_l (.) s(a_l); pbar_l = rb_l (.) r_l (.) (1 - s(a_l)); rb_{l+1} = tau_l A_{l+1}^T
//                eb_1 = tau_L W1a^T; tau'_l = eb_l (.) s(h_l); qbar_l = eb_l (.) e_l (.) (1 - s(h_l)); eb_{l+1} = tau'_l W_{l+1}^T
//   ordinary backward seeded by qbar/pbar:
//                qhat_L = qbar_L; qhat_{l-1} = qbar_{l-1} + (qhat_l W_l) (.) s(h_{l-1});
//                phat_L = pbar_L + (qhat_1 W1a) (.) s(a_L); phat_{l-1} = pbar_{l-1} + (phat_l A_l) (.) s(a_{l-1})
//                ctx branch: Qsum_b = sum_{i in b} qhat_1[i]  (reduce over S BEFORE the ctx chain), chat_L = (Qsum W1c) (.) s(c_L) ...
//   weight gradients (one batched launch): see cdae_wgrads().
//   res kinds (1 / 3: direct score, g = fc(h_L) + d_f): no score pass and no forward-mode chain, one ordinary backward from gbar.
//
// The unconditional kinds (models/graddae/mlp.py:118-207, models/resdae/mlp.py:92-167) are the special case without the two encoders:
// the energy MLP reads the input itself, a_L := xbar, so W1a [h, h] becomes W1x [h, z] and the per-image bias [W1c c_L + d_1](b) the
// plain d_1.  Every line above that names A_l, C_l, a_l (l < L), c_l, r_l, tau_l, pbar_l, phat_l or Qsum drops out:
//   g = e_1 W1x;  eb_1 = gbar W1x^T;  W1x's gradient = e_1 (x) gbar + qhat_1 (x) xbar.
// The plain DAEs (kinds 6 / 7; models/graddae/mlp.py:39-116, models/resdae/mlp.py:27-90) are the unconditional kinds whose network does not see
// sigma: W1 = W1x [h, z], no w1s, h_1 = sp(W1x xbar + d_1).  The loss keeps its per-row sigma.
// The plain conditional DAEs (kinds 10 / 11; models/graddae/mlp.py:210-339, models/resdae/mlp.py:170-284) relate to kinds 0 / 1 as 6 / 7 do to 2 / 3:
// W1 = [W1a | W1c] [h, 2h], no w1s, h_1 = sp(W1a a_L + [W1c c_L + d_1](b)).  The loss keeps its per-row sigma.
// The conditional DAE without an input encoder (kind 13; models/dae/mlp.py:85-193 with enc_input=False) is kind 11 whose energy MLP reads the
// perturbed rows themselves beside the encoded context: a_L := xbar, W1 = [W1x | W1c] [h, z + h], h_1 = sp(W1x xbar + [W1c c_L + d_1](b)).  Every line
// that names A_l, a_l or phat_l drops out: one ordinary backward from gbar, W1x's gradient = qhat_1 (x) xbar, W1c's through Qsum as before.
// (Kinds 7 / 11 / 13 also serve the reconstruction DAEs of models/dae/mlp.py: with sigma = 1 and eps = -x the loss layer's rho is y - x.)
// The conditional AR-DAEs without an input encoder (kinds 16 / 17; models/graddae/mlp.py:341-483, models/resdae/mlp.py:286-413 with enc_input=False)
// are kinds 0 / 1 whose energy MLP reads the perturbed rows themselves: a_L := xbar, W1 = [W1x | W1c | w1s] [h, z + h + 1],
// h_1 = sp(W1x xbar + [W1c c_L + d_1](b) + sigma w1s).  Every line that names A_l, a_l (l < L), r_l, tau_l, pbar_l or phat_l drops out.  Kind 17 is to
// kind 1 what kind 13 is to kind 11: one ordinary backward from gbar.  Kind 16 is the unconditional kind 2's update (g = e_1 W1x, eb_1 = gbar W1x^T,
// W1x's gradient = e_1 (x) gbar + qhat_1 (x) xbar) with the per-image bias in layer 1 and the ctx branch seeded by Qsum = sum_S qhat_1, which holds
// the first- and the second-order term as kind 0's does.  Launch decisions: kind 17 follows kind 13 (the backward layer by layer, the split hint
// 3L + 1), kind 16 kind 0 for the context chain, the ctx branch and the split hint, and kind 2 for the N-row runs; its N == B score takes the
// general path (the one-launch chain of kind 0 walks the input encoder).
// In the code: `cond` marks what exists for kinds 0 / 1 / 10 / 11 / 13 / 16 / 17 only, `enc_inp` the input encoder (cond without kinds 13 / 16 / 17),
// `grad` what the energy kinds (0 / 2 / 6 / 10 / 16) add to the res kinds, `has_sigma` the sigma column of W1 (kinds 0 - 3, 16, 17).
#include <vector>

#include "ardae_hip.h"
#include "common.h"
#include "elementwise.h"
#include "host_util.h"

namespace ardae {
namespace {

bool cond_kind(int kind) { return kind < 2 || kind == 10 || kind == 11 || kind == 13 || kind == 16 || kind == 17; }
bool input_encoder_kind(int kind) { return kind < 2 || kind == 10 || kind == 11; }
bool sigma_column_kind(int kind) { return kind < 4 || kind == 16 || kind == 17; }

struct CdaeLayout {
  int kind, z, c, h, L, act;
  bool cond, enc_inp, grad, has_sigma;
  std::vector<Lin> ctx, inp, neg;   // ctx (cond) / inp (enc_inp): L linears (L-1 hidden + fc); neg: L hidden + fc (= neglogprob / dae / main)
  size_t total = 0;
  // W1 = neg[0] is [W1a | W1c | w1s] (enc_inp), [W1x | W1c] (kind 13), [W1x | W1c | w1s] (kinds 16 / 17) or [W1x | w1s]: its N-row panel has k1 columns, then (cond) W1c's h, then
  // (has_sigma) the sigma column
  int k1() const { return enc_inp ? h : z; }
  int sigma_col() const { return cond ? k1() + h : z; }

  explicit CdaeLayout(const ardae_cdae_desc& d)
      : kind(d.kind), z(d.input_dim), c(d.context_dim), h(d.h_dim), L(d.n_layers), act(d.act), cond(cond_kind(d.kind)), enc_inp(input_encoder_kind(d.kind)), grad(d.kind % 2 == 0), has_sigma(sigma_column_kind(d.kind)) {
    size_t off = 0;
    auto add = [&](std::vector<Lin>& v, int out, int in) { v.push_back(next_lin(off, out, in)); };
    if (cond)
      for (int l = 0; l < L; ++l) add(ctx, h, l == 0 ? c : h);
    if (enc_inp)
      for (int l = 0; l < L; ++l) add(inp, h, l == 0 ? z : h);
    for (int l = 0; l < L; ++l) add(neg, h, l == 0 ? sigma_col() + (has_sigma ? 1 : 0) : h);
    add(neg, grad ? 1 : z, h);
    total = off;
  }
};

// offsets into the packed-weight buffer
struct PackedLayout {
  std::vector<size_t> ctx_f, ctx_b, inp_f, inp_b, neg_f, neg_b;   // ctx: cond only, inp: enc_inp only; neg_*[0] unused (W1 is split below)
  size_t w1_f, w1_b, w1c_f, w1c_b, w1s;                           // w1: W1's N-row panel (W1a | W1x); w1c: cond only; w1s: has_sigma only
  size_t fc_f, fc_b;   // res kinds only (dae.fc / main.fc [z,h])
  PackedLayout(const CdaeLayout& P, PackList& pl) {
    const size_t L = P.L;
    for (auto* v : {&ctx_f, &ctx_b, &inp_f, &inp_b, &neg_f, &neg_b}) v->assign(L, 0);
    if (P.cond)
      for (size_t l = 0; l < L; ++l) { pl.pair(P.ctx[l], ctx_f[l], ctx_b[l]); if (P.enc_inp) pl.pair(P.inp[l], inp_f[l], inp_b[l]); }
    const Lin& W1 = P.neg[0];
    pl.pair(W1, w1_f, w1_b, 0, P.k1());
    w1c_f = w1c_b = 0;
    if (P.cond) pl.pair(W1, w1c_f, w1c_b, P.k1(), P.h);
    w1s = P.has_sigma ? pl.take(P.h) : 0;            // the sigma column, gathered by cdae_pack_impl
    for (size_t l = 1; l < L; ++l) pl.pair(P.neg[l], neg_f[l], neg_b[l]);
    fc_f = fc_b = 0;
    if (!P.grad) pl.pair(P.neg[L], fc_f, fc_b);
  }
  explicit PackedLayout(const CdaeLayout& P, PackList&& sizing = PackList()) : PackedLayout(P, sizing) {}   // offsets only
};

int desc_ok(const ardae_cdae_desc* d) {
  ARDAE_CHECK_ARG(d != nullptr, "cdae: desc is NULL");
  ARDAE_CHECK_ARG((d->kind >= 0 && d->kind <= 3) || d->kind == 6 || d->kind == 7 || d->kind == 10 || d->kind == 11 || d->kind == 13 || d->kind == 16 || d->kind == 17,
                  "cdae: kind must be 0 (mlp-grad), 1 (mlp-res), 2 (unconditional grad), 3 (unconditional res), 6 (plain DAE grad), 7 (plain DAE res), "
                  "10 (plain conditional DAE grad), 11 (plain conditional DAE res), 13 (conditional DAE without an input encoder), "
                  "16 (mlp-grad without an input encoder) or 17 (mlp-res without an input encoder)");
  ARDAE_CHECK_ARG(!cond_kind(d->kind) || d->context_dim >= 1, "cdae: kinds 0 / 1 / 10 / 11 / 13 / 16 / 17 need context_dim >= 1 (got %d)", d->context_dim);
  ARDAE_CHECK_ARG(cond_kind(d->kind) || d->context_dim == 0, "cdae: kinds 2 / 3 / 6 / 7 have no context: context_dim must be 0 (got %d)", d->context_dim);
  ARDAE_CHECK_ARG(d->input_dim >= 1 && d->h_dim >= 1 && d->n_layers >= 1, "cdae: bad dimensions");
  ARDAE_CHECK_ARG(d->n_layers <= 6, "cdae: n_layers <= 6 supported (3L+1 gradient problems per batch)");
  // every activation of get_nonlinear_func; with a piecewise linear one mlp-grad's second-order terms vanish, as
  // they do under autograd in the reference
  ARDAE_CHECK_ARG(d->act > ACT_NONE && d->act <= ACT_LAST, "cdae: unknown activation %d", d->act);
  return 0;
}

// the workspace of cdae_impl: forward / score-pass buffers, then (need_grads) the double backward's
struct CdaeWs {
  std::vector<float*> cL, a, hh, e, r, tau, taup, pbar, qbar, chat;   // [l], l = 1..L; cL / chat: [B, h], the rest [N, h]
  float *cb, *gbar, *gbuf, *tile_loss, *chain_cnt, *Qsum, *cs_taup;
  int ltiles, ctiles;
};

// Kinds 0 / 1 / 10 / 11 take every buffer whichever of the two reads it (kinds 1 / 11 leave e, r, tau, tau', pbar and cs_taup unused); kinds 13 /
// 16 / 17 and the unconditional kinds take what they read, so hh[1] is the first N-row piece of the arena (the fused front ends fill it).
void cdae_carve(const CdaeLayout& P, Bump& ws, int B, int S, bool need_grads, CdaeWs& W) {
  const int N = B * S, h = P.h, L = P.L, z = P.z;
  const size_t Bh = (size_t)B * h, Nh = (size_t)N * h;
  const bool cond = P.cond, enc = P.enc_inp, score = enc || P.grad;
  for (auto* v : {&W.cL, &W.a, &W.hh, &W.e, &W.r, &W.tau, &W.taup, &W.pbar, &W.qbar, &W.chat}) v->assign(L + 1, nullptr);
  W.cb = W.chain_cnt = W.Qsum = W.cs_taup = nullptr;
  if (cond) {
    for (int l = 1; l <= L; ++l) W.cL[l] = ws.take(Bh);
    W.cb = ws.take(Bh);
  }
  for (int l = 1; l <= L; ++l) {
    if (enc) W.a[l] = ws.take(Nh);
    W.hh[l] = ws.take(Nh);
    if (score) W.e[l] = ws.take(Nh);
    if (enc) W.r[l] = ws.take(Nh);
  }
  if (need_grads)
    for (int l = 1; l <= L; ++l) {
      if (enc) W.tau[l] = ws.take(Nh);
      if (score) W.taup[l] = ws.take(Nh);
      if (enc) W.pbar[l] = ws.take(Nh);
      W.qbar[l] = ws.take(Nh);
    }
  W.gbar = ws.take((size_t)N * z);
  W.gbuf = ws.take((size_t)N * z);
  W.ltiles = linear_row_tiles(N, z) * linear_col_panels(N, z);
  W.tile_loss = ws.take(W.ltiles);
  if (enc) W.chain_cnt = ws.take((size_t)LINEAR_SMALL_CHAIN_COUNTER_WORDS * ((N + 15) / 16));   // row-block counters of the per-image chain launch (score pass)
  W.ctiles = linear_row_tiles(N, h);
  if (!need_grads) return;
  if (cond) {
    W.Qsum = ws.take(Bh);
    for (int l = 1; l <= L; ++l) W.chat[l] = ws.take(Bh);
  }
  if (score) W.cs_taup = ws.take((size_t)W.ctiles * h);                                           // colsum of tau'_L
}

// every weight-gradient problem of the update (one batched launch), with its scratch taken from ws
// (qhat_l / phat_l live in qbar_l / pbar_l: the backward overwrites them in place)
void cdae_wgrads(const CdaeLayout& P, const CdaeWs& W, const float* xbar, const float* sigma, const float* ctx, int B, int S, WgradList& wl, Bump& ws) {
  const int N = B * S, h = P.h, L = P.L, z = P.z;
  const std::vector<float*>&a = W.a, &hh = W.hh, &e = W.e, &r = W.r, &tau = W.tau, &taup = W.taup, &qhat = W.qbar, &phat = W.pbar;
  const int ld1 = P.neg[0].in;
  const size_t gW1 = P.neg[0].w;
  // One N-row layer's weight [h, I] and bias.  grad kinds: s (x) t of the score pass + ghat (x) x of the backward; res kinds: the second term
  // alone; the bias gradient is ghat's column sums.  first: W1's N-row panel, which (has_sigma) also yields w1s = sum_i sigma_i ghat[i]
  auto push = [&](const Lin& lin, int I, const float* s, const float* t, const float* ghat, const float* x, bool first) {
    const bool scol = first && P.has_sigma;
    const float* rs = scol ? sigma : nullptr;
    float* out_rs = scol ? wl.g(gW1 + P.sigma_col()) : nullptr;
    const int ld = first ? ld1 : I, ld_rs = scol ? ld1 : 0;
    if (P.grad) wl.push2(N, h, I, s, t, I, ghat, x, I, 1, rs, wl.g(lin.w), ld, wl.g(lin.b), out_rs, ld_rs);
    else wl.push2(N, h, I, ghat, x, I, nullptr, nullptr, 0, 0, rs, wl.g(lin.w), ld, wl.g(lin.b), out_rs, ld_rs);
  };
  if (P.enc_inp)
    for (int l = 1; l <= L; ++l)   // inp A_l: r_l (x) tau_{l-1}  +  phat_l (x) a_{l-1}   (tau_0 = gbar, a_0 = xbar)
      push(P.inp[l - 1], l == 1 ? z : h, r[l], l == 1 ? W.gbar : tau[l - 1], phat[l], l == 1 ? xbar : a[l - 1], false);
  push(P.neg[0], P.k1(), e[1], P.enc_inp ? tau[L] : W.gbar, qhat[1], P.enc_inp ? a[L] : xbar, true);                                  // W1a | W1x, d_1, w1s
  if (P.cond) wl.push2(B, h, h, W.Qsum, W.cL[L], h, nullptr, nullptr, 0, -1, nullptr, wl.g(gW1 + P.k1()), ld1, nullptr, nullptr, 0);   // W1c
  for (int l = 2; l <= L; ++l)     // W_l: e_l (x) tau'_{l-1} + qhat_l (x) h_{l-1}
    push(P.neg[l - 1], h, e[l], taup[l - 1], qhat[l], hh[l - 1], false);
  if (!P.grad) wl.push2(N, z, h, W.gbar, hh[L], h, nullptr, nullptr, 0, 0, nullptr, wl.g(P.neg[L].w), h, wl.g(P.neg[L].b), nullptr, 0);   // dae.fc / main.fc
  if (P.cond)
    for (int l = 1; l <= L; ++l)   // ctx C_l: chat_l (x) c_{l-1}
      wl.push2(B, h, P.ctx[l - 1].in, W.chat[l], l == 1 ? ctx : W.cL[l - 1], l == 1 ? P.c : h, nullptr, nullptr, 0, 0, nullptr,
               wl.g(P.ctx[l - 1].w), P.ctx[l - 1].in, wl.g(P.ctx[l - 1].b), nullptr, 0);
  wl.assign(ws, P.cond ? 3 * L + 1 : L + 1);   // the split hint: the list's length (res kinds keep their grad sibling's, kind 13 kind 11's)
}

// dry run of cdae_carve() and the weight-gradient list on a null arena
size_t workspace_floats(const CdaeLayout& P, int B, int S, bool need_grads) {
  Bump ws;
  CdaeWs W;
  cdae_carve(P, ws, B, S, need_grads, W);
  if (need_grads) {
    WgradList wl(nullptr);
    cdae_wgrads(P, W, nullptr, nullptr, nullptr, B, S, wl, ws);
  }
  return ws.off;
}

int cdae_pack_impl(const CdaeLayout& P, const float* params, float* packed, hipStream_t st) {
  PackList pl(params, packed);
  const PackedLayout K(P, pl);
  if (P.has_sigma) ARDAE_TRY(launch_gather_strided(params + P.neg[0].w + P.sigma_col(), P.neg[0].in, P.h, packed + K.w1s, st));
  return pl.launch(st);
}

// the arguments of one fused Linear launch with a single source (lin1 of host_util.h, without the launch)
LinArgs lin_args(int act, int M, int Nout, const float* x, int ldx, int K, const float* wp, LinArgs a) {
  a.M = M; a.Nout = Nout; a.nsrc = 1; a.act = act;
  a.src[0].x = x; a.src[0].ld = ldx; a.src[0].K = K; a.src[0].wp = wp;
  return a;
}

// A run of consecutive N-row layers of one epilogue kind, each reading its predecessor's output: the longest prefixes that
// qualify go out as ONE launch each (linear_chain.hip: the small-shard regime), the rest layer by layer.
// one_by_one: no grouping, every layer is a launch of its own (the backward of kinds 1 / 11: moving it onto grouped launches is a change of its own, to be measured).
struct LayerRun {
  int epi;
  hipStream_t st;
  bool one_by_one;
  std::vector<LinArgs> v;
  LayerRun(int epi_, hipStream_t st_, bool one_by_one_ = false) : epi(epi_), st(st_), one_by_one(one_by_one_) {}
  void add(const LinArgs& a) { v.push_back(a); }
  int flush() {
    size_t i = 0;
    while (i < v.size()) {
      size_t n = one_by_one ? 1 : v.size() - i;
      while (n >= 2 && !linear_chain_eligible(v.data() + i, (int)n, epi)) --n;
      if (n >= 2) {
        ARDAE_TRY(launch_linear_chain(v.data() + i, (int)n, epi, st));
        i += n;
        continue;
      }
      // many tiles per workgroup: the same run layer-major in the weight-stationary kernel (one launch, the slab loaded once per layer)
      size_t m = one_by_one ? 1 : std::min<size_t>(v.size() - i, 6);
      while (m >= 2 && !linear_wide_layers_eligible(v.data() + i, (int)m, epi)) --m;
      if (m >= 2) {
        ARDAE_TRY(launch_linear_wide_layers(v.data() + i, (int)m, epi, st));
        i += m;
      } else {
        ARDAE_TRY(launch_linear(v[i], epi, st));
        i += 1;
      }
    }
    v.clear();
    return 0;
  }
};

// first_ready: a fused front end has written the first N-row layer's output where the carve puts it (a_1 with an input encoder, else h_1);
// for kinds 16 / 17 it has also run the context chain (cL, cb), which is then not run again
int cdae_impl(const ardae_cdae_desc* d, const float* params, const float* packed, const float* xbar, const float* sigma,
              const float* eps, const float* ctx, int B, int S, float* workspace, size_t ws_floats, float* loss, float* grads,
              float* score_out, bool need_grads, hipStream_t st, bool first_ready = false) {
  ARDAE_TRY(desc_ok(d));
  const CdaeLayout P(*d);
  const bool cond = P.cond, grad = P.grad;
  const bool enc = P.enc_inp;
  ARDAE_CHECK_ARG(cond || ctx == nullptr, "cdae: kinds 2 / 3 / 6 / 7 take no context: ctx must be NULL");
  const bool ctx_ready = first_ready && cond && !enc;
  // the plain DAEs' score does not read sigma (DAE.glogprob / ConditionalDAE.glogprob ignore std); their loss layer does
  ARDAE_CHECK_ARG(params && packed && xbar && (sigma || (!P.has_sigma && !need_grads)) && (ctx || !cond) && workspace, "cdae: null pointer argument");
  ARDAE_CHECK_ARG(B > 0 && S > 0 && (int64_t)B * S < (int64_t)1 << 30, "cdae: bad batch (B=%d, S=%d)", B, S);
  ARDAE_CHECK_ARG(!need_grads || (eps && loss && grads), "cdae: loss/grads/eps must be given");
  ARDAE_CHECK_ARG(need_grads || score_out, "cdae: score_out is NULL");
  const PackedLayout K(P);
  const int N = B * S, h = P.h, L = P.L, z = P.z, act = P.act, k1 = P.k1();
  // the whole arena up front: the buffers, then (need_grads) the weight-gradient list with its scratch
  Bump ws(workspace, ws_floats);
  CdaeWs W;
  cdae_carve(P, ws, B, S, need_grads, W);
  WgradList wl(grads);
  if (need_grads) cdae_wgrads(P, W, xbar, sigma, ctx, B, S, wl, ws);
  ARDAE_CHECK_ARG(ws.ok, "cdae: workspace too small (%zu < %zu floats)", ws_floats, ws.off);
  const std::vector<float*>&cL = W.cL, &a = W.a, &hh = W.hh, &e = W.e, &r = W.r, &tau = W.tau, &taup = W.taup, &pbar = W.pbar, &qbar = W.qbar, &chat = W.chat;
  float *cb = W.cb, *gbar = W.gbar, *Qsum = W.Qsum, *cs_taup = W.cs_taup;
  float* g = score_out ? score_out : W.gbuf;
  const float* x1 = enc ? a[L] : xbar;        // the energy MLP's input rows [N, k1]
  const float* wfc = params + P.neg[L].w;      // grad kinds: w [1,h]

  // ------------------------------------------------------------------ the layers of the forward and of the score pass
  auto ctx_layer = [&](int l) { LinArgs A{}; A.bias = params + P.ctx[l - 1].b; A.Y = cL[l]; A.ldY = h;
                                return lin_args(act, B, h, l == 1 ? ctx : cL[l - 1], l == 1 ? P.c : h, P.ctx[l - 1].in, packed + K.ctx_f[l - 1], A); };
  auto inp_layer = [&](int l) { LinArgs A{}; A.bias = params + P.inp[l - 1].b; A.Y = a[l]; A.ldY = h;
                                return lin_args(act, N, h, l == 1 ? xbar : a[l - 1], l == 1 ? z : h, P.inp[l - 1].in, packed + K.inp_f[l - 1], A); };
  auto ctx_bias = [&]() {  // per-image bias of the first energy layer: cb = W1c c_L + d_1
    LinArgs A{}; A.bias = params + P.neg[0].b; A.Y = cb; A.ldY = h;
    return lin_args(ACT_NONE, B, h, cL[L], h, h, packed + K.w1c_f, A);
  };
  auto energy_layer = [&](int l) {
    LinArgs A{}; A.Y = hh[l]; A.ldY = h;
    if (l == 1 && P.has_sigma) { A.rowscale = sigma; A.rowscale_w = packed + K.w1s; }
    if (l == 1 && cond) { A.rowbias = cb; A.rowbias_ld = h; A.rows_per_group = S; } else A.bias = params + P.neg[l - 1].b;
    if (grad && l == L) { A.Y2 = e[L]; A.ldY2 = h; A.R = wfc; }   // e_L = -w (.) s(h_L)
    return l == 1 ? lin_args(act, N, h, x1, k1, k1, packed + K.w1_f, A) : lin_args(act, N, h, hh[l - 1], h, h, packed + K.neg_f[l - 1], A);
  };
  auto e_layer = [&](int l) {   // e_{l-1} from e_l, l = L..2
    LinArgs A{}; A.S = hh[l - 1]; A.ldS = h; A.Y = e[l - 1]; A.ldY = h;
    return lin_args(act, N, h, e[l], h, h, packed + K.neg_b[l - 1], A);
  };
  auto r_layer = [&](int l) {   // r_{l-1} from r_l, l = L+1..2, with r_{L+1} W := e_1 W1a
    LinArgs A{}; A.S = a[l - 1]; A.ldS = h; A.Y = r[l - 1]; A.ldY = h;
    return l > L ? lin_args(act, N, h, e[1], h, h, packed + K.w1_b, A) : lin_args(act, N, h, r[l], h, h, packed + K.inp_b[l - 1], A);
  };
  auto g_layer = [&](LinArgs A) {   // the score g [N, z]: the last link of the score pass (r_1 A_1 | e_1 W1x), or fc(h_L) of the res kinds
    A.Y = g; A.ldY = z;
    if (grad) return lin_args(ACT_NONE, N, z, enc ? r[1] : e[1], h, h, packed + (enc ? K.inp_b[0] : K.w1_b), A);
    A.bias = params + P.neg[L].b;
    return lin_args(ACT_NONE, N, z, hh[L], h, h, packed + K.fc_f, A);
  };

  // ------------------------------------------------------------------ forward: ctx (B rows, once per image), inp and energy (N rows)
  if (!need_grads && enc && grad && N == B && linear_small_eligible(inp_layer(1), EPI_ACT)) {
    // The sigma = 0 score pass of the VAE update (glogprob on B rows, models/graddae/mlp.py:446-483): 4 L + 2 per-image problems, every one
    // a link of a dependent chain - ONE launch walks them level by level (linear_small_chain_kernel): [ctx_l | inp_l] l = 1..L, the
    // per-image bias of the first energy layer, the energy layers, the score layers, g.
    std::vector<LinArgs> pr; std::vector<int> ep, lv;
    int level = 0;
    auto add = [&](const LinArgs& A, int epi, int lev) { pr.push_back(A); ep.push_back(epi); lv.push_back(lev); };
    for (int l = 1; l <= L; ++l, ++level) { add(ctx_layer(l), EPI_ACT, level); add(inp_layer(l), EPI_ACT, level); }
    add(ctx_bias(), EPI_ACT, level++);
    for (int l = 1; l <= L; ++l) add(energy_layer(l), EPI_ACT, level++);
    for (int l = L; l >= 2; --l) add(e_layer(l), EPI_DACT, level++);
    for (int l = L + 1; l >= 2; --l) add(r_layer(l), EPI_DACT, level++);
    add(g_layer(LinArgs{}), EPI_ACT, level++);
    return launch_linear_small_chain(pr.data(), ep.data(), lv.data(), (int)pr.size(), W.chain_cnt, st);
  }
  {
    LayerRun run(EPI_ACT, st);      // the forward N-row layers: A_1 (2) .. A_L, then W_1 (2) .. W_L
    if (enc && !first_ready && linear_small_eligible(inp_layer(1), EPI_ACT)) {
      // few rows: the two encoders are independent chains of per-image launches - level l of both in ONE launch
      for (int l = 1; l <= L; ++l) ARDAE_TRY(launch_linear_pair(ctx_layer(l), inp_layer(l), EPI_ACT, st));
      ARDAE_TRY(launch_linear(ctx_bias(), EPI_ACT, st));
    } else if (cond) {
      // the whole per-image branch FIRST (context encoder, then the bias it contributes to the first energy layer): the N-row forward
      // layers of both networks then form ONE run (round 4: one multi-layer launch instead of two with a per-image launch between them)
      if (!ctx_ready) {
        for (int l = 1; l <= L; ++l) ARDAE_TRY(launch_linear(ctx_layer(l), EPI_ACT, st));
        ARDAE_TRY(launch_linear(ctx_bias(), EPI_ACT, st));
      }
      if (enc) for (int l = first_ready ? 2 : 1; l <= L; ++l) run.add(inp_layer(l));
    }
    for (int l = !enc && first_ready ? 2 : 1; l <= L; ++l) run.add(energy_layer(l));
    ARDAE_TRY(run.flush());
  }
  if (grad) {
    // ------------------------------------------------------------------ score pass (input-gradient of the energy)
    LayerRun run(EPI_DACT, st);
    for (int l = L; l >= 2; --l) run.add(e_layer(l));
    if (enc) for (int l = L + 1; l >= 2; --l) run.add(r_layer(l));
    ARDAE_TRY(run.flush());
  }
  if (!need_grads) return launch_linear(g_layer(LinArgs{}), EPI_ACT, st);   // glogprob
  const float inv_nz = 1.0f / ((float)N * (float)z);
  {
    LinArgs A{}; A.sigma = sigma; A.eps = eps; A.ldeps = z; A.scale = inv_nz; A.Y2 = gbar; A.ldY2 = z; A.tile_loss = W.tile_loss;
    ARDAE_TRY(launch_linear(g_layer(A), EPI_DAE_LOSS, st));
  }
  ARDAE_TRY(launch_sum_scale(W.tile_loss, W.ltiles, inv_nz, loss, st));

  // -------------------------------------------------------------------- backward
  const std::vector<float*>&qhat = qbar, &phat = pbar;   // in-place: qhat_l overwrites qbar_l, phat_l overwrites pbar_l
  if (grad) {
    // forward-mode chain through the score pass
    LayerRun run(EPI_CHAIN, st);
    if (enc)
      for (int l = 1; l <= L; ++l) {
        LinArgs A{}; A.S = a[l]; A.ldS = h; A.R = r[l]; A.ldR = h; A.Y = tau[l]; A.ldY = h; A.Y2 = pbar[l]; A.ldY2 = h;
        run.add(l == 1 ? lin_args(act, N, h, gbar, z, z, packed + K.inp_f[0], A) : lin_args(act, N, h, tau[l - 1], h, h, packed + K.inp_f[l - 1], A));
      }
    for (int l = 1; l <= L; ++l) {
      LinArgs A{}; A.S = hh[l]; A.ldS = h; A.R = e[l]; A.ldR = h; A.Y = taup[l]; A.ldY = h; A.Y2 = qbar[l]; A.ldY2 = h;
      if (l == L) A.colsum = cs_taup;
      run.add(l == 1 ? lin_args(act, N, h, enc ? tau[L] : gbar, k1, k1, packed + K.w1_f, A) : lin_args(act, N, h, taup[l - 1], h, h, packed + K.neg_f[l - 1], A));
    }
    ARDAE_TRY(run.flush());
    // wbar = -colsum(tau'_L)  -> grads of neglogprob.fc.weight [1,h]
    ARDAE_TRY(launch_segment_sum(cs_taup, h, 1, W.ctiles, h, -1.0f, grads + P.neg[L].w, h, st));
  } else {
    // direct-score variant: the backward starts from gbar
    LinArgs A{}; A.S = hh[L]; A.ldS = h; A.Y = qhat[L]; A.ldY = h;
    ARDAE_TRY(lin1(EPI_DACT, act, N, h, gbar, z, z, packed + K.fc_b, A, st));
  }
  {
    // ordinary backward of the energy chain and (cond) the input encoder; the grad kinds seed every layer with its qbar_l / pbar_l
    LayerRun run(EPI_DACT, st, cond && !grad);
    for (int l = L; l >= 2; --l) {
      LinArgs A{}; A.S = hh[l - 1]; A.ldS = h; A.Y = qhat[l - 1]; A.ldY = h;
      if (grad) { A.Q = qbar[l - 1]; A.ldQ = h; }
      run.add(lin_args(act, N, h, qhat[l], h, h, packed + K.neg_b[l - 1], A));
    }
    if (enc)
      for (int l = L + 1; l >= 2; --l) {   // phat_{l-1} from phat_l, with phat_{L+1} A := qhat_1 W1a
        LinArgs A{}; A.S = a[l - 1]; A.ldS = h; A.Y = phat[l - 1]; A.ldY = h;
        if (grad) { A.Q = pbar[l - 1]; A.ldQ = h; }
        run.add(l > L ? lin_args(act, N, h, qhat[1], h, h, packed + K.w1_b, A) : lin_args(act, N, h, phat[l], h, h, packed + K.inp_b[l - 1], A));
      }
    ARDAE_TRY(run.flush());
  }
  if (cond) {
    // ctx branch: reduce over the S samples of each image first, then B-row back-prop
    ARDAE_TRY(launch_segment_sum(qhat[1], h, B, S, h, 1.0f, Qsum, h, st));
    for (int l = L + 1; l >= 2; --l) {     // chat_{l-1} from chat_l, with chat_{L+1} C := Qsum W1c
      LinArgs A{}; A.S = cL[l - 1]; A.ldS = h; A.Y = chat[l - 1]; A.ldY = h;
      ARDAE_TRY(lin1(EPI_DACT, act, B, h, l > L ? Qsum : chat[l], h, h, packed + (l > L ? K.w1c_b : K.ctx_b[l - 1]), A, st));
    }
  }

  // -------------------------------------------------------------------- weight gradients: one batched launch (cdae_wgrads)
  return wl.launch(st);
}

}  // namespace

// what the fused front end of dae_perturb.hip needs of an unconditional network: where W1 / d_1 live, and the carved h_1 it writes
int dae_front_slots(const ardae_cdae_desc* d, int N, float* workspace, size_t ws_floats, size_t* w1, size_t* b1, float** h1) {
  ARDAE_TRY(desc_ok(d));
  const CdaeLayout P(*d);
  ARDAE_CHECK_ARG(!P.cond, "dae_perturb_loss_grads: the network must be unconditional");
  const size_t need = workspace_floats(P, N, 1, true);
  ARDAE_CHECK_ARG(ws_floats >= need, "dae_perturb_loss_grads: workspace too small (%zu < %zu floats)", ws_floats, need);
  Bump ws(workspace, ws_floats);
  CdaeWs W;
  cdae_carve(P, ws, N, 1, true, W);
  *w1 = P.neg[0].w; *b1 = P.neg[0].b; *h1 = W.hh[1];
  return 0;
}
int dae_loss_grads_from_h1(const ardae_cdae_desc* d, const float* params, const float* packed, const float* xbar, const float* sigma, const float* eps,
                           int N, float* workspace, size_t ws_floats, float* loss, float* grads, hipStream_t st) {
  return cdae_impl(d, params, packed, xbar, sigma, eps, nullptr, N, 1, workspace, ws_floats, loss, grads, nullptr, true, st, true);
}

}  // namespace ardae

using namespace ardae;

extern "C" {

size_t ardae_cdae_param_floats(const ardae_cdae_desc* d) {
  if (desc_ok(d) != 0) return 0;
  return CdaeLayout(*d).total;
}
size_t ardae_cdae_packed_floats(const ardae_cdae_desc* d) {
  if (desc_ok(d) != 0) return 0;
  PackList pl;
  PackedLayout(CdaeLayout(*d), pl);
  return pl.total();
}
size_t ardae_cdae_workspace_floats(const ardae_cdae_desc* d, int B, int S, int need_grads) {
  if (desc_ok(d) != 0 || B <= 0 || S <= 0) return 0;
  return workspace_floats(CdaeLayout(*d), B, S, need_grads != 0);
}
int ardae_cdae_pack(const ardae_cdae_desc* d, const float* params, float* packed, void* stream) {
  ARDAE_TRY(desc_ok(d));
  ARDAE_CHECK_ARG(params && packed, "cdae_pack: null pointer");
  return cdae_pack_impl(CdaeLayout(*d), params, packed, (hipStream_t)stream);
}
int ardae_cdae_loss_grads(const ardae_cdae_desc* d, const float* params, const float* packed, const float* xbar,
                          const float* sigma, const float* eps, const float* ctx, int B, int S, float* workspace,
                          size_t workspace_floats, float* loss, float* grads, float* score_out, void* stream) {
  return cdae_impl(d, params, packed, xbar, sigma, eps, ctx, B, S, workspace, workspace_floats, loss, grads, score_out, true,
                   (hipStream_t)stream);
}
int ardae_cdae_perturb_fused_ok(const ardae_cdae_desc* d, int nz, int nstd) {
  if (desc_ok(d) != 0) return 0;
  const CdaeLayout P(*d);   // the fused draw + first-layer kernel is the conditional AR-DAE kinds' (it draws sigma): A_1, or W1x of kinds 16 / 17
  return P.cond && P.has_sigma && nstd == 1 && latent_perturb_draw_fwd_ok(nz, P.z, P.h, P.act) ? 1 : 0;
}
int ardae_cdae_perturb_loss_grads(const ardae_cdae_desc* d, const float* params, const float* packed, const float* latent, const float* z0,
                                  const float* ctx, int B, int nz, float std_scale, float delta, uint64_t seed, uint64_t offset_xi,
                                  uint64_t offset_eps, const void* state, uint64_t first_row, float* xbar, float* sigma, float* eps_out,
                                  float* std_b, float* workspace, size_t ws_floats, float* loss, float* grads, void* stream) {
  ARDAE_TRY(desc_ok(d));
  ARDAE_CHECK_ARG(ardae_cdae_perturb_fused_ok(d, nz, 1), "cdae_perturb_loss_grads: shape not eligible (nz=%d): use ardae_latent_perturb* + ardae_cdae_loss_grads", nz);
  ARDAE_CHECK_ARG(params && packed && workspace && B > 0, "cdae_perturb_loss_grads: null pointer argument");
  const CdaeLayout P(*d);
  const PackedLayout K(P);
  ARDAE_CHECK_ARG(ws_floats >= workspace_floats(P, B, nz, true), "cdae_perturb_loss_grads: workspace too small");
  Bump ws(workspace, ws_floats);
  CdaeWs W;
  cdae_carve(P, ws, B, nz, true, W);   // the kernel below leaves a_1 (kinds 16 / 17: h_1) where cdae_impl reads it
  const hipStream_t st = (hipStream_t)stream;
  if (!P.enc_inp) {
    // the per-image branch first, with cdae_impl's own launches: ctx_encode, then cb = W1c c_L + d_1 - the kernel adds it (and sigma w1s) to W1x xbar
    ARDAE_CHECK_ARG(latent && z0 && ctx && xbar && sigma && eps_out && std_b && loss && grads, "cdae_perturb_loss_grads: null pointer argument");
    const int h = P.h, L = P.L;
    for (int l = 1; l <= L; ++l) {
      LinArgs A{}; A.bias = params + P.ctx[l - 1].b; A.Y = W.cL[l]; A.ldY = h;
      ARDAE_TRY(launch_linear(lin_args(P.act, B, h, l == 1 ? ctx : W.cL[l - 1], l == 1 ? P.c : h, P.ctx[l - 1].in, packed + K.ctx_f[l - 1], A), EPI_ACT, st));
    }
    LinArgs A{}; A.bias = params + P.neg[0].b; A.Y = W.cb; A.ldY = h;
    ARDAE_TRY(launch_linear(lin_args(ACT_NONE, B, h, W.cL[L], h, h, packed + K.w1c_f, A), EPI_ACT, st));
    const bool seed_e = P.grad && L == 1;   // the only hidden layer: the score pass's seed e_1 comes with it
    ARDAE_TRY(launch_latent_perturb_draw_fwd(latent, z0, B, nz, P.z, std_scale, delta, seed, offset_xi, offset_eps, state, first_row, xbar, sigma, eps_out,
                                             std_b, packed + K.w1_f, W.cb, h, P.act, W.hh[1], st, packed + K.w1s, seed_e ? params + P.neg[L].w : nullptr,
                                             seed_e ? W.e[1] : nullptr));
    return cdae_impl(d, params, packed, xbar, sigma, eps_out, ctx, B, nz, workspace, ws_floats, loss, grads, nullptr, true, st, true);
  }
  ARDAE_TRY(launch_latent_perturb_draw_fwd(latent, z0, B, nz, P.z, std_scale, delta, seed, offset_xi, offset_eps, state, first_row, xbar, sigma,
                                           eps_out, std_b, packed + K.inp_f[0], params + P.inp[0].b, P.h, P.act, W.a[1],
                                           (hipStream_t)stream));
  return cdae_impl(d, params, packed, xbar, sigma, eps_out, ctx, B, nz, workspace, ws_floats, loss, grads, nullptr, true, (hipStream_t)stream,
                   true);
}
int ardae_cdae_score(const ardae_cdae_desc* d, const float* params, const float* packed, const float* x, const float* sigma,
                     const float* ctx, int B, int S, float* workspace, size_t workspace_floats, float* score_out, void* stream) {
  return cdae_impl(d, params, packed, x, sigma, nullptr, ctx, B, S, workspace, workspace_floats, nullptr, nullptr, score_out, false,
                   (hipStream_t)stream);
}

}  // extern "C"
