// Host-side helpers shared by the model families (model / convmodel / auxmodel / resmodel .hip) and cdae.hip: the bump
// allocator that carves a workspace arena, one-/two-source linear launches and the dense-layer calls written with them, the
// list of weight-gradient problems a backward pass hands to launch_wgrad_batch, the Linear on a concat whose first half is
// per image (forward, backward-data, weight-gradient problems), the list of weight panels a network's packed
// buffer is made of, and what every model family is made of (the Family table row, its sizing / pack triple, the prologue of
// an entry point).
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"
#include "elementwise.h"
#include "linear.h"
#include "wgrad.h"

namespace ardae {

inline size_t al64(size_t n) { return (n + 63) & ~size_t(63); }
inline unsigned nblk(int64_t n) { return (unsigned)((n + 255) / 256); }

// Carves 64-float-aligned pieces out of an arena.  With a null base it only counts (the sizing pass of every
// *_workspace_floats): take() returns nullptr and `off` ends up as the floats a real arena needs.
struct Bump {
  float* base; size_t cap; size_t off = 0; bool ok = true;
  Bump(float* b, size_t c) : base(b), cap(c) {}
  Bump() : base(nullptr), cap(~size_t(0) >> 2) {}   // sizing pass
  float* take(size_t n) {
    size_t o = off; off += al64(n);
    if (off > cap) { ok = false; return base; }
    return base ? base + o : nullptr;
  }
};

// one linear launch, one or two sources
inline int lin1(int epi, int act, int M, int Nout, const float* x, int ldx, int K, const float* wp, LinArgs a, hipStream_t st) {
  a.M = M; a.Nout = Nout; a.nsrc = 1; a.act = act;
  a.src[0].x = x; a.src[0].ld = ldx; a.src[0].K = K; a.src[0].wp = wp;
  return launch_linear(a, epi, st);
}
inline int lin2(int epi, int act, int M, int Nout, const float* x0, int ld0, int K0, const float* wp0, const float* x1, int ld1, int K1, const float* wp1,
                LinArgs a, hipStream_t st) {
  a.M = M; a.Nout = Nout; a.nsrc = 2; a.act = act;
  a.src[0].x = x0; a.src[0].ld = ld0; a.src[0].K = K0; a.src[0].wp = wp0;
  a.src[1].x = x1; a.src[1].ld = ld1; a.src[1].K = K1; a.src[1].wp = wp1;
  return launch_linear(a, epi, st);
}

// The dense layers of the model families (wp: the packed panel of the operator; every buffer is dense, ld = its column count):
//   y [M, n] = act(x [M, K] W^T + bias)   (bias null: none - with ACT_NONE also the backward-data product g W of a layer
//   whose input has no activation in front)
inline int dense_fwd(int act, int M, int n, const float* x, int ldx, int K, const float* wp, const float* bias, float* y, hipStream_t st) {
  LinArgs A{}; A.bias = bias; A.Y = y; A.ldY = n;
  return lin1(EPI_ACT, act, M, n, x, ldx, K, wp, A, st);
}
//   y [M, n] = (g [M, K] W) (.) act'(S) (+ Q)   (S: the saved post-activation [M, n]; with ACT_NONE act' == 1 and S is only a placeholder)
inline int dense_bwd(int act, int M, int n, const float* g, int K, const float* wp, const float* S, float* y, hipStream_t st, const float* Q = nullptr) {
  LinArgs A{}; A.S = S; A.ldS = n; A.Q = Q; A.ldQ = Q ? n : 0; A.Y = y; A.ldY = n;
  return lin1(EPI_DACT, act, M, n, g, K, K, wp, A, st);
}
//   y [M, n] = (g0 [M, K] W0 + g1 [M, K] W1) (.) act'(S): two heads back into the layer both read
inline int dense_bwd2(int act, int M, int n, const float* g0, const float* wp0, const float* g1, const float* wp1, int K, const float* S, float* y,
                      hipStream_t st) {
  LinArgs A{}; A.S = S; A.ldS = n; A.Y = y; A.ldY = n;
  return lin2(EPI_DACT, act, M, n, g0, K, K, wp0, g1, K, K, wp1, A, st);
}

// A Linear in the flat parameter buffer: weight [out, in] at w, bias at b (offsets in floats)
struct Lin { size_t w, b; int out, in; };
// the next Linear at parameter offset `off` (advanced past the weight and nbias bias entries; default: one per output)
inline Lin next_lin(size_t& off, int out, int in, int nbias = -1) {
  Lin l; l.out = out; l.in = in; l.w = off; off += (size_t)out * in; l.b = off; off += nbias < 0 ? out : nbias;
  return l;
}

// The panels of a packed-weight buffer, written ONCE per network: the constructor of a family's *Packed struct reserves
// every panel through this list and keeps the returned offsets.  Over the real (params, packed) pointers each reservation
// also records the pack_batch item that fills it, and launch() packs them all; over null pointers (the sizing pass of
// *_packed_floats and of every entry point that only needs the offsets) it only counts, and total() is the buffer's size.
struct PackList {
  std::vector<PackItem> items;
  const float* params; float* packed;
  size_t off = 0;
  PackList() : params(nullptr), packed(nullptr) {}   // sizing pass
  PackList(const float* params_, float* packed_) : params(params_), packed(packed_) {}
  // a raw reservation (filled by something other than the pack launch)
  size_t take(size_t n) { size_t o = off; off += al64(n); return o; }
  // the panel of W[nout, k] (transpose: of W[k, nout]^T) with leading dimension ldw; W starts src floats into params, or
  // (src_in_packed: a weight composed there by an earlier launch on the same stream) into the packed buffer itself
  size_t panel(size_t src, int ldw, int nout, int k, bool transpose, bool src_in_packed = false) {
    const size_t o = take(packed_floats(nout, k));
    if (packed) {
      if (items.empty()) items.reserve(PACK_BATCH_MAX);   // one allocation for all but the residual-conv lists
      items.push_back(PackItem{(src_in_packed ? packed : params) + src, ldw, nout, k, transpose ? 1 : 0, packed + o});
    }
    return o;
  }
  // the common pair: the forward panel of l's columns [col0, col0 + k) (default: all of them), then its transpose
  void pair(const Lin& l, size_t& f, size_t& b, int col0 = 0, int k = 0) {
    if (k == 0) k = l.in;
    f = panel(l.w + col0, l.in, l.out, k, false);
    b = panel(l.w + col0, l.in, k, l.out, true);
  }
  size_t total() const { return off; }
  int launch(hipStream_t st) { return launch_pack_batch(items.data(), (int)items.size(), st); }
};

// The weight-gradient problems of one backward, written ONCE per family: the backward pushes them with its real buffers,
// assigns their scratch out of the arena and launches; *_workspace_floats runs the same code over a sizing Bump with null
// buffers (nothing is dereferenced) and reads the arena offset.
struct WgradList {
  std::vector<WgradProblem> probs;
  float* grads;      // flat gradient buffer (null in a sizing pass)
  float beta;        // out = beta * out + sum, for every problem pushed
  size_t next = 0;   // first problem not launched yet
  explicit WgradList(float* grads_, float beta_ = 0.f) : grads(grads_), beta(beta_) {}
  float* g(size_t off) const { return grads ? grads + off : nullptr; }

  // dW[O, I] = G[M, O]^T X[M, I] (+ the bias gradient, G's column sums, where out_bias is given)
  WgradProblem& push(int M, int O, int I, const float* G, const float* X, int ldX, float* out, int ldout, float* out_bias) {
    WgradProblem p;
    memset(&p, 0, sizeof(p));
    p.M = M; p.O = O; p.I = I; p.npairs = 1;
    p.G[0] = G; p.ldG[0] = O; p.X[0] = X; p.ldX[0] = ldX;
    p.bias_pair = out_bias ? 0 : -1;
    p.out = out; p.ldout = ldout; p.out_bias = out_bias; p.beta = beta;
    return add(p);
  }
  // the cDAE's form: a second (G, X) pair (G1 null: none), the pair whose G gives the bias gradient (-1: none), a row scale
  WgradProblem& push2(int M, int O, int I, const float* G0, const float* X0, int ldX0, const float* G1, const float* X1, int ldX1, int bias_pair,
                      const float* rowscale, float* out, int ldout, float* out_bias, float* out_rs, int ld_rs) {
    WgradProblem p;
    memset(&p, 0, sizeof(p));
    p.M = M; p.O = O; p.I = I;
    p.npairs = G1 ? 2 : 1;
    p.G[0] = G0; p.ldG[0] = O; p.X[0] = X0; p.ldX[0] = ldX0;
    p.G[1] = G1; p.ldG[1] = O; p.X[1] = X1; p.ldX[1] = ldX1;
    p.bias_pair = bias_pair; p.rowscale = rowscale;
    p.out = out; p.ldout = ldout; p.out_bias = out_bias; p.out_rowscale = out_rs; p.ld_rowscale = ld_rs; p.beta = beta;
    return add(p);
  }
  WgradProblem& add(const WgradProblem& p) {
    if (probs.empty()) probs.reserve(WGRAD_MAX_PROBLEMS + 2);   // one allocation per list
    probs.push_back(p);
    return probs.back();
  }
  size_t pending() const { return probs.size() - next; }
  // splits (wgrad_splits with the family's hint) and scratch for the next n pending problems, in list order
  void assign(Bump& ws, int hint, size_t n = ~size_t(0)) {
    const size_t end = next + std::min(n, pending());
    for (size_t i = next; i < end; ++i) {
      WgradProblem& p = probs[i];
      p.splits = wgrad_splits(p.M, p.O, p.I, hint);
      p.partial = ws.take((size_t)p.splits * p.O * p.I);
      p.partial_vec = ws.take((size_t)p.splits * 2 * p.O);
    }
  }
  // launches the next n pending problems (default: all of them), WGRAD_MAX_PROBLEMS per batch at most; a caller that wants
  // a batch boundary elsewhere names it through n
  int launch(hipStream_t st, size_t n = ~size_t(0)) {
    const size_t end = next + std::min(n, pending());
    while (next < end) {
      const size_t m = std::min<size_t>(end - next, WGRAD_MAX_PROBLEMS);
      ARDAE_TRY(launch_wgrad_batch(probs.data() + next, (int)m, st));
      next += m;
    }
    return 0;
  }
};

// Linear on cat[ctx | s] -> [B rpg, n]: ctx [B, cw], the first cw columns of the weight, is per image - its product (+ the bias) is made once as the row
// bias rb [B, n], which the s half's launch on the rows s [B rpg, sd] adds to each group of rpg rows.  wp_*: the forward panels of the two halves.
inline int cat_fwd(int act, int B, int rpg, int n, const float* ctx, int cw, const float* wp_ctx, const float* bias, const float* s, int sd, const float* wp_s,
                   float* rb, float* y, hipStream_t st) {
  ARDAE_TRY(dense_fwd(ACT_NONE, B, n, ctx, cw, cw, wp_ctx, bias, rb, st));
  LinArgs A{}; A.Y = y; A.ldY = n; A.rowbias = rb; A.rowbias_ld = n; A.rows_per_group = rpg;
  return lin1(EPI_ACT, act, B * rpg, n, s, sd, sd, wp_s, A, st);
}
// its backward-data from dpre [M, n] = d(pre-activation), one row per image: ds [M, sd] = dpre Ws (+ qs), then dctx [M, cw] = dpre Wc (+ qc) unless dctx
// is null (a ctx that takes no gradient).  q: what else arrives there; the output must not be its q.  wb_*: the backward panels.
inline int cat_bwd(int M, int n, const float* dpre, int sd, const float* wb_s, const float* qs, float* ds, int cw, const float* wb_ctx, const float* qc,
                   float* dctx, hipStream_t st) {
  auto half = [&](int k, const float* wb, const float* q, float* y) {
    if (q) return dense_bwd(ACT_NONE, M, k, dpre, n, wb, q, y, st, q);      // act' == 1: S is only a placeholder
    return dense_fwd(ACT_NONE, M, k, dpre, n, n, wb, nullptr, y, st);
  };
  ARDAE_TRY(half(sd, wb_s, qs, ds));
  return dctx ? half(cw, wb_ctx, qc, dctx) : 0;
}
// its two weight-gradient problems on M rows (one per image): the s half (+ bias), then the ctx half
inline void cat_wgrads(WgradList& wl, int M, const Lin& l, int cw, const float* dpre, const float* s, const float* ctx) {
  const int sd = l.in - cw;
  wl.push(M, l.out, sd, dpre, s, sd, wl.g(l.w + cw), l.in, wl.g(l.b));
  wl.push(M, l.out, cw, dpre, ctx, cw, wl.g(l.w), l.in, nullptr);
}

// the caller's noise, or (null: a std = 0 pass, the reference multiplies its draw by 0) the n floats at `zero`, filled with zeros
inline int noise_or_zero(const float*& noise, float* zero, size_t n, hipStream_t st) {
  if (noise) return 0;
  noise = zero;
  return launch_fill(zero, (int64_t)n, 0.f, st);
}

// ------------------------------------------------------------------------------------------------ the model families
// One row of csrc/model.hip's table by kind (encode: hidden_out / raw0 and decode: out1 are NULL for the families that have no
// such output / input).  Each family file defines its own.  The row carries everything the entry points decide by: they know no kind number.
struct GaussFamily;   // csrc/vaemodel.h
// what a descriptor of the family can do (a row may serve two kinds, so these are read per descriptor)
enum { CAP_GAUSS_DECODER = 1,   // the decoder has mean and logvar heads: ardae_model_decode needs out1, ardae_model_loss_rows the Gaussian likelihood
       CAP_HIDDEN = 2,          // ardae_model_encode_hidden: the hidden1a context
       CAP_HIDDEN_RAW = 4 };    // ardae_model_encode_hidden_raw: the same with an unscaled eps0
struct Family {
  int (*desc_check)(const ardae_model_desc* d);    // the family's descriptor rules, next to its layout: 0, or -1 with the message set
  unsigned (*caps)(const ardae_model_desc& d);     // CAP_*
  size_t (*param_floats)(const ardae_model_desc&);
  size_t (*packed_floats)(const ardae_model_desc&);
  size_t (*workspace_floats)(const ardae_model_desc&, int B, int nz, int mode);   // mode 2: decode only, 3: encode_pair
  int (*pack)(const ardae_model_desc&, const float* params, float* packed, hipStream_t);
  int (*encode)(const ardae_model_desc&, const float* params, const float* packed, const float* x, const float* noise, int B, int nz,
                float* workspace, size_t wsf, float* z_out, float* hidden_out, hipStream_t, const float* raw0);
  int (*decode)(const ardae_model_desc&, const float* params, const float* packed, const float* z, int R, float* workspace, size_t wsf,
                float* out0, hipStream_t, float* out1);
  int (*vae_forward)(const ardae_model_desc&, const float* params, const float* packed, const float* x, const float* noise, int B, int nz,
                     DevFloat beta, float* workspace, size_t wsf, float* z_out, float* losses, hipStream_t);
  int (*vae_backward)(const ardae_model_desc&, const float* params, const float* packed, const float* x, const float* noise, int B, int nz,
                      DevFloat beta, float dloss, const float* dz_extra, float* workspace, size_t wsf, float* grads, float grads_beta, hipStream_t);
  const GaussFamily* gauss;   // the Gaussian-posterior kinds' ardae_vae_* bodies; null for the implicit kinds
  // the fused ardae_model_encode_pair (phase as in the ABI); null: the entry point runs two passes of `encode` over the same workspace
  int (*encode_pair)(const ardae_model_desc&, const float* params, const float* packed, const float* x, const float* noise, int B, int nz,
                     float* workspace, size_t wsf, float* z0_out, float* z_out, int phase, hipStream_t);
  // the two halves of vae_backward as calls of their own (decoder: loss gradients + decoder backward up to dz; sampler: dz += seed_scale
  // dz_extra, then the sampler's backward and the weight gradients); null: the family has no split backward
  int (*vae_backward_decoder)(const ardae_model_desc&, const float* params, const float* packed, const float* x, const float* noise, int B, int nz,
                              DevFloat beta, float dloss, float* workspace, size_t wsf, hipStream_t);
  int (*vae_backward_sampler)(const ardae_model_desc&, const float* params, const float* packed, const float* x, const float* noise, int B, int nz,
                              const float* dz_extra, DevFloat seed_scale, float* workspace, size_t wsf, float* grads, float grads_beta, hipStream_t);
};
inline unsigned no_caps(const ardae_model_desc&) { return 0; }
// the flag rule of an implicit family's desc_check: nothing outside `allowed`, and known log-variance clip codes
inline int desc_flags_ok(const ardae_model_desc* d, int allowed) {
  ARDAE_CHECK_ARG((d->flags & ~allowed) == 0,
                  "model: unknown flags %d (ARDAE_MODEL_NO_CENTER / the sampler-head bits / ARDAE_MODEL_CLIPPED: residual-conv kinds 5 / 6 only; "
                  "the log-variance clip codes: kinds 3 / 7 only)", d->flags);
  ARDAE_CHECK_ARG(((d->flags >> ARDAE_MODEL_CLIP_Z0_SHIFT) & 15) <= 10 && ((d->flags >> ARDAE_MODEL_CLIP_Z_SHIFT) & 15) <= 10, "model: unknown log-variance clip code");
  return 0;
}
// the table (csrc/model.hip): the row of a kind, null where the number is not a kind; family(d) where the kind has been checked
const Family* family_of(int kind);
inline const Family& family(const ardae_model_desc* d) { return *family_of(d->kind); }

// A family is a Layout (the Linears' offsets in the flat parameter buffer, from the desc) and a Packed (the panels' offsets in the
// packed buffer, reserved on a PackList).  Where the pack launch is all a family's pack does, these three are its first members:
template <class Layout, class Packed> size_t family_param_floats(const ardae_model_desc& d) { return Layout(d).total; }
template <class Layout, class Packed> size_t family_packed_floats(const ardae_model_desc& d) {
  const Layout P(d);
  PackList pl;
  const Packed K(P, pl);
  return pl.total();
}
template <class Layout, class Packed> int family_pack(const ardae_model_desc& d, const float* params, float* packed, hipStream_t st) {
  const Layout P(d);
  PackList pl(params, packed);
  const Packed K(P, pl);
  return pl.launch(st);
}

// What every entry point opens with: the layout, the panel offsets, the arena, and the buffers the family's carve(P, ws, ..., W)
// takes out of it.  `auto& [P, K, ws, W] = entry;` names them.
template <class Layout, class Packed, class Ws> struct Entry {
  const Layout P; const Packed K; Bump ws; Ws W{};
  template <class... CarveArgs> Entry(const ardae_model_desc& d, float* workspace, size_t wsf, CarveArgs... args) : P(d), K(P), ws(workspace, wsf) {
    carve(P, K, ws, args..., W);
  }
};

// y = x * act'(S)  (S = saved post-activation); y may alias x
int launch_mul_dact(const float* x, const float* S, int act, float* y, int64_t n, hipStream_t st);
// [B, HW, C] (NHWC rows) <-> [B, C*HW] (PyTorch's .view(B, -1) of NCHW); to_nhwc: `in` is the NCHW side
int launch_nhwc_nchw(const float* in, int B, int HW, int C, float* out, bool to_nhwc, hipStream_t st);

}  // namespace ardae
