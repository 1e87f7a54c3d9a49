// The two pieces the MLP model families (csrc/model.hip: kinds 0 / 1, csrc/auxmodel.hip: kinds 3 / 7) are built of: a plain
// stack of Linear -> act layers, and the decoder - such a stack from z with one (logits) or two (mean, logvar) linear heads.
#pragma once
#include <vector>

#include "host_util.h"

namespace ardae {

// n Linear -> act layers; layer l (1-based) reads a[l - 1] (a[0]: the stack's input x, passed on its own) and writes a[l]
struct MlpStack {
  std::vector<Lin> lin;
  std::vector<size_t> f, b;   // forward / backward panels
  MlpStack() {}
  // the layers (parameter order) and their panels, reserved pair by pair in that order
  MlpStack(const Lin* l, size_t n, PackList& pl) : lin(l, l + n), f(n), b(n) {
    for (size_t i = 0; i < n; ++i) pl.pair(lin[i], f[i], b[i]);
  }
  size_t n() const { return lin.size(); }

  // a[l] = act(a[l - 1] W_l^T + b_l), l = first .. n, on M rows  (first > 1: a[first - 1] is already there)
  int fwd(const float* params, const float* packed, int act, int M, const float* x, float* const* a, hipStream_t st, size_t first = 1) const {
    for (size_t l = first; l <= n(); ++l) {
      const Lin& L = lin[l - 1];
      ARDAE_TRY(dense_fwd(act, M, L.out, l == 1 ? x : a[l - 1], L.in, L.in, packed + f[l - 1], params + L.b, a[l], st));
    }
    return 0;
  }
  // d[l - 1] = (d[l] W_l) (.) act'(a[l - 1]), l = n .. 2   (what lies below d[1] is the caller's: the stack's input is not its own)
  int bwd(const float* packed, int act, int M, float* const* a, float* const* d, hipStream_t st) const {
    for (size_t l = n(); l >= 2; --l) ARDAE_TRY(dense_bwd(act, M, lin[l - 1].in, d[l], lin[l - 1].out, packed + b[l - 1], a[l - 1], d[l - 1], st));
    return 0;
  }
  // dW_l = d[l]^T a[l - 1] (+ bias), l = 1 .. n
  void wgrads(WgradList& wl, int M, const float* x, float* const* a, float* const* d) const {
    for (size_t l = 1; l <= n(); ++l) {
      const Lin& L = lin[l - 1];
      wl.push(M, L.out, L.in, d[l], l == 1 ? x : a[l - 1], L.in, wl.g(L.w), L.in, wl.g(L.b));
    }
  }
  // a[1 .. n] (a[0] stays null), M rows each
  void carve(Bump& ws, size_t M, std::vector<float*>& a) const {
    a.assign(n() + 1, nullptr);
    for (size_t l = 1; l <= n(); ++l) a[l] = ws.take(M * lin[l - 1].out);
  }
};

// z [R, zd] -> stack -> head(s) [R, D]
struct MlpDecoder {
  MlpStack stack;
  Lin head[2];
  size_t head_f[2], head_b[2];
  int nh = 0;
  MlpDecoder() {}
  // panels: the stack's, then the heads'
  MlpDecoder(const Lin* layers, size_t n, const Lin* heads, int nheads, PackList& pl) : stack(layers, n, pl), nh(nheads) {
    for (int k = 0; k < nh; ++k) { head[k] = heads[k]; pl.pair(head[k], head_f[k], head_b[k]); }
  }
  int zd() const { return stack.lin[0].in; }
  int D() const { return head[0].out; }

  struct Bufs {
    std::vector<float*> hid, dhid;   // [1 .. n]: the hidden layers and their gradients, [R, h]
    float* o[2] = {nullptr, nullptr};     // head outputs [R, D]
    float* dox[2] = {nullptr, nullptr};   // ... and the loss gradients w.r.t. them
    float *dzq = nullptr, *dz = nullptr;  // [R, zd]: the part of dL/dz that does not pass through the decoder (prior + injected seed); dL/dz
  };
  // decode only: the hidden layers; train: everything
  void carve(Bump& ws, size_t R, bool train, Bufs& u) const {
    stack.carve(ws, R, u.hid);
    if (!train) return;
    for (int k = 0; k < nh; ++k) { u.o[k] = ws.take(R * D()); u.dox[k] = ws.take(R * D()); }
    stack.carve(ws, R, u.dhid);
    u.dzq = ws.take(R * zd()); u.dz = ws.take(R * zd());
  }

  int fwd(const float* params, const float* packed, int act, int R, const float* z, float* const* hid, float* const* out, hipStream_t st) const {
    ARDAE_TRY(stack.fwd(params, packed, act, R, z, hid, st));
    for (int k = 0; k < nh; ++k)
      ARDAE_TRY(dense_fwd(ACT_NONE, R, head[k].out, hid[stack.n()], head[k].in, head[k].in, packed + head_f[k], params + head[k].b, out[k], st));
    return 0;
  }
  // from the loss gradients u.dox (and u.dzq) down to u.dz = dhid_1 W_1 + dzq
  int bwd(const float* packed, int act, int R, const Bufs& u, hipStream_t st) const {
    const size_t n = stack.n();
    const int h = head[0].in;
    if (nh == 2) ARDAE_TRY(dense_bwd2(act, R, h, u.dox[0], packed + head_b[0], u.dox[1], packed + head_b[1], D(), u.hid[n], u.dhid[n], st));
    else ARDAE_TRY(dense_bwd(act, R, h, u.dox[0], D(), packed + head_b[0], u.hid[n], u.dhid[n], st));
    ARDAE_TRY(stack.bwd(packed, act, R, u.hid.data(), u.dhid.data(), st));
    return dense_bwd(ACT_NONE, R, zd(), u.dhid[1], h, packed + stack.b[0], u.dzq, u.dz, st, u.dzq);   // act' == 1: S is only a placeholder
  }
  // the heads' problems, then layers 1 .. n
  void wgrads(WgradList& wl, int R, const float* z, const Bufs& u) const {
    for (int k = 0; k < nh; ++k) wl.push(R, head[k].out, head[k].in, u.dox[k], u.hid[stack.n()], head[k].in, wl.g(head[k].w), head[k].in, wl.g(head[k].b));
    stack.wgrads(wl, R, z, u.hid.data(), u.dhid.data());
  }

  // ardae_model_decode: workspace floats (mode 2) and the call (out1: the entry point has asked for it where nh == 2, CAP_GAUSS_DECODER)
  size_t decode_floats(size_t R) const {
    Bump ws;
    Bufs u;
    carve(ws, R, false, u);
    return ws.off;
  }
  int decode(const float* params, const float* packed, int act, const float* z, int R, float* workspace, size_t wsf, float* out0, float* out1,
             hipStream_t st) const {
    Bump ws(workspace, wsf);
    Bufs u;
    carve(ws, (size_t)R, false, u);
    ARDAE_CHECK_ARG(ws.ok, "model_decode: workspace too small");
    float* const out[2] = {out0, out1};
    return fwd(params, packed, act, R, z, u.hid.data(), out, st);
  }
};

// the descriptor rules of the implicit MLP families (allowed: the flag bits the family knows)
inline int mlp_desc_check(const ardae_model_desc* d, int allowed) {
  ARDAE_TRY(desc_flags_ok(d, allowed));
  ARDAE_CHECK_ARG(d->input_dim >= 1 && d->noise_dim >= 1 && d->h_dim >= 1 && d->z_dim >= 1 && d->n_layers >= 1 && d->n_layers <= 4, "model: bad dimensions");
  ARDAE_CHECK_ARG(d->act > ACT_NONE && d->act <= ACT_LAST, "model: unknown activation %d (relu, softplus, elu, tanh, leaky_relu, swish)", d->act);
  return 0;
}

// the `decode` member of a Family whose Packed holds its MlpDecoder as `dec` (and whose Layout the activation as `act`)
template <class Layout, class Packed>
int mlp_decode(const ardae_model_desc& d, const float* params, const float* packed, const float* z, int R, float* workspace, size_t wsf, float* out0,
               hipStream_t st, float* out1) {
  const Layout P(d);
  return Packed(P).dec.decode(params, packed, P.act, z, R, workspace, wsf, out0, out1, st);
}

}  // namespace ardae
