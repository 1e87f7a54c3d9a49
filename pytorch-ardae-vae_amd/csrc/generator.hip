// The implicit generator of notebooks/ardae_fit.ipynb (`Generator.main`): Linear(z_dim, h) -> act -> [Linear(h, h) -> act] x (L - 1) ->
// Linear(h, D), as a device network: an MlpStack (mlp.h) and one linear head.  Forward from a noise batch, backward from an output seed
// (every weight gradient in one batch), and a front end that draws the noise and computes the first layer in one kernel.
#include <vector>

#include "ardae_hip.h"
#include "front_layer.h"
#include "mlp.h"
#include "philox.h"
#include "profile.h"

namespace ardae {
namespace {

constexpr int GEN_ZMAX = 16;     // widest noise the fused front end takes as plain FMAs
constexpr int GEN_MAX_LAYERS = 16;

struct GenLayout {
  int zd, h, L, D, act;
  std::vector<Lin> lin;   // the L hidden layers, main.{0, 2, ...}
  Lin head;               // main.{2 L}
  size_t total = 0;
  GenLayout(int z_dim, int h_dim, int n_layers, int out_dim, int act_) : zd(z_dim), h(h_dim), L(n_layers), D(out_dim), act(act_) {
    size_t off = 0;
    for (int l = 0; l < L; ++l) lin.push_back(next_lin(off, h, l == 0 ? zd : h));
    head = next_lin(off, D, h);
    total = off;
  }
};

struct GenPacked {
  MlpStack stack;
  size_t head_f, head_b;
  GenPacked(const GenLayout& P, PackList& pl) : stack(P.lin.data(), P.lin.size(), pl) { pl.pair(P.head, head_f, head_b); }
  explicit GenPacked(const GenLayout& P, PackList&& sizing = PackList()) : GenPacked(P, sizing) {}   // offsets only
};

// a[1 .. L] (a[1] is the arena's first piece: the fused front end fills it), then their gradients d[1 .. L]
struct GenWs { std::vector<float*> a, d; };
void carve(const GenPacked& K, Bump& ws, int B, GenWs& W) {
  K.stack.carve(ws, (size_t)B, W.a);
  K.stack.carve(ws, (size_t)B, W.d);
}
// the head's problem, then layers 1 .. L; scratch out of the arena
void gen_wgrads(const GenLayout& P, const GenPacked& K, const GenWs& W, int B, const float* z, const float* dx, WgradList& wl, Bump& ws) {
  wl.push(B, P.D, P.h, dx, W.a[P.L], P.h, wl.g(P.head.w), P.h, wl.g(P.head.b));
  K.stack.wgrads(wl, B, z, W.a.data(), W.d.data());
  wl.assign(ws, P.L + 1);
}

bool shape_ok(int z_dim, int h_dim, int n_layers, int out_dim, int act) {
  return z_dim >= 1 && h_dim >= 1 && n_layers >= 1 && n_layers <= GEN_MAX_LAYERS && out_dim >= 1 && act > ACT_NONE && act <= ACT_LAST &&
         z_dim <= (1 << 16) && h_dim <= (1 << 16) && out_dim <= (1 << 16);
}
bool fused_ok(int z_dim, int h_dim, int n_layers, int out_dim, int act) {
  return shape_ok(z_dim, h_dim, n_layers, out_dim, act) && z_dim <= GEN_ZMAX && (h_dim == 64 || h_dim == 128 || h_dim == 256);
}
#define GEN_CHECK_DESC(what)                                                                                                               \
  ARDAE_CHECK_ARG(shape_ok(z_dim, h_dim, n_layers, out_dim, act),                                                                           \
                  what ": bad network (z_dim=%d, h_dim=%d, n_layers=%d, out_dim=%d, act=%d): dimensions >= 1, n_layers 1 .. 16, an activation", \
                  z_dim, h_dim, n_layers, out_dim, act)
#define GEN_CHECK_BATCH(what) \
  ARDAE_CHECK_ARG(B > 0 && (int64_t)B * std::max(h_dim, std::max(z_dim, out_dim)) < (int64_t)1 << 31, what ": bad batch (B=%d)", B)

// One workgroup per tile of 64 rows.  Phase 1: the tile's 16 z_dim Philox counters (one per thread; tile row 0 = element 64 tile z_dim of
// the draw, a multiple of 4) - z written out and kept in LDS.  Phase 2: front_first_layer.  Elements at or beyond B z_dim (a last partial
// tile) are drawn like the others and written nowhere.
__global__ __launch_bounds__(256) void gen_draw_fwd_kernel(int B, int zd, uint64_t seed, uint64_t offset, const StepState* __restrict__ state,
                                                           float* __restrict__ z_out, const float* __restrict__ W1, const float* __restrict__ b1,
                                                           int h, int act, float* __restrict__ h1) {
  __shared__ __attribute__((aligned(16))) float zb[FRONT_ROWS * GEN_ZMAX];
  const int t = threadIdx.x;
  const int row0 = blockIdx.x * FRONT_ROWS;
  const uint64_t base_off = state ? state->rng_offset : 0;
  if (t < 16 * zd) {
    float v[4];
    const int64_t e0 = (int64_t)row0 * zd + 4 * t, n = (int64_t)B * zd;
    philox_normal4(seed, offset + base_off, (uint64_t)(e0 >> 2), v);
    *reinterpret_cast<f32x4*>(zb + 4 * t) = f32x4{v[0], v[1], v[2], v[3]};
    if (e0 + 4 <= n && (reinterpret_cast<uintptr_t>(z_out) & 15) == 0) {
      *reinterpret_cast<f32x4*>(z_out + e0) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
      for (int i = 0; i < 4 && e0 + i < n; ++i) z_out[e0 + i] = v[i];
    }
  }
  __syncthreads();
  front_first_layer<GEN_ZMAX, false>(zb, nullptr, zd, row0, B, W1, zd, b1, h, act, h1);
}

// everything behind the first layer: layers 2 .. L and the head
int forward_from(const GenLayout& P, const GenPacked& K, const GenWs& W, const float* params, const float* packed, const float* z, int B,
                 float* x_out, size_t first, hipStream_t st) {
  ARDAE_TRY(K.stack.fwd(params, packed, P.act, B, z, W.a.data(), st, first));
  return dense_fwd(ACT_NONE, B, P.D, W.a[P.L], P.h, P.h, packed + K.head_f, params + P.head.b, x_out, st);
}

}  // namespace
}  // namespace ardae

using namespace ardae;

extern "C" {

size_t ardae_gen_param_floats(int z_dim, int h_dim, int n_layers, int out_dim, int act) {
  return shape_ok(z_dim, h_dim, n_layers, out_dim, act) ? GenLayout(z_dim, h_dim, n_layers, out_dim, act).total : 0;
}

size_t ardae_gen_packed_floats(int z_dim, int h_dim, int n_layers, int out_dim, int act) {
  if (!shape_ok(z_dim, h_dim, n_layers, out_dim, act)) return 0;
  const GenLayout P(z_dim, h_dim, n_layers, out_dim, act);
  PackList pl;
  const GenPacked K(P, pl);
  return pl.total();
}

size_t ardae_gen_workspace_floats(int z_dim, int h_dim, int n_layers, int out_dim, int act, int B) {
  if (!shape_ok(z_dim, h_dim, n_layers, out_dim, act) || B <= 0) return 0;
  const GenLayout P(z_dim, h_dim, n_layers, out_dim, act);
  const GenPacked K(P);
  Bump ws;
  GenWs W;
  carve(K, ws, B, W);
  WgradList wl(nullptr);
  gen_wgrads(P, K, W, B, nullptr, nullptr, wl, ws);
  return ws.off;
}

int ardae_gen_pack(int z_dim, int h_dim, int n_layers, int out_dim, int act, const float* params, float* packed, void* stream) {
  GEN_CHECK_DESC("gen_pack");
  ARDAE_CHECK_ARG(params && packed, "gen_pack: null pointer argument");
  const GenLayout P(z_dim, h_dim, n_layers, out_dim, act);
  PackList pl(params, packed);
  const GenPacked K(P, pl);
  return pl.launch((hipStream_t)stream);
}

int ardae_gen_forward(int z_dim, int h_dim, int n_layers, int out_dim, int act, const float* params, const float* packed, const float* z,
                      int B, float* workspace, size_t workspace_floats, float* x_out, void* stream) {
  GEN_CHECK_DESC("gen_forward");
  GEN_CHECK_BATCH("gen_forward");
  ARDAE_CHECK_ARG(params && packed && z && workspace && x_out, "gen_forward: null pointer argument");
  const GenLayout P(z_dim, h_dim, n_layers, out_dim, act);
  const GenPacked K(P);
  Bump ws(workspace, workspace_floats);
  GenWs W;
  carve(K, ws, B, W);
  ARDAE_CHECK_ARG(ws.ok, "gen_forward: workspace too small");
  return forward_from(P, K, W, params, packed, z, B, x_out, 1, (hipStream_t)stream);
}

int ardae_gen_backward(int z_dim, int h_dim, int n_layers, int out_dim, int act, const float* params, const float* packed, const float* z,
                       const float* dx, int B, float* workspace, size_t workspace_floats, float* grads, void* stream) {
  GEN_CHECK_DESC("gen_backward");
  GEN_CHECK_BATCH("gen_backward");
  ARDAE_CHECK_ARG(params && packed && z && dx && workspace && grads, "gen_backward: null pointer argument");
  const GenLayout P(z_dim, h_dim, n_layers, out_dim, act);
  const GenPacked K(P);
  Bump ws(workspace, workspace_floats);
  GenWs W;
  carve(K, ws, B, W);
  WgradList wl(grads);
  gen_wgrads(P, K, W, B, z, dx, wl, ws);
  ARDAE_CHECK_ARG(ws.ok, "gen_backward: workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  // d_L = (dx W_head) (.) act'(a_L), then down the stack; the input gets no gradient
  ARDAE_TRY(dense_bwd(P.act, B, P.h, dx, P.D, packed + K.head_b, W.a[P.L], W.d[P.L], st));
  ARDAE_TRY(K.stack.bwd(packed, P.act, B, W.a.data(), W.d.data(), st));
  return wl.launch(st);
}

int ardae_gen_draw_fused_ok(int z_dim, int h_dim, int n_layers, int out_dim, int act) { return fused_ok(z_dim, h_dim, n_layers, out_dim, act) ? 1 : 0; }

int ardae_gen_draw_forward(int z_dim, int h_dim, int n_layers, int out_dim, int act, const float* params, const float* packed, int B,
                           uint64_t seed, uint64_t offset, const void* state, float* z_out, float* workspace, size_t workspace_floats,
                           float* x_out, void* stream) {
  GEN_CHECK_DESC("gen_draw_forward");
  GEN_CHECK_BATCH("gen_draw_forward");
  ARDAE_CHECK_ARG(fused_ok(z_dim, h_dim, n_layers, out_dim, act),
                  "gen_draw_forward: shape not eligible (ardae_gen_draw_fused_ok): use ardae_philox_normal_at + ardae_gen_forward");
  ARDAE_CHECK_ARG(params && packed && z_out && workspace && x_out, "gen_draw_forward: null pointer argument");
  const GenLayout P(z_dim, h_dim, n_layers, out_dim, act);
  const GenPacked K(P);
  Bump ws(workspace, workspace_floats);
  GenWs W;
  carve(K, ws, B, W);
  ARDAE_CHECK_ARG(ws.ok, "gen_draw_forward: workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  prof_begin(st, "gen_draw_fwd_kernel", 2.0 * (double)B * h_dim * z_dim, 4.0 * ((double)B * h_dim + (double)B * z_dim));
  hipLaunchKernelGGL(gen_draw_fwd_kernel, dim3((unsigned)ceil_div(B, FRONT_ROWS)), dim3(256), 0, st, B, z_dim, seed, offset, (const StepState*)state,
                     z_out, params + P.lin[0].w, params + P.lin[0].b, h_dim, act, W.a[1]);
  prof_end(st);
  ARDAE_LAUNCH_CHECK();
  return forward_from(P, K, W, params, packed, z_out, B, x_out, 2, st);
}

}  // extern "C"
