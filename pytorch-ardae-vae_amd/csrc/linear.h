// Fused "linear" kernel family:  Y = epilogue( sum_s X_s[M,K_s] * Wp_s^T )  on FP32 MFMA (gfx950).
//
// Replaces the reference's `MLP.forward` Linear->act chain (models/layers.py:501-515) and, with the
// derivative epilogues, the autograd passes PyTorch builds for it (first backward, the
// create_graph=True score pass of models/graddae/mlp.py:35-36,437 and its double backward).
#pragma once
#include <stdarg.h>

#include <type_traits>

#include "ardae_hip.h"
#include "common.h"
#include "profile.h"

namespace ardae {

using LinSrc = ardae_lin_src;
using LinArgs = ardae_linear_args;   // value-initialise: `LinArgs a{};`

enum Epi : int {
  EPI_ACT = ARDAE_EPI_ACT,
  EPI_DACT = ARDAE_EPI_DACT,
  EPI_CHAIN = ARDAE_EPI_CHAIN,
  EPI_DAE_LOSS = ARDAE_EPI_DAE_LOSS
};

// number of floats of the packed image of an [nout, k] matrix
size_t packed_floats(int nout, int k);
// rows per row-tile of the geometry launch_linear() picks for this Nout (colsum / tile_loss sizing)
int linear_row_tile(int M, int nout);
int linear_row_tiles(int M, int nout);
int linear_col_panels(int M, int nout);

// M[n][k] = transpose ? W[k*ldw + n] : W[n*ldw + k]
int launch_pack_weight(const float* W, int ldw, int nout, int k, bool transpose, float* out, hipStream_t st);
int launch_linear(const LinArgs& a, int epi, hipStream_t st);
// pack many matrices with one launch (the per-step refresh of a network's weight images)
struct PackItem { const float* W; int ldw, nout, k, transpose; float* out; };
constexpr int PACK_BATCH_MAX = 48;
int launch_pack_batch(const PackItem* items, int n, hipStream_t st);
// split-K 32 x 32 kernel for the per-image (B-row) problems (linear_small.hip): latency, not throughput
bool linear_small_eligible(const LinArgs& a, int epi);
int launch_linear_small(const LinArgs& a, int epi, hipStream_t st);
// two INDEPENDENT per-image problems of one epilogue kind in one launch where both run on the split-K kernel (else two launches)
int launch_linear_pair(const LinArgs& a0, const LinArgs& a1, int epi, hipStream_t st);
// a run of row-local K = Nout = 256 layers as one layer-major launch of the weight-stationary kernel (linear_wide.hip)
bool linear_wide_layers_eligible(const LinArgs* L, int nl, int epi);
int launch_linear_wide_layers(const LinArgs* L, int nl, int epi, hipStream_t st);
// a dependent CHAIN of per-image levels (one or two independent problems each, probs[i] on level level_of[i], levels ascending) in
// ONE launch with a row-block counter hand-over between the levels (linear_small.hip); counters: scratch of
// LINEAR_SMALL_CHAIN_COUNTER_WORDS words (one 128-byte line) per 16-row block, 32 x ceil(M / 16) words in all
constexpr int LINEAR_SMALL_CHAIN_COUNTER_WORDS = 32;
int launch_linear_small_chain(const LinArgs* probs, const int* epis, const int* level_of, int nprob, float* counters, hipStream_t st);
// streaming kernel for N-row layers with Nout <= 32 and K = 256 (linear_narrow.hip): HBM-bound
bool linear_narrow_eligible(const LinArgs& a, int epi);
int launch_linear_narrow(const LinArgs& a, int epi, hipStream_t st);
// N-row forward layers with K <= 128 that is not a multiple of 32 (linear_shortk.hip): A fragments stay in registers
bool linear_shortk_eligible(const LinArgs& a, int epi);
int launch_linear_shortk(const LinArgs& a, int epi, hipStream_t st);
// that layer fused with the latent-space layer behind it (N2 <= 32 columns): the hidden rows never reach memory
bool sampler_tail_eligible(const LinArgs& first, int n2);
int launch_sampler_tail(const LinArgs& first, const float* wp2, const float* bias2, float* Z, int ldz, int n2, hipStream_t st,
                        const float* wp2b = nullptr, const float* bias2b = nullptr, float* Zb = nullptr, int ldzb = 0);   // second head (mean | logvar)
// software-pipelined 64 x 256 kernel (linear_wide.hip): full tiles, K % 32 == 0
bool linear_wide_eligible(const LinArgs& a, int epi);
int launch_linear_wide(const LinArgs& a, int epi, hipStream_t st);

// row-local CHAINS of K = Nout = 256 layers in one launch (linear_chain.hip): the small-shard regime (few tiles per workgroup)
bool linear_chain_eligible(const LinArgs* layers, int nl, int epi);
int launch_linear_chain(const LinArgs* layers, int nl, int epi, hipStream_t st);

// ----------------------------------------------------------------------------------------------
// The launch layer's shared host code.  launch_linear() validates once (validate_linear, before any eligibility rule); the
// launchers below it only pick a template instantiation and report their cost.
// ----------------------------------------------------------------------------------------------
int validate_linear(const LinArgs& a, int epi);

// The activations a kernel family is instantiated for, in the order its dispatcher tries them.
template <int... ACTS>
struct ActList {};
using ActsAll = ActList<ACT_NONE, ACT_RELU, ACT_SOFTPLUS, ACT_ELU, ACT_TANH, ACT_LEAKY, ACT_SWISH>;   // linear_kernel, per-image blocks: ACT, DACT
using ActsChainEpi = ActList<ACT_SOFTPLUS, ACT_RELU, ACT_ELU, ACT_TANH, ACT_LEAKY, ACT_SWISH>;        // ... their CHAIN (no second derivative of the identity)
using ActsShipped = ActList<ACT_RELU, ACT_SOFTPLUS, ACT_NONE>;                                        // wide ACT / DACT, short-K, sampler tail
using ActsSoftplus = ActList<ACT_SOFTPLUS>;                                                           // wide CHAIN
using ActsHidden = ActList<ACT_SOFTPLUS, ACT_RELU>;                                                   // layer chains, layer runs, the per-image pair

// f(std::integral_constant<int, A>{}) for the first A of the list that equals `act`; ACT_UNLISTED when none does (the caller
// raises its family's error).  A LEFT fold: the compiler meets, and emits, the kernels behind f in list order - a translation
// unit's device code keeps its layout when a ladder of `if (act == A) return launch<A>(..)` is rewritten as a list.
constexpr int ACT_UNLISTED = INT32_MIN;
template <int... ACTS, typename F>
inline int dispatch_act(ActList<ACTS...>, int act, F&& f) {
  int rc = ACT_UNLISTED;
  (void)(... || (act == ACTS && ((rc = f(std::integral_constant<int, ACTS>{})), true)));
  return rc;
}

// The profile log's cost model (bench.py builds its roofline from it): algorithmic flops and bytes - X read once, `tensors`
// operands / results of M x Nout floats read or written once, the weights once.
struct LinCost {
  double flops = 0, bytes = 0;
  LinCost& operator+=(const LinCost& o) { flops += o.flops; bytes += o.bytes; return *this; }
};
inline LinCost lin_cost(double M, double Nout, double ksum, double tensors) {
  return {2.0 * M * Nout * ksum, 4.0 * (M * ksum + tensors * M * Nout + ksum * Nout)};
}
inline LinCost lin_cost(const LinArgs& a, double tensors) {
  double ksum = 0;
  for (int s = 0; s < a.nsrc; ++s) ksum += a.src[s].K;
  return lin_cost(a.M, a.Nout, ksum, tensors);
}
// Y, Y2 and what the epilogue reads per element: S (DACT, CHAIN), R (CHAIN), Q (DACT)
inline double epi_tensors(const LinArgs& a, int epi) {
  return 1.0 + (a.Y2 ? 1 : 0) + ((epi == EPI_DACT || epi == EPI_CHAIN) ? 1 : 0) + ((epi == EPI_CHAIN) ? 1 : 0) + ((epi == EPI_DACT && a.Q) ? 1 : 0);
}
// the problems of one launch; tensors(problem) -> its count
template <typename F>
inline LinCost lin_cost_sum(const LinArgs* probs, int n, F&& tensors) {
  LinCost c;
  for (int i = 0; i < n; ++i) c += lin_cost(probs[i], tensors(probs[i]));
  return c;
}
// prof_begin under a printf-style name; call it behind `if (g_prof_enabled)`, so that an unprofiled launch computes no cost
__attribute__((format(printf, 3, 4))) inline void prof_begin_named(hipStream_t st, const LinCost& c, const char* fmt, ...) {
  char name[128];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(name, sizeof(name), fmt, ap);
  va_end(ap);
  prof_begin(st, name, c.flops, c.bytes);
}

}  // namespace ardae
