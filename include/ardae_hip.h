/* ardae_hip.h  --  C ABI of libardae_hip.so: the MI355X (gfx950) engine for the AR-DAE-VAE inner training loop.
 *
 * The reference (lim0606/pytorch-ardae-vae) has no FFI of its own: its hot path is PyTorch autograd over
 * Python modules.  This header is the boundary a maintainer binds instead (ctypes stub: INTEGRATION.md);
 * each entry point names the reference code (file:line under the reference root) it replaces.
 *
 * Conventions (all entry points):
 *   - plain pointers are DEVICE pointers to fp32 unless the name says `host_`; the caller owns all memory,
 *     nothing is retained past the call, nothing is allocated or freed by the library;
 *   - `stream` is a hipStream_t (pass PyTorch's current stream); calls are asynchronous and stream-ordered,
 *     no hidden device synchronisation;
 *   - return value: 0 ok, <0 invalid argument, >0 a hipError_t; `ardae_last_error()` has the message;
 *   - matrices are row-major; `nn.Linear` weights are [out, in] exactly as the reference stores them.
 */
#ifndef ARDAE_HIP_H
#define ARDAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARDAE_ABI_VERSION 1

/* activations: reference utils/models.py:14-32 (F.relu, F.softplus beta=1 threshold=20) */
/* get_nonlinear_func (reference utils/models.py:14-32): relu, softplus ('csoftplus' = log(exp(x) + 1) is the same function; it is evaluated in softplus' overflow- and cancellation-free form), elu (alpha 1), tanh, leaky_relu
 * (slope 0.2), swish (x sigmoid(x), utils/models.py:8-10).  Derivatives are rebuilt from saved OUTPUTS; swish is not monotonic, so its
 * forward records the branch (x below / above the minimum at -1.27846) in the lowest mantissa bit of the stored output (<= 1 ulp) and
 * the derivative epilogues invert it by bisection (csrc/common.h::swish_f).  The software-pipelined N-row kernels exist for
 * NONE / RELU / SOFTPLUS (every shipped recipe); ELU / TANH / LEAKY / SWISH layers run on the generic kernels. */
enum { ARDAE_ACT_NONE = 0, ARDAE_ACT_RELU = 1, ARDAE_ACT_SOFTPLUS = 2, ARDAE_ACT_ELU = 3, ARDAE_ACT_TANH = 4, ARDAE_ACT_LEAKY_RELU = 5, ARDAE_ACT_SWISH = 6 };

/* epilogues of ardae_linear */
enum {
  ARDAE_EPI_ACT = 0,      /* Y = act(V + bias[c] + rowbias[r / rows_per_group][c] + rowscale[r] * rowscale_w[c]);
                             if Y2: Y2 = -R[c] * act'(Y)  (R is an [Nout] vector: seed of the score pass)               */
  ARDAE_EPI_DACT = 1,     /* Y = V * act'(S) (+ Q)          : one back-prop step through Linear->act                    */
  ARDAE_EPI_CHAIN = 2,    /* Y = V * act'(S); Y2 = V * R * (1 - act'(S)) : forward-mode step of the double backward    */
  ARDAE_EPI_DAE_LOSS = 3  /* g = V + bias; rho = sigma[r]*g + eps; Y = g; Y2 = 2*sigma*rho*scale; tile_loss += rho^2   */
};

typedef struct ardae_lin_src {
  const float* x;  /* activations [M, K], row stride ld                                   */
  int ld;
  int K;
  const float* wp; /* weight matrix [Nout, K] in the packed image written by ardae_pack_weight */
} ardae_lin_src;

typedef struct ardae_linear_args {
  int M, Nout;
  int nsrc;              /* 1 or 2 operand pairs accumulated into the same output (concat inputs)       */
  ardae_lin_src src[2];
  int act;
  const float* bias;     /* [Nout] or NULL                                                               */
  const float* rowbias;  /* [M / rows_per_group, rowbias_ld] per-image term or NULL                      */
  int rowbias_ld;
  int rows_per_group;
  const float* rowscale;   /* [M] (sigma) or NULL                                                        */
  const float* rowscale_w; /* [Nout]                                                                     */
  const float* S; int ldS; /* saved post-activation                                                      */
  const float* R; int ldR;
  const float* Q; int ldQ;
  const float* sigma;      /* [M]   (EPI_DAE_LOSS)                                                       */
  const float* eps; int ldeps;
  float scale;
  float* Y;  int ldY;
  float* Y2; int ldY2;
  float* colsum;     /* optional [ardae_linear_row_tiles(M,Nout), Nout] per-tile column sums of Y       */
  float* tile_loss;  /* [row_tiles * col_panels] partial sums (EPI_DAE_LOSS)                             */
} ardae_linear_args;

const char* ardae_last_error(void);
int ardae_abi_version(void);

/* ---- K1: fused Linear(+concat)(+act / derivative epilogue) on FP32 MFMA -----------------------------------
 * replaces models/layers.py:501-515 (MLP.forward) and the autograd passes over it.                          */
size_t ardae_packed_floats(int nout, int k);
int ardae_linear_row_tiles(int M, int nout);
int ardae_linear_col_panels(int M, int nout);
/* M[n][k] = transpose ? W[k*ldw + n] : W[n*ldw + k]  ->  MFMA-lane-linear image (out: ardae_packed_floats) */
int ardae_pack_weight(const float* W, int ldw, int nout, int k, int transpose, float* out, void* stream);
int ardae_linear(const ardae_linear_args* args, int epilogue, void* stream);
/* A row-local CHAIN of nl layers (layer l's input = layer l - 1's Y) in ONE launch: the workgroup keeps its 64-row tile in LDS
 * between layers and reloads the next layer's weight slab behind the current layer's MFMAs - what the N-row passes of the cDAE
 * update (models/graddae/mlp.py:400-444: forward, score, forward-mode and backward runs of h x h layers) use when a rank's shard
 * is only a few tiles per CU (data-parallel runs).  Results are bit-identical to nl calls of ardae_linear.
 * ardae_linear_chain_eligible: 1 if the shapes qualify (K = Nout = 256, M % 64 == 0, few row tiles, one epilogue kind). */
int ardae_linear_chain_eligible(const ardae_linear_args* layers, int nl, int epilogue);
int ardae_linear_chain(const ardae_linear_args* layers, int nl, int epilogue, void* stream);
/* The same run LAYER-major for MANY tiles per workgroup (the full-size shard): one launch of the weight-stationary N-row kernel walks all
 * its row tiles for layer l (the wave's weight slab loaded once per layer, as in a launch of its own), then layer l + 1 on the rows it has
 * written itself - no hand-over between workgroups, no dispatch ramp / drain between the layers.  Bit-identical to nl calls of ardae_linear.
 * Eligible: K = Nout = 256, every layer reading its predecessor's Y, one epilogue kind / activation (relu, softplus) / set of operands
 * (forward layers with a bias only; DACT all with Q or all without; CHAIN). */
int ardae_linear_wide_layers_eligible(const ardae_linear_args* layers, int nl, int epilogue);
int ardae_linear_wide_layers(const ardae_linear_args* layers, int nl, int epilogue, void* stream);


/* ---- K6w: batched weight gradients  dW[o][i] = sum_pairs sum_m G[m][o] X[m][i]  -------------------------------
 * replaces the grad_weight / grad_bias products of autograd's Linear backward executed by
 * cdae_loss.backward() (ivae_ardae.py:771) and model_loss.backward() / latent.backward(grad) (:804,:834).      */
#define ARDAE_WGRAD_MAX_PROBLEMS 20
typedef struct ardae_wgrad_problem {
  int M, O, I;
  int npairs;                 /* 1 or 2 (G,X) pairs summed into the same dW                                  */
  const float* G[2]; int ldG[2]; /* [M, O] output-side factors                                               */
  const float* X[2]; int ldX[2]; /* [M, I] input-side factors                                                */
  int bias_pair;              /* pair whose G is column-summed into out_bias / out_rowscale, or -1           */
  const float* rowscale;      /* optional [M]: out_rowscale[o] = sum_m rowscale[m] * G[bias_pair][m][o]      */
  int splits;                 /* row splits: ardae_wgrad_splits, or any value >= 1 (it sizes partial and
                               * partial_vec; the launch sizes nothing from it and may use fewer: the tiled
                               * kernels run min(256 / tiles in their launch, smallest splits in it))       */
  float* partial;             /* scratch [splits, O, I]                                                      */
  float* partial_vec;         /* scratch [splits, 2, O] (needed when bias_pair >= 0)                         */
  float* out; int ldout;      /* [O, I] view of the gradient buffer (row stride ldout)                       */
  float* out_bias;            /* [O] or NULL                                                                 */
  float* out_rowscale; int ld_rowscale; /* strided [O] (one column of an [O, *] matrix) or NULL              */
  float beta;                 /* out = beta*out + sum                                                        */
} ardae_wgrad_problem;
int ardae_wgrad_splits(int M, int O, int I, int nproblems_hint);
int ardae_wgrad_batch(const ardae_wgrad_problem* problems, int nproblems, void* stream);


/* ---- helper kernels ---------------------------------------------------------------------------------------- */
/* ivae_ardae.py:753-761 + models/graddae/mlp.py:21-23:  u = s(z - z0[b]); std_b = delta*mean_d(std_nz(u)) (unbiased);
 * sigma[b,i] = std_b*xi[b,i]; xbar = u + sigma*eps.   latent [B,nz,z], z0 [B,z], xi [B*nz], eps [B*nz,z]            */
int ardae_latent_perturb(const float* latent, const float* z0, const float* xi, const float* eps, int B, int nz, int z,
                         float std_scale, float delta, float* xbar, float* sigma, float* std_b, void* stream);
/* --train-nstd-cdae > 1 (ivae_ardae.py:759-767): every one of the nz sample rows is used nstd times, each with its own sigma and eps;
 * the statistics are those of the nz samples.  xi [B*nz*nstd], eps / xbar [B*nz*nstd, z], sigma [B*nz*nstd]; row (b, i, j) <- latent[b, i] */
int ardae_latent_perturb_nstd(const float* latent, const float* z0, const float* xi, const float* eps, int B, int nz, int nstd, int z,
                              float std_scale, float delta, float* xbar, float* sigma, float* std_b, void* stream);
/* The same perturbation with its two draws made INSIDE the kernel (ivae_ardae.py:761 `torch.randn_like(std)` and
 * models/graddae/mlp.py:21-23 `add_gaussian_noise`): no xi / eps inputs; the kernel generates the Philox counters of its image's rows,
 * keyed exactly like ardae_philox_normal_at (element i of this rank's rows = element first_row [* z] + i of the global draw with
 * (seed, offset_xi / offset_eps [+ the step state's base offset])), and writes the eps rows to eps_out for the DAE loss.  Same
 * numbers as two ardae_philox_normal_at calls followed by ardae_latent_perturb, two launches and 2 x N (z + 1) floats of HBM traffic
 * less.  ardae_latent_perturb_draw_ok: 1 if (nz, nstd, z) qualifies (nstd == 1, z a power of two, nz % 4 == 0, nz z <= 8192). */
int ardae_latent_perturb_draw_ok(int nz, int nstd, int z);
int ardae_latent_perturb_draw(const float* latent, const float* z0, int B, int nz, int z, float std_scale, float delta, uint64_t seed,
                              uint64_t offset_xi, uint64_t offset_eps, const void* state, uint64_t first_row, float* xbar, float* sigma,
                              float* eps_out, float* std_b, void* stream);
/* u = s (z - z0[b])  (ivae_ardae.py:827) */
int ardae_center_scale(const float* latent, const float* z0, int B, int nz, int z, float std_scale, float* u, void* stream);
/* Philox4x32-10 counter RNG (replaces torch.randn at ivae/mnist.py:73, ivae_ardae.py:761, graddae/mlp.py:22) */
int ardae_philox_normal(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);
int ardae_philox_uniform(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);
/* dynamic binarisation x ~ Bernoulli(p[col]) (datasets/mnist.py:36-40) */
int ardae_bernoulli(const float* p, int64_t rows, int cols, float* out, uint64_t seed, uint64_t offset, void* stream);
/* utils/optim.py:49-108 (vendored Adam, eps before the bias correction); vmax non-NULL = amsgrad; step >= 1 */
int ardae_adam_ref_step(float* p, const float* g, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, int64_t n,
                        double lr, double beta1, double beta2, double eps, int step, void* stream);
/* Device-resident step state, so that a whole train step (ivae_ardae.py:707-846) can be captured once in a HIP graph and
 * replayed: kernel arguments are frozen at capture, the 32-byte state block is not.  Layout: u64 rng_offset, i64 adam_step,
 * f32 lr/(1-beta1^t), f32 sqrt(1-beta2^t); zero-initialise it.  `advance` (first node of the step) adds rng_inc to the
 * Philox base offset, increments t and refreshes the two Adam coefficients (utils/optim.py:84-104, computed in double);
 * the _dev variants read the state instead of taking offset / step by value (offset = state.rng_offset + offset_add). */
#define ARDAE_STEP_STATE_BYTES 32
int ardae_step_state_advance(void* state, uint64_t rng_inc, double lr, double beta1, double beta2, void* stream);
int ardae_philox_normal_dev(float* out, int64_t n, uint64_t seed, const void* state, uint64_t offset_add, void* stream);
/* Elements [first_element, first_element + n) of the draw identified by (seed, offset + state.rng_offset): a rank that holds
 * rows [r0, r1) of a [rows, cols] draw passes first_element = r0 * cols (a multiple of 4) and gets exactly the numbers a single
 * process would have put there, so a data-parallel run does not depend on the number of ranks.  state may be NULL. */
int ardae_philox_normal_at(float* out, int64_t n, uint64_t seed, uint64_t offset, const void* state, uint64_t first_element,
                           void* stream);
int ardae_adam_ref_step_dev(float* p, const float* g, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, int64_t n,
                            double beta1, double beta2, double eps, const void* state, void* stream);
/* The TRAIN STATE: the step state with the KL weight of the coming step in its last 8 bytes - f32 beta (bytes 24..27), f32 seed_scale
 * (bytes 28..31), which no step-state consumer reads - so that a captured step replays through --beta-annealing (ivae_ardae.py:704).
 * `ardae_train_state_advance` does what ardae_step_state_advance does and then, for the new t and i = t - 1 (the reference's zero-based
 * i_ep), in double, every operation rounded on its own and in this order (utils/msc.py:53-55, the host's Python arithmetic bit for bit):
 *   beta = beta_annealing < 0 ? beta_fin : beta_init + (beta_fin - beta_init) / beta_annealing * min(beta_annealing, i)
 *   seed_scale = std_scale * beta / seed_rows      the factor of the entropy seed, ivae_ardae.py:834 (seed_rows = B * nz of the VAE batch)
 * each rounded to float once.  beta_annealing == 0 and seed_rows <= 0 are argument errors.  The `_dev` twins of the entry points that
 * take `float beta` / `float seed_scale` (ardae_model_vae_forward_dev, ..., ardae_log_scalars_dev) take the block in its place; the
 * kernels are the value forms' own, reading the float through a pointer. */
int ardae_train_state_advance(void* state, uint64_t rng_inc, double lr, double beta1, double beta2, double beta_init, double beta_fin,
                              int64_t beta_annealing, double std_scale, int64_t seed_rows, void* stream);
/* g[i] *= state.seed_scale, i < n: the entropy seed of the single-call backward (ardae_model_vae_backward_dev takes dz_extra scaled) */
int ardae_seed_scale_dev(float* g, int64_t n, const void* state, void* stream);
/* Weight averaging of the model parameters: --m-weight-avg swa | polyak (torchcontrib.optim.SWA / Polyak around the model
 * optimiser, ivae_ardae.py:158-164,559-565, freq 1).  t = model-optimiser steps done, the current one included: state.adam_step
 * when state is non-NULL (read on the device: a captured step replays correctly), else the argument t.  origin = the t of the
 * first averaging step (start + 1).  t < origin: avg is not written; t == origin: avg = p (a copy); t > origin, k = t - origin:
 *   avg = avg + (p - avg) * w,  w = fp32(1 / (k + 1)) (SWA) | fp32(1 - decay) (Polyak), each operation rounded separately.
 * avg and p must not overlap; float4 accesses where both share their offset inside 16 bytes, scalar ones otherwise. */
#define ARDAE_WEIGHT_AVG_SWA 0
#define ARDAE_WEIGHT_AVG_POLYAK 1
int ardae_weight_avg(float* avg, const float* p, int64_t n, int kind, double decay, int64_t origin, const void* state, int64_t t,
                     void* stream);
/* torch.optim.RMSprop(lr, momentum) as built at ivae_ardae.py:625-626 (alpha .99, eps 1e-8, not centred) */
int ardae_rmsprop_step(float* p, const float* g, float* square_avg, float* momentum_buffer, int64_t n, double lr,
                       double alpha, double eps, double momentum, void* stream);
/* torch.optim.SGD as ivae_ardae.py:546-547 (model) / :613-614 (cDAE) construct it - lr only: p -= lr g */
int ardae_sgd_step(float* p, const float* g, int64_t n, double lr, void* stream);

/* ---- K4-K6: conditional AR-DAE (models/graddae/mlp.py:341-483, models/resdae/mlp.py:286-413) -----------------
 * Parameters live in ONE flat fp32 buffer in the reference's named_parameters() order
 * (ctx_encode.layers.*, ctx_encode.fc, inp_encode.*, neglogprob.* | dae.*), each tensor [out,in] row-major. */
typedef struct ardae_cdae_desc {
  int kind;        /* 0 = mlp-grad (MLPGradCARDAE: score = input-gradient of an energy MLP), 1 = mlp-res (direct score);
                    * 2 / 3 = the same two WITHOUT a context (MLPGradARDAE / MLPResARDAE, see "unconditional AR-DAE" below);
                    * 6 / 7 = the plain DAEs, without a context and without the sigma input (MLPGradDAE / MLPResDAE, see "plain DAE"
                    * below); 10 / 11 = the plain CONDITIONAL DAEs, kinds 0 / 1 without the sigma input (MLPGradCDAE / MLPResCDAE, see
                    * "plain conditional DAE" below); 13 = the conditional DAE WITHOUT an input encoder (MLPCDAE with enc_input=False, see
                    * "reconstruction DAE" below); 16 / 17 = kinds 0 / 1 WITHOUT an input encoder (MLPGradCARDAE / MLPResCARDAE with
                    * enc_input=False, see "conditional AR-DAE without an input encoder" below).  4, 5, 8, 9 and 12 are not kinds */
  int input_dim;   /* z */
  int context_dim; /* c  (kinds 0 / 1 / 10 / 11 / 13 / 16 / 17: >= 1; kinds 2 / 3 / 6 / 7: 0) */
  int h_dim;
  int n_layers;    /* --cdae-n-layers */
  int act;         /* any ARDAE_ACT_* but NONE (with a piecewise linear one mlp-grad's second-order terms are zero)  */
} ardae_cdae_desc;
size_t ardae_cdae_param_floats(const ardae_cdae_desc* d);
size_t ardae_cdae_packed_floats(const ardae_cdae_desc* d);
size_t ardae_cdae_workspace_floats(const ardae_cdae_desc* d, int B, int S, int need_grads);
/* refresh the MFMA-packed weight images after every optimiser step */
int ardae_cdae_pack(const ardae_cdae_desc* d, const float* params, float* packed, void* stream);
/* ConditionalARDAE.forward + loss.backward() fused: DAE loss  mean((sigma*score(xbar|ctx,sigma) + eps)^2)  and the
 * gradient of every parameter (graddae/mlp.py:400-444 + ivae_ardae.py:771).  xbar [B*S,z] (already perturbed),
 * sigma [B*S], eps [B*S,z], ctx [B,c]; loss: device scalar; grads: flat buffer (parameter layout), OVERWRITTEN
 * except neglogprob.fc.bias which receives no gradient in the reference and is left untouched; score_out optional. */
int ardae_cdae_loss_grads(const ardae_cdae_desc* d, const float* params, const float* packed, const float* xbar,
                          const float* sigma, const float* eps, const float* ctx, int B, int S, float* workspace,
                          size_t workspace_floats, float* loss, float* grads, float* score_out, void* stream);
/* North star "fused per-sample Gaussian-perturb + sigma-scaling + DAE-forward kernel": ivae_ardae.py:753-776 in one call.  ONE kernel per
 * image draws xi / eps (Philox, keyed as ardae_latent_perturb_draw), computes the latent statistics, sigma and xbar = u + sigma eps
 * (graddae/mlp.py:21-23, ivae_ardae.py:753-767) and - the rows still in LDS - the first layer of the score network's input encoder,
 * a_1 = act(xbar A_1^T + b_1) (graddae/mlp.py:414-434), written into the cDAE workspace; the rest is ardae_cdae_loss_grads from layer 2 on.
 * xbar / sigma / eps_out / std_b are written as by ardae_latent_perturb_draw (the weight gradient of A_1 and the DAE-loss layer read them).
 * ardae_cdae_perturb_fused_ok: 1 if the shape qualifies (nstd == 1, the draw kernel's conditions, z % 8 == 0, z <= 64, nz % 32 == 0,
 * h % 32 == 0, relu / softplus; kinds 0 / 1 / 16 / 17 - the kernel draws sigma, so 0 for kinds 10 / 11); otherwise call ardae_latent_perturb* and
 * ardae_cdae_loss_grads.  Kinds 16 / 17: the layer is the energy MLP's own first one, see below. */
int ardae_cdae_perturb_fused_ok(const ardae_cdae_desc* d, int nz, int nstd);
int ardae_cdae_perturb_loss_grads(const ardae_cdae_desc* d, const float* params, const float* packed, const float* latent, const float* z0,
                                  const float* ctx, int B, int nz, float std_scale, float delta, uint64_t seed, uint64_t offset_xi,
                                  uint64_t offset_eps, const void* state, uint64_t first_row, float* xbar, float* sigma, float* eps_out,
                                  float* std_b, float* workspace, size_t workspace_floats, float* loss, float* grads, void* stream);
/* ConditionalARDAE.glogprob (graddae/mlp.py:446-483): score at x [B*S,z] for noise level sigma [B*S] */
int ardae_cdae_score(const ardae_cdae_desc* d, const float* params, const float* packed, const float* x,
                     const float* sigma, const float* ctx, int B, int S, float* workspace, size_t workspace_floats,
                     float* score_out, void* stream);

/* ---- conditional AR-DAE without an input encoder (the same classes with enc_input=False): ardae_cdae_desc.kind 16 / 17 -----------
 * With enc_input=False the reference drops inp_encode and the last MLP reads the perturbed sample itself beside the encoded context and the noise
 * level: neglogprob / dae = MLP(z + h + 1, h, ...).  Kind 16 (MLPGradCARDAE) is an energy kind: the score is the input-gradient of the energy MLP;
 * kind 17 (MLPResCARDAE) a direct-score kind.  Parameters in named_parameters() order: ctx_encode.layers.{0..L-2}.{weight,bias}, ctx_encode.fc.*,
 * then neglogprob.layers.{0..L-1}.*, neglogprob.fc.* (kind 16) or dae.layers.*, dae.fc.* (kind 17); layers.0.weight is [h, z + h + 1] =
 * [W1x | W1c | w1s], so h_1 = act(W1x x_bar + sigma w1s + [W1c c_L + d_1](b)): the context half enters as a row bias computed once per image, the
 * sigma column as for kinds 0 / 1.  context_dim >= 1 and ctx non-NULL.  ardae_cdae_param_floats / packed_floats / workspace_floats / pack /
 * loss_grads / score take the two kinds; the workspace is smaller than kind 0 / 1's at equal shape (no a_l, r_l, tau_l, pbar_l of an input encoder).
 * The update: kind 17 is kind 1's with every inp_encode term removed (what kind 13 is to kind 11: one ordinary backward from the seed); kind 16 is
 * the unconditional kind 2's (score pass g = e_1 W1x, tangent chain, backward) with the context bias in layer 1 and the backward of ctx_encode
 * through the per-image reduction of layer 1's pre-activation gradient, first- and second-order contributions both, as kind 0 forms it for W1c;
 * it leaves neglogprob.fc.bias's gradient untouched.  Launch decisions: kind 17 follows kind 13, kind 16 kind 0 on the per-image branch and kind 2
 * on the N-row runs (its N == B score takes the general path).
 * ardae_cdae_perturb_fused_ok follows the rule above.  ardae_cdae_perturb_loss_grads for these kinds: ctx_encode and the row bias
 * cb[b] = W1c c_L + d_1 run first (B rows); then one kernel per image draws xi / eps, computes the statistics, sigma and x_bar as for kinds 0 / 1
 * (the same bits as ardae_latent_perturb_draw) and - the rows still in LDS - writes h_1 = act(x_bar W1x^T + sigma[r] w1s + cb[b]) where
 * ardae_cdae_loss_grads would have put the first N-row layer's output (with L = 1, kind 16, also the score pass's seed e_1); the rest is
 * ardae_cdae_loss_grads from layer 2 on, and the context chain does not run a second time.  Measured, the fused form does not beat the draw +
 * perturb launch followed by the stand-alone layer beyond the run-to-run spread (profiles/noenc_score_timing.json), so the engines do not use
 * it for these kinds unless asked to. */

/* ---- unconditional AR-DAE (models/graddae/mlp.py:118-207, models/resdae/mlp.py:92-167): ardae_cdae_desc.kind 2 / 3 -------------
 * The score network on [x_bar | sigma] alone: MLP(input_dim + 1, h, 1) whose input-gradient is the score (kind 2, MLPGradARDAE)
 * or MLP(input_dim + 1, h, input_dim) that is the score (kind 3, MLPResARDAE).  context_dim must be 0.  Parameters in the
 * reference's named_parameters() order: neglogprob.layers.{0..L-1}.{weight,bias}, neglogprob.fc.* (kind 2) / main.layers.*,
 * main.fc.* (kind 3); layers.0.weight is [h, d + 1] = [W1x | w1s].  ardae_cdae_param_floats / packed_floats / workspace_floats /
 * pack / loss_grads / score take these kinds with ctx == NULL (anything else is an argument error) and N = B * S rows in any
 * factorisation; kind 2 leaves neglogprob.fc.bias's gradient untouched like kind 0.
 *
 * ardae_dae_perturb: add_gaussian_noise on a broadcast batch (graddae/mlp.py:21-23 after the notebooks'
 * x.unsqueeze(1).expand(B, nsigma, d)): xbar[(b, j)] = fma(sigma[(b, j)], eps[(b, j)], x[b]); the broadcast is never written. */
int ardae_dae_perturb(const float* x /* [B, d] */, const float* sigma /* [B*nsigma] */, const float* eps /* [B*nsigma, d] */,
                      int B, int nsigma, int d, float* xbar, void* stream);
/* Draw + perturbation + first layer in ONE kernel over 64-row tiles of the N = B * nsigma rows, then ardae_cdae_loss_grads from
 * layer 2 on.  Row r of the call = element first_row + r of the global sigma draw (seed, offset_sigma [+ state.rng_offset]) and
 * elements (first_row + r) d ... of the eps draw, keyed exactly like ardae_philox_normal_at (first_row a multiple of 4):
 * sigma = delta * n (one multiply), xbar = fma(sigma, eps, x[b]); xbar, sigma, eps_out are written as the three separate launches
 * would, and h_1 = act(W1x xbar + sigma w1s + d_1) goes into the workspace slot ardae_cdae_loss_grads reads.
 * ardae_dae_perturb_fused_ok: 1 if (d, h, L, act, nsigma) qualifies (kind 2 / 3, input_dim <= 8, h_dim 64 | 128 | 256,
 * n_layers >= 2, nsigma >= 1; any N - a last partial tile is masked); otherwise: ardae_philox_normal_at x 2, sigma *= delta,
 * ardae_dae_perturb, ardae_cdae_loss_grads. */
int ardae_dae_perturb_fused_ok(const ardae_cdae_desc* d, int nsigma);
int ardae_dae_perturb_loss_grads(const ardae_cdae_desc* d, const float* params, const float* packed, const float* x, int B, int nsigma,
                                 float delta, uint64_t seed, uint64_t offset_sigma, uint64_t offset_eps, const void* state,
                                 uint64_t first_row, float* xbar, float* sigma, float* eps_out, float* workspace,
                                 size_t workspace_floats, float* loss, float* grads, void* stream);

/* ---- plain DAE (models/graddae/mlp.py:39-116, models/resdae/mlp.py:27-90; notebooks/dae_toy.ipynb): ardae_cdae_desc.kind 6 / 7 ------
 * The score network that is NOT amortised over the noise level: MLP(input_dim, h, 1) on x_bar alone whose input-gradient is the
 * score (kind 6, MLPGradDAE, graddae/mlp.py:57,88-92) or MLP(input_dim, h, input_dim) that is the score (kind 7, MLPResDAE,
 * resdae/mlp.py:45,73).  context_dim must be 0 and ctx NULL, as for kinds 2 / 3.  Parameters in named_parameters() order:
 * neglogprob.layers.{0..L-1}.{weight,bias}, neglogprob.fc.* (kind 6) / main.layers.*, main.fc.* (kind 7); layers.0.weight is
 * [h, d] - there is no sigma column.  ardae_cdae_param_floats / packed_floats / workspace_floats / pack / loss_grads / score take
 * these kinds, N = B * S rows in any factorisation; the update is the one of kinds 2 / 3 with every sigma-column term removed.  The
 * loss is unchanged, mean((sigma[r] g + eps)^2) with a per-row sigma [N] (graddae/mlp.py:96: `std * glogprob` broadcasts a float or
 * a tensor alike); ardae_cdae_score ignores `sigma` (NULL allowed), as DAE.glogprob ignores std (graddae/mlp.py:101-116).  Kind 6
 * leaves neglogprob.fc.bias's gradient untouched like kinds 0 / 2.
 *
 * ardae_dae_noise_perturb: add_gaussian_noise (graddae/mlp.py:21-23) with ONE noise level on a broadcast batch:
 * xbar[(b, j)] = fma(s, eps[(b, j)], x[b]) and sigma_out[r] = s for all N = B * nsigma rows, where s is the f32 in bytes 24..27 of
 * the block `dae_state` (ardae_dae_state_advance) when that is non-NULL, else the argument `sigma`.  The update is then
 * ardae_philox_normal_at (eps), ardae_dae_noise_perturb, ardae_cdae_loss_grads; a fused draw + perturbation + first-layer kernel like
 * ardae_dae_perturb_loss_grads' was built and measured, and did not pay. */
int ardae_dae_noise_perturb(const float* x /* [B, d] */, const float* eps /* [B*nsigma, d] */, int B, int nsigma, int d, float sigma,
                            const void* dae_state, float* xbar, float* sigma_out /* [B*nsigma] */, void* stream);
/* The DAE STATE: the step state with the noise level of the coming step as f32 in bytes 24..27 (the train state's beta slot; bytes
 * 28..31 stay zero), so that a captured step replays through the notebook's sigma annealing (dae_toy.ipynb's training cell).
 * `ardae_dae_state_advance` does what ardae_step_state_advance does and then, for the new t and i = t - 1 (the notebook's i_ep), in
 * double, every operation rounded on its own and in the notebook's order, rounded to float once:
 *   perc = min((i + 1) / (double)sigma_annealing, 1.0);  sigma = sigma_max * (1 - perc) + sigma_min * perc
 * sigma_annealing <= 0: the constant sigma_min. */
int ardae_dae_state_advance(void* state, uint64_t rng_inc, double lr, double beta1, double beta2, double sigma_max, double sigma_min,
                            int64_t sigma_annealing, void* stream);

/* ---- plain conditional DAE (models/graddae/mlp.py:210-339, models/resdae/mlp.py:170-284): ardae_cdae_desc.kind 10 / 11 ----------------
 * ConditionalDAE, the conditional score network that is NOT amortised over the noise level (MLPGradCDAE, kind 10: score = input-gradient
 * of an energy MLP; MLPResCDAE, kind 11: the MLP's output is the score).  Parameters in the order of kinds 0 / 1 - ctx_encode.*,
 * inp_encode.*, neglogprob.* (kind 10) / dae.* (kind 11) - but layers.0.weight is [h, 2h] = [W1a | W1c]: there is no sigma column,
 * h_1 = act(W1a a_L + [W1c c_L + d_1](b)).  context_dim >= 1 and ctx non-NULL, as for kinds 0 / 1.  ardae_cdae_param_floats /
 * packed_floats / workspace_floats / pack / loss_grads / score take these kinds; the update is the one of kinds 0 / 1 with every
 * sigma-column term removed, and every launch decision is the sibling's (kind 10: kind 0's, the one-launch chain of the N == B score pass
 * included; kind 11: kind 1's).  The loss is unchanged, mean((sigma[r] g + eps)^2) with a per-row sigma [N]; ardae_cdae_score ignores
 * `sigma` (NULL allowed), as ConditionalDAE.glogprob never reads std.  Kind 10 leaves neglogprob.fc.bias's gradient untouched.
 * ardae_cdae_perturb_fused_ok and ardae_dae_perturb_fused_ok are 0 for these kinds (those kernels draw sigma); a fused first-layer kernel
 * did not pay for kinds 6 / 7 and none is built here.
 *
 * ardae_latent_noise_perturb: ivae_ardae.py:753-767 with ONE noise level, the counterpart of ardae_latent_perturb_nstd:
 * u = std_scale (latent[b, i] - z0[b]), rounded as ardae_center_scale rounds it; xbar[(b, i, j)] = fma(s, eps[(b, i, j)], u) and
 * sigma_out[r] = s for all N = B * nz * nstd rows, where s is the f32 in bytes 24..27 of `dae_state` (ardae_dae_state_advance) when
 * that is non-NULL, else the argument `sigma`.  latent [B, nz, z], z0 [B, z], eps / xbar [N, z]; the broadcast over j is never written.
 * ardae_latent_noise_perturb_draw: the same with eps made in the kernel, the counterpart of ardae_latent_perturb_draw: element i of the
 * call's rows = element first_row * z + i of the draw (seed, offset_eps [+ dae_state's rng_offset]), keyed exactly like
 * ardae_philox_normal_at (first_row a multiple of 4), written to eps_out; xbar / sigma_out / eps_out hold the bits of
 * ardae_philox_normal_at followed by ardae_latent_noise_perturb.  64-row tiles, a last partial tile is masked.
 * ardae_latent_noise_perturb_draw_ok: 1 for every positive (nz, nstd, z). */
int ardae_latent_noise_perturb(const float* latent, const float* z0, const float* eps, int B, int nz, int nstd, int z, float std_scale, float sigma,
                               const void* dae_state, float* xbar, float* sigma_out, void* stream);
int ardae_latent_noise_perturb_draw_ok(int nz, int nstd, int z);
int ardae_latent_noise_perturb_draw(const float* latent, const float* z0, int B, int nz, int nstd, int z, float std_scale, float sigma,
                                    const void* dae_state, uint64_t seed, uint64_t offset_eps, uint64_t first_row, float* xbar, float* sigma_out,
                                    float* eps_out, void* stream);

/* ---- reconstruction DAE (models/dae/mlp.py: DAE :21-82 = MLPDAE, ConditionalDAE :85-193 = MLPCDAE): kinds 7 / 11 / 13 --------------------
 * The classical denoising autoencoders: x_recon = main(x_bar), loss = mse(x_recon, x) (dae/mlp.py:49-70,131-165), and the score read off the
 * residual, glogprob = (main(x) - x) / std^2 (:72-82,167-193).  The loss layer is not new: ardae_cdae_loss_grads forms rho = sigma y + eps, and
 * with sigma = 1, eps = -x that is y - x exactly, so loss and gradients on a given x_bar are ardae_cdae_loss_grads of the res-kind network on
 * (x_bar, 1, -x) with score_out = x_recon.  MLPDAE's network is kind 7's (`main.*`), MLPCDAE's with enc_input=True kind 11's.
 *
 * ardae_cdae_desc.kind 13: ConditionalDAE with enc_input=False (its default), the conditional direct-output network WITHOUT an input encoder:
 * the last MLP reads the perturbed sample itself beside the encoded context (dae/mlp.py:116-120,151-159).  Parameters in named_parameters()
 * order: ctx_encode.*, dae.*, with dae.layers.0.weight [h, z + h] = [W1x | W1c]; no sigma column.  h_1 = act(W1x x_bar + [W1c c_L + d_1](b)): the
 * context half enters as a row bias, once per context row.  context_dim >= 1, ctx non-NULL, N = B * S rows in the caller's factorisation (one
 * context per row: B = N, S = 1).  ardae_cdae_param_floats / packed_floats / workspace_floats / pack / loss_grads / score take it; the update is
 * kind 11's with every inp_encode term removed (k1 = z): one ordinary backward from the seed, W1x's gradient = ghat_1 (x) x_bar, W1c's through the
 * per-image reduction over S.  ardae_cdae_score gives the network's output and ignores `sigma`.  ardae_cdae_perturb_fused_ok and
 * ardae_dae_perturb_fused_ok are 0 for it.  12 is not a kind (an even number would be an energy kind).
 *
 * ardae_philox_uniform_at: torch.rand_like of add_uniform_noise (dae/mlp.py:16-18): the [0, 1) map of ardae_philox_uniform, (word >> 8) 2^-24,
 * keyed like ardae_philox_normal_at - elements [first_element, first_element + n) of the draw (seed, offset + state.rng_offset), the same numbers
 * for any partition.  first_element and n may be any values (a first or last counter may be partial).  state may be NULL. */
int ardae_philox_uniform_at(float* out, int64_t n, uint64_t seed, uint64_t offset, const void* state, uint64_t first_element, void* stream);
/* ardae_recon_perturb: add_noise (dae/mlp.py:12-18,40-47) on a broadcast batch with ONE noise level: row (b, j) of the N = B * nsigma rows reads
 * x[b] (the broadcast is never written).  noise 0 (gaussian): xbar = fma(s, draw, x); noise 1 (uniform, draw in [0, 1)):
 * xbar = x + ((2 s) draw - s), each operation rounded on its own, the reference's order.  s is the f32 in bytes 24..27 of `dae_state`
 * (ardae_dae_state_advance) when that is non-NULL, else the argument `sigma`.  It also writes what the loss layer reads: sigma_out[r] = 1 and
 * target_out[r, k] = -x[b, k].  draw / xbar / target_out [N, d], sigma_out [N].
 * ardae_recon_perturb_draw: the same with the draw made in the kernel: element i of the call's rows = element first_row * d + i of the draw
 * (seed, offset [+ dae_state's rng_offset]), keyed exactly like ardae_philox_normal_at / ardae_philox_uniform_at (first_row a multiple of 4),
 * written to draw_out; xbar / sigma_out / target_out / draw_out hold the bits of the stand-alone draw followed by ardae_recon_perturb.  64-row
 * tiles, a last partial tile is masked. */
int ardae_recon_perturb(const float* x /* [B, d] */, const float* draw /* [B*nsigma, d] */, int B, int nsigma, int d, int noise, float sigma,
                        const void* dae_state, float* xbar, float* sigma_out, float* target_out, void* stream);
int ardae_recon_perturb_draw(const float* x, int B, int nsigma, int d, int noise, float sigma, const void* dae_state, uint64_t seed, uint64_t offset,
                             uint64_t first_row, float* xbar, float* sigma_out, float* target_out, float* draw_out, void* stream);
/* The conditional engine's counterparts, next to ardae_latent_noise_perturb(_draw): u = std_scale (latent[b, i] - z0[b]), rounded as
 * ardae_center_scale rounds it (ivae_ardae.py:753-767); xbar = perturb(u) as above, target_out = -u, sigma_out = 1; rows (b, i, j) of the
 * N = B * nz * nstd rows.  latent [B, nz, z], z0 [B, z], draw / xbar / target_out [N, z]. */
int ardae_latent_recon_perturb(const float* latent, const float* z0, const float* draw, int B, int nz, int nstd, int z, float std_scale, int noise,
                               float sigma, const void* dae_state, float* xbar, float* sigma_out, float* target_out, void* stream);
int ardae_latent_recon_perturb_draw(const float* latent, const float* z0, int B, int nz, int nstd, int z, float std_scale, int noise, float sigma,
                                    const void* dae_state, uint64_t seed, uint64_t offset, uint64_t first_row, float* xbar, float* sigma_out,
                                    float* target_out, float* draw_out, void* stream);
/* glogprob's last line (dae/mlp.py:80-81,191-192): out = (recon - x) / s^2 on [n, d]; s from `dae_state` (bytes 24..27) when that is non-NULL,
 * else `sigma` - read on the device, so the caller needs no host synchronisation.  out may alias recon. */
int ardae_recon_score(const float* recon, const float* x, int n, int d, float sigma, const void* dae_state, float* out, void* stream);

/* ---- energy-function fitting (notebooks/ardae_fit.ipynb): energies, the implicit generator, torch.optim.Adam + StepLR -------------
 * One iteration of the notebook: num_dae_updates AR-DAE updates, each on a fresh sample of the generator, then one generator update
 * whose output gradient is (alpha dE/dx + score(x, sigma = 0)) / B.  What changes from iteration to iteration (the Philox base
 * offset, Adam's t and bias corrections, the StepLR learning rate, the annealed energy weight alpha) lives in the FIT STATE, a device
 * block of ARDAE_FIT_STATE_BYTES: its first ARDAE_STEP_STATE_BYTES are the step state (ardae_philox_normal_at / *_dev consumers read
 * it as such), then f32 alpha, f32 lr of the COMING iteration, then f32 alpha, f32 lr of the iteration just done.  Zero-initialise. */
#define ARDAE_FIT_STATE_BYTES 48
/* utils/energy.py: regularization_func alone (any d), energy_func1..4 (each with regularization_func; x is [R, 2]) and
 * normal_energy_func(x, mu, logvar) (any d) */
enum { ARDAE_ENERGY_REG = 0, ARDAE_ENERGY_1 = 1, ARDAE_ENERGY_2 = 2, ARDAE_ENERGY_3 = 3, ARDAE_ENERGY_4 = 4, ARDAE_ENERGY_NORMAL = 5 };
/* energy[r] = E(x[r]) and grad[r] = dE/dx (x[r]) - what autograd returns for the reference's function - for x [R, d]; either output
 * may be NULL.  Evaluated in double per row and rounded once.  mu / logvar: ARDAE_ENERGY_NORMAL only.  Kinds 1 - 4 refuse d != 2. */
int ardae_energy(int kind, const float* x, int R, int d, float mu, float logvar, float* energy, float* grad, void* stream);
/* The generator's output seed of one iteration: seed[r] = (alpha * dE/dx (x[r]) + score[r]) / R, three separately rounded fp32
 * operations on the fp32 gradient of ardae_energy, and mean_energy[0] = mean_r E(x[r]) (a two-stage sum in a fixed order, in double:
 * no atomics).  alpha: the fit state's (coming iteration) when fit_state is non-NULL, else the argument.  partial: scratch of
 * ardae_energy_partial_floats(R) floats. */
size_t ardae_energy_partial_floats(int R);
int ardae_energy_seed(int kind, const float* x, const float* score, int R, int d, float mu, float logvar, float alpha,
                      const void* fit_state, float* seed, float* mean_energy, float* partial, void* stream);
/* The implicit generator (ardae_fit.ipynb `Generator.main`): Linear(z_dim, h) -> act -> [Linear(h, h) -> act] x (n_layers - 1) ->
 * Linear(h, out_dim).  Parameters in ONE flat buffer in named_parameters() order (main.0.weight, main.0.bias, main.2.weight, ...),
 * each weight [out, in] row-major.  n_layers 1 .. 16, act any ARDAE_ACT_* but NONE.
 * forward: x_out [B, out_dim] from z [B, z_dim]; the hidden layers stay in `workspace` for the backward call (same B).
 * backward: grads (flat, parameter layout, OVERWRITTEN) = d <dx, x_out> / d params from the seed dx [B, out_dim], every weight
 * gradient in one ardae_wgrad_batch. */
size_t ardae_gen_param_floats(int z_dim, int h_dim, int n_layers, int out_dim, int act);
size_t ardae_gen_packed_floats(int z_dim, int h_dim, int n_layers, int out_dim, int act);
size_t ardae_gen_workspace_floats(int z_dim, int h_dim, int n_layers, int out_dim, int act, int B);
int ardae_gen_pack(int z_dim, int h_dim, int n_layers, int out_dim, int act, const float* params, float* packed, void* stream);
int ardae_gen_forward(int z_dim, int h_dim, int n_layers, int out_dim, int act, const float* params, const float* packed, const float* z,
                      int B, float* workspace, size_t workspace_floats, float* x_out, void* stream);
int ardae_gen_backward(int z_dim, int h_dim, int n_layers, int out_dim, int act, const float* params, const float* packed, const float* z,
                       const float* dx, int B, float* workspace, size_t workspace_floats, float* grads, void* stream);
/* Draw + first layer in ONE kernel over 64-row tiles: z [B, z_dim] = the draw (seed, offset [+ state.rng_offset]) keyed exactly like
 * ardae_philox_normal_at on B * z_dim elements (written out: the first layer's weight gradient reads it) and h_1 = act(W_1 z + b_1)
 * into the workspace slot ardae_gen_forward would fill; then ardae_gen_forward from layer 2 on.  ardae_gen_draw_fused_ok: 1 if
 * z_dim <= 16 and h_dim is 64, 128 or 256; otherwise ardae_philox_normal_at + ardae_gen_forward. */
int ardae_gen_draw_fused_ok(int z_dim, int h_dim, int n_layers, int out_dim, int act);
int ardae_gen_draw_forward(int z_dim, int h_dim, int n_layers, int out_dim, int act, const float* params, const float* packed, int B,
                           uint64_t seed, uint64_t offset, const void* state, float* z_out, float* workspace, size_t workspace_floats,
                           float* x_out, void* stream);
/* torch.optim.Adam (no amsgrad, no weight decay): m = lerp(m, g, 1 - beta1); v = beta2 v + (1 - beta2) g g;
 * p -= step_size * (m / (sqrt(v) / sqrt(1 - beta2^t) + eps)) - epsilon AFTER the bias correction, unlike ardae_adam_ref_step.
 * step_size = lr / (1 - beta1^t) and sqrt(1 - beta2^t) come from the head of the fit (or step) state. */
int ardae_adam_torch_step_dev(float* p, const float* g, float* exp_avg, float* exp_avg_sq, int64_t n, double beta1, double beta2,
                              double eps, const void* state, void* stream);
/* Advance the fit state to the next iteration (last node of an iteration): the iteration just done keeps its alpha / lr in the
 * second pair, rng_offset += rng_inc, t += 1, and for iteration i = t - 1, in double:
 *   lr_i = max(lr_min, lr0 * lr_gamma^(i / lr_step_size))   the notebook's StepLR (utils/lr_scheduler.py), stepped after the optimiser
 *   step_size = lr_i / (1 - beta1^t), sqrt(1 - beta2^t)     torch.optim.Adam's coefficients
 *   alpha_i = alpha_init + (alpha_fin - alpha_init) / alpha_annealing * min(alpha_annealing, i)   (utils/msc.py:53-55;
 *             alpha_annealing < 0: None, alpha_fin) */
int ardae_fit_state_advance(void* fit_state, uint64_t rng_inc, double lr0, double beta1, double beta2, int64_t lr_step_size,
                            double lr_gamma, double lr_min, double alpha_init, double alpha_fin, int64_t alpha_annealing, void* stream);


/* ---- K2/K8: implicit-posterior VAE (models/ivae/mnist.py, models/ivae/toy.py enc_type='concat') ---------------
 * Parameters: ONE flat fp32 buffer in the reference's named_parameters() order
 *   kind 0 (MNISTIPVAE): encode.inp_encode.{layers.0..n_layers, fc}, encode.fc.{layers.0, fc}, decode.main.{layers.*, fc},
 *                        decode.reparam.logit_fn;   Bernoulli decoder, x rescaled to 2x-1 inside the encoder
 *   kind 1 (ToyIPVAE)  : encode.inp_encode.{layers.0..n_layers-2, fc}, encode.fc.{layers.0..n_layers-1, fc} (ContextConcatMLP:
 *                        every layer eats [hidden, noise]), decode.main.*, decode.reparam.{mean_fn, logvar_fn}; Gaussian decoder
 *   kind 2 (ConvIPVAE) : models/ivae/conv.py (28 x 28 x 1 only)
 *   kind 3 (MNISTAuxIPVAE, models/ivae/auxmnist.py): encode.aux_encode.{main.*, reparam.{mean_fn, logvar_fn}},
 *                        encode.encode.{fc.*, reparam.{mean_fn, logvar_fn}}, decode.main.*, decode.reparam.logit_fn.  Its sampler takes TWO
 *                        draws per call: every `noise` argument of this kind is ONE [rows, noise_dim + z_dim] tensor, row = [eps0 | eps]
 *                        (z0 = mu0 + exp(lv0/2) eps0,  z = mu + exp(lv/2) eps)
 *   kind 4 (MNISTConvAuxIPVAE, models/ivae/auxconv.py): the same hierarchical sampler with two conv trunks
 *                        (encode.aux_encode.{conv1-3, fc, reparam.*}, encode.encode.{conv1-3, fc, reparam.*}) and ConvIPVAE's decoder;
 *                        noise_dim = z0_dim, h_dim = 800 (the fc width), 28 x 28 x 1 only; same noise layout as kind 3
 *   kind 5 (ResConvIPVAE, models/ivae/resconv.py, `--model resconvct-res`: do_center, enc_type 'res-wn-mlp'): weight-normalised
 *                        residual blocks (models/layers2.py:50-93,237-352; models/layers.py:25-85,559-622), each operator's
 *                        parameters in the order direction, scale, bias: encode.inp_encode.{0,2,4,6,8}.{conv_0h,conv_h1,conv_01},
 *                        encode.inp_encode.11.{dot_0h,dot_h1,dot_01}, encode.fc.layers.0.*, encode.fc.fc.*, decode.dec.{0,2}.dot_*,
 *                        decode.dec.{6,8,12,14,17}.conv_*; c_dim 512, h_dim = the ResMLP width, n_layers 1, act ARDAE_ACT_ELU, 28 x 28 x 1
 *   kind 6 (MNISTResConvAuxIPVAE, models/ivae/auxresconv.py, `--model auxresconvct`): the same trunk as encode.inp_encode.enc.*
 *                        (c_dim = h_dim, 450 in the recipe), encode.aux_encode.reparam.{mean_fn,logvar_fn}, encode.encode.fc.0,
 *                        encode.encode.reparam.{mean_fn,logvar_fn} (log-variances clipped 'spm4'), the same decoder; noise_dim = z0_dim,
 *                        noise layout of kind 3; its hidden1a context is h [B, h_dim]
 *   kind 7 (ToyAuxIPVAE, models/ivae/auxtoy.py; `--model auxmlp`): kind 3's networks WITHOUT the 2x - 1 rescale, the Gaussian decoder of
 *                        kind 1 (decode.main.*, decode.reparam.{mean_fn, logvar_fn}), and a SQUARE sampling scheme: a call with nz rows per
 *                        image (nz = q^2, else refused) draws q z0's per image and q z's per z0 (auxtoy.py:215,230: `_nz = int(sqrt(nz))`);
 *                        noise of such a call = [eps0: B q x noise_dim | eps: B q q x z_dim], two consecutive blocks; hidden1a context
 *                        cat(h0, h) [B, 2 h_dim] */
typedef struct ardae_model_desc {
  int kind;     /* 0 .. 7 above; 8 / 9 / 11 / 12: the Gaussian-posterior baselines of vae.py (see "Gaussian-posterior VAE baselines" below; noise_dim 0);
                 * 14 / 15 / 17 / 19: the auxiliary-variable baselines (see "Auxiliary-variable Gaussian baselines", "the hierarchical conv baseline" and
                 * "the hierarchical resconv baseline" below).  10, 13, 16 and 18 are not kinds */
  int input_dim, noise_dim, h_dim, z_dim;
  int n_layers; /* --model-n-layers */
  int act;      /* any ARDAE_ACT_* but NONE; kinds 5 / 6: ARDAE_ACT_ELU */
  int flags;    /* kinds 5 / 6 / 12: ARDAE_MODEL_NO_CENTER = do_center False (--model resconv-res / auxresconv: the trunk sees x, not 2x - 1;
                 * ivae/resconv.py:131-132, vae/auxresconv.py:56-58); 0 elsewhere */
} ardae_model_desc;
enum { ARDAE_MODEL_NO_CENTER = 1,
       /* kind 5 (ResConvIPVAE): the sampler head `encode.fc` (models/ivae/resconv.py:101-116, ivae_ardae.py:323-442), flags bits 1-3:
        * 0 'res-wn-mlp' (--model resconv[ct]-res), 1 'mlp' (resconv[ct]), 2 'res-mlp' (-res2), 3 'res-wn-mlp-lin' (-res3), 4 'res-mlp-lin' (-res4) */
       ARDAE_MODEL_HEAD_SHIFT = 1, ARDAE_MODEL_HEAD_MASK = 7 << 1,
       /* kind 6: MNISTResConvAuxIPVAEClipped (--model auxresconv-clip / auxresconvct-clip, models/ivae/auxresconv2.py:71-72,91): the two
        * log-variance heads WITHOUT the 'spm4' clip, and z0 = mu0 + (std exp(lv0 / 2) + 1) eps0 (`min_std = 1.`).  A sampler call with noise
        * takes it as the unscaled draws (std = 1); a std = 0 pass is a RANDOM draw for this class: ardae_model_encode_hidden_raw */
       ARDAE_MODEL_CLIPPED = 16,
       /* kinds 3 / 7 (MNISTAuxIPVAE / ToyAuxIPVAE): NormalDistribution.clip_logvar of the two Gaussian heads (models/reparam.py:17-41;
        * constructor arguments clip_z0_logvar / clip_z_logvar, models/ivae/auxmnist.py:56-72,144-161) - a code per head:
        * 0 none, 1 'hard' (clamp to [-4, 2]), 2 'softplus', 3 .. 8 'spm10' / 'spm6' / 'spm5' / 'spm4' / 'spm3' / 'spm2'
        * (softplus(x + k) - k), 9 'tanh', 10 '2tanh'.  z0 head: flags bits 8-11, z head: bits 12-15. */
       ARDAE_MODEL_CLIP_Z0_SHIFT = 8, ARDAE_MODEL_CLIP_Z_SHIFT = 12, ARDAE_MODEL_CLIP_MASK = 0xff00 };
size_t ardae_model_param_floats(const ardae_model_desc* d);
size_t ardae_model_packed_floats(const ardae_model_desc* d);
/* mode 0: encode only; mode 1: vae_forward + vae_backward; mode 2: decode only (B = rows, nz = 1); mode 3: encode_pair; mode 4: kinds 14 / 15 / 17 only,
 * ardae_vae_aux_iwae_draw on B images x nz samples */
size_t ardae_model_workspace_floats(const ardae_model_desc* d, int B, int nz, int mode);
int ardae_model_pack(const ardae_model_desc* d, const float* params, float* packed, void* stream);
/* Encoder.forward (ivae/mnist.py:102-121): z[B*nz, z] = f(x[B, input_dim], noise[B*nz, noise_dim]); noise NULL = zeros,
 * i.e. encode(x, std=0) */
int ardae_model_encode(const ardae_model_desc* d, const float* params, const float* packed, const float* x,
                       const float* noise, int B, int nz, float* workspace, size_t workspace_floats, float* z_out,
                       void* stream);
/* The two sampler calls that open a cDAE update (ivae_ardae.py:735,749) on the same images in one pass: z0 = encode(x, std=0)
 * [B, z] and z = forward_hidden(x, nz) [B*nz, z] share the per-image trunk (inp_encode and the image half of the first
 * concat layer), which is computed once.  Workspace: ardae_model_workspace_floats(d, B, nz, 3).
 * phase 0: everything; phase 1: trunk + z0 only (no noise needed yet); phase 2: the B*nz-row part only, reading the trunk a
 * phase-1 call left in the same workspace - so a caller can wait for its noise between the two. */
int ardae_model_encode_pair(const ardae_model_desc* d, const float* params, const float* packed, const float* x,
                            const float* noise, int B, int nz, float* workspace, size_t workspace_floats, float* z0_out,
                            float* z_out, int phase, void* stream);
/* ImplicitPosteriorVAE.forward (ivae/mnist.py:267-301): z_out [B*nz, z]; losses[3] = {loss, recon.mean, prior.mean}
 * (device); activations stay in `workspace` for the backward call */
int ardae_model_vae_forward(const ardae_model_desc* d, const float* params, const float* packed, const float* x,
                            const float* noise, int B, int nz, float beta, float* workspace, size_t workspace_floats,
                            float* z_out, float* losses, void* stream);
int ardae_model_vae_forward_dev(const ardae_model_desc* d, const float* params, const float* packed, const float* x,
                                const float* noise, int B, int nz, const void* state, float* workspace, size_t workspace_floats,
                                float* z_out, float* losses, void* stream);
/* Aux models (kinds 3 and 4): the std = 0 pass of the sampler, returning the latent mean z0 [B, z] (may be NULL) AND the encoder hiddens
 * cat(h0, h) [B, 2 h] that --cdae-ctx-type hidden1a uses as the cDAE context (ivae_ardae.py:737-739, ivae/auxmnist.py:125-132).
 * Workspace: mode 0 with nz = 1. */
int ardae_model_encode_hidden(const ardae_model_desc* d, const float* params, const float* packed, const float* x, int B,
                              float* workspace, size_t workspace_floats, float* z0_out, float* hidden_out, void* stream);
/* The same for the clipped class (kind 6 + ARDAE_MODEL_CLIPPED): raw0 [B, noise_dim] is the unscaled eps0 its z0 keeps at std = 0
 * (z0 = mu0 + raw0; NULL: zeros).  The reference's loop makes TWO such calls per phase with separate draws - one for the context, one for the
 * latent mean (ivae_ardae.py:737-739,748 / 815-817,826) - so z0_out or hidden_out may be NULL here. */
int ardae_model_encode_hidden_raw(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* raw0, int B,
                                  float* workspace, size_t workspace_floats, float* z0_out, float* hidden_out, void* stream);
/* Decoder.forward (ivae/mnist.py:188-199, toy.py:725-737) without the sample: head outputs for z [R, z_dim]:
 * out0 = logits (kind 0) / mean (kind 1) [R, input_dim], out1 = logvar (kind 1) or NULL.  Workspace: mode 2.
 * Used by the IWAE evaluator (ivae/mnist.py:420-425). */
int ardae_model_decode(const ardae_model_desc* d, const float* params, const float* packed, const float* z, int R,
                       float* workspace, size_t workspace_floats, float* out0, float* out1, void* stream);
/* per-row -log p(x|z) and prior energy (utils/vae.py:21-30,36-52; utils/energy.py:69-77): rows = B*nz, x [B, input_dim] */
int ardae_model_loss_rows(const ardae_model_desc* d, const float* out0, const float* out1, const float* x, const float* z,
                          int rows, int nz, float* recon_row, float* prior_row, void* stream);
/* grads = grads_beta*grads + d/dparams [ dloss*loss + <dz_extra, z> ]   (model_loss.backward() and
 * latent.backward(seed), ivae_ardae.py:804,834).  Needs the workspace of the matching vae_forward call. */
int ardae_model_vae_backward(const ardae_model_desc* d, const float* params, const float* packed, const float* x,
                             const float* noise, int B, int nz, float beta, float dloss, const float* dz_extra,
                             float* workspace, size_t workspace_floats, float* grads, float grads_beta, void* stream);
int ardae_model_vae_backward_dev(const ardae_model_desc* d, const float* params, const float* packed, const float* x,
                                 const float* noise, int B, int nz, const void* state, float dloss, const float* dz_extra,
                                 float* workspace, size_t workspace_floats, float* grads, float grads_beta, void* stream);
/* The same backward in two calls, for callers that compute the entropy seed late (ivae_ardae.py:829-834: it needs the UPDATED
 * cDAE): _decoder = model_loss.backward() through the decoder down to dL/dz (:804; needs only the vae_forward workspace, so it
 * can run beside the cDAE update), _sampler = dL/dz += seed_scale * dz_extra (:834), back-propagation through the sampler and
 * all weight gradients.  MLP models (kind 0 / 1); the conv model keeps the single call. */
int ardae_model_vae_backward_decoder(const ardae_model_desc* d, const float* params, const float* packed, const float* x,
                                     const float* noise, int B, int nz, float beta, float dloss, float* workspace,
                                     size_t workspace_floats, void* stream);
int ardae_model_vae_backward_sampler(const ardae_model_desc* d, const float* params, const float* packed, const float* x,
                                     const float* noise, int B, int nz, const float* dz_extra, float seed_scale,
                                     float* workspace, size_t workspace_floats, float* grads, float grads_beta, void* stream);
int ardae_model_vae_backward_decoder_dev(const ardae_model_desc* d, const float* params, const float* packed, const float* x,
                                         const float* noise, int B, int nz, const void* state, float dloss, float* workspace,
                                         size_t workspace_floats, void* stream);
int ardae_model_vae_backward_sampler_dev(const ardae_model_desc* d, const float* params, const float* packed, const float* x,
                                         const float* noise, int B, int nz, const float* dz_extra, const void* state,
                                         float* workspace, size_t workspace_floats, float* grads, float grads_beta, void* stream);


/* ---- Gaussian-posterior VAE baselines (vae.py; models/vae/mnist.py, toy.py, conv.py, resconv.py; csrc/vaemodel.hip, csrc/convvae.hip, csrc/resvae.hip):
 * ardae_model_desc.kind 8 / 9 / 11 / 12 ------
 * The second trainer of the reference: an encoder MLP with a Gaussian head and its analytic KL, no sampler noise, no score network.
 *   kind 8 (MNISTVAE, `vae.py --model mnist`): encode.main.{layers.0..n_layers-2, fc}, encode.reparam.{mean_fn, logvar_fn}, decode.main.{layers.*, fc},
 *                        decode.reparam.logit_fn; Bernoulli decoder, x rescaled to 2x - 1 inside the encoder (vae/mnist.py:54)
 *   kind 9 (ToyVAE, `vae.py --model toy`): the same without the rescale, decode.reparam.{mean_fn, logvar_fn}: Gaussian decoder
 *   kind 11 (MNISTConvVAE, `vae.py --model conv`, models/vae/conv.py; 28 x 28 x 1 only): encode.conv{1,2,3} (the trunk of kind 2 on 2x - 1), encode.fc
 *                        512 -> 800, encode.reparam.{mean_fn, logvar_fn} [z_dim, 800], then kind 2's decoder: decode.fc.{layers.0, fc}, decode.deconv{1,2},
 *                        decode.reparam.logit_fn.  input_dim 784, h_dim 800 (the fc width, as kind 4 records it), n_layers 1, z_dim >= 1; every entry
 *                        point below takes it, with the same workspace modes.  10 is not a kind.
 *   kind 12 (MNISTResConvVAE, `vae.py --model resconv`, models/vae/resconv.py; 28 x 28 x 1 only): the weight-normalised residual trunk of kinds 5 / 6 as
 *                        encode.enc.{0,2,4,6,8}.conv_{0h,h1,01}.{direction,scale,bias} and encode.enc.11.dot_* (512 -> c_dim), the plain Linears
 *                        encode.reparam.{mean_fn, logvar_fn} [z_dim, c_dim] (no log-variance clip), then the decoder of kinds 5 / 6: decode.dec.{0,2}.dot_*,
 *                        decode.dec.{6,8,12,14,17}.conv_*.  input_dim 784, h_dim = c_dim >= 1 (450 in the recipe), n_layers 1, act ARDAE_ACT_ELU, z_dim >= 1;
 *                        flags 0 (do_center: the trunk sees 2x - 1) or ARDAE_MODEL_NO_CENTER (what vae.py passes).  ardae_model_pack composes the effective
 *                        weights as for kinds 5 / 6.  Its decode-only workspace (mode 2) keeps ONE columns scratch for all blocks and, with the fused tail
 *                        below, no buffer of the last stage: about a third of the floats per decoded row of kinds 5 / 6.
 * noise_dim must be 0 and flags 0 (kind 12: 0 or ARDAE_MODEL_NO_CENTER); n_layers 1 .. 4 (kinds 11 / 12: 1).  ardae_model_param_floats / packed_floats / workspace_floats (nz = 1; mode 0: encode_stats, 1: forward +
 * backward, 2: decode) / pack / decode / loss_rows take these kinds; ardae_model_encode and ardae_model_vae_* refuse them (there is no sampler).
 *
 * ardae_vae_forward: mu = M h + m, lv = L h + l on the encoder's last hidden rows h, z = mu + exp(lv / 2) eps,
 *   kld_b = -0.5 sum_c (1 + lv - mu^2 - exp(lv)) (utils/vae.py:78-92), the decoder and the row reconstruction loss;
 *   losses[3] = {mean_b(recon_b + beta kld_b), mean recon, mean kld} as VAE.forward returns them (unscaled: loss_scale enters the backward only).
 *   x [B, input_dim]; eps [B, z_dim], or NULL: drawn in the head kernel - element i = element i of the draw (seed, offset [+ state.rng_offset]),
 *   keyed exactly like ardae_philox_normal_at(out, B z_dim, seed, offset, state, 0).  z_out [B, z_dim]; eps_out [B, z_dim] (the eps used; may be
 *   NULL).  Activations stay in `workspace` for the backward call.  The _dev twins read beta from the train state block `beta_state`.
 * ardae_vae_backward: grads = grads_beta * grads + d/dparams [loss_scale * loss] from the workspace of the matching forward.  With c = loss_scale / B the
 *   head is closed form: dmu = dz + c beta mu, dlv = dz (z - mu) / 2 + c beta (exp(lv) - 1) / 2 (one element-wise launch); every weight gradient
 *   goes out as one ardae_wgrad_batch problem list.
 * ardae_vae_encode_stats: mu, lv [B, z_dim] without a draw (the encoder call of logprob and of the latent plots).  Workspace: mode 0.
 * ardae_vae_head: the head alone on hidden rows hid [B, h_dim] -> mu, lv, z_out [B, z_dim], kld [B], eps_out (may be NULL with variant 1).
 *   variant 1: gauss_head_kernel, ONE launch over 8-row tiles (a masked last row tile, any h_dim; every product sum over ascending k from a
 *   zero accumulator, the bias added after, each row's KL terms added in ascending column order: a row's bits do not depend on B);
 *   variant 2: the unfused launches (two narrow linears, the draw, the reparameterisation, the KL rows); variant 0: what ardae_vae_forward runs - the
 *   fused kernel where ardae_vae_head_fused_ok, unless ARDAE_VAE_HEAD_UNFUSED=1 is set under ARDAE_DEBUG_KNOBS=1.  ardae_vae_head_fused_ok: 1 where
 *   z_dim <= 64 and the rows of both head matrices start on 16 bytes (h_dim a multiple of 4 and both parameter offsets multiples of 4 floats: the
 *   recipe's 300 -> 2 x 32); variant 1 runs for any z_dim <= 64, reading float by float where that does not hold (the toy recipe's z_dim 2, where it only
 *   ties with the unfused launches, which are the default there).  Kind 11: on its 800-wide hidden rows gauss_head_kernel loses to the unfused
 *   launches (51.0 against 19.8 us at 128 x 800 -> 2 x 32), so that kind's variant 1 is another fused head: the two products on the MFMA linears, then ONE
 *   launch for the draw, the reparameterisation and the KL rows (three launches, every output equal to variant 2's bit for bit); ardae_vae_head_fused_ok is 1
 *   for it wherever z_dim <= 64.  Kind 12: variant 1 is gauss_head_kernel, variant 2 the unfused launches, as for kind 8; its default is variant 2
 *   (ardae_vae_head_fused_ok is 0: the recipe's c_dim 450 is no multiple of 4, and the kernel's float-by-float path loses there).
 * ardae_vae_kld_rows: kld[b] = -0.5 sum_c (1 + lv - mu^2 - exp(lv)) from mu, lv [B, z], the terms in double and added over ascending c - the row values
 *   of the head, for callers that hold the statistics (the ELBO rows of the evaluator). */
int ardae_vae_head_fused_ok(const ardae_model_desc* d);
int ardae_vae_kld_rows(const float* mu, const float* lv, int B, int z, float* kld, void* stream);
int ardae_vae_head(const ardae_model_desc* d, const float* params, const float* packed, const float* hid, const float* eps, int B, uint64_t seed,
                   uint64_t offset, const void* state, int variant, float* mu, float* lv, float* z_out, float* eps_out, float* kld, void* stream);
int ardae_vae_forward(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* eps, int B, float beta,
                      float loss_scale, uint64_t seed, uint64_t offset, const void* state, float* workspace, size_t workspace_floats, float* z_out,
                      float* eps_out, float* losses, void* stream);
int ardae_vae_forward_dev(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* eps, int B,
                          const void* beta_state, float loss_scale, uint64_t seed, uint64_t offset, const void* state, float* workspace,
                          size_t workspace_floats, float* z_out, float* eps_out, float* losses, void* stream);
int ardae_vae_backward(const ardae_model_desc* d, const float* params, const float* packed, const float* x, int B, float beta, float loss_scale,
                       float* workspace, size_t workspace_floats, float* grads, float grads_beta, void* stream);
int ardae_vae_backward_dev(const ardae_model_desc* d, const float* params, const float* packed, const float* x, int B, const void* beta_state,
                           float loss_scale, float* workspace, size_t workspace_floats, float* grads, float grads_beta, void* stream);
int ardae_vae_encode_stats(const ardae_model_desc* d, const float* params, const float* packed, const float* x, int B, float* workspace,
                           size_t workspace_floats, float* mu_out, float* lv_out, void* stream);
/* Importance-weighted evaluation under the analytic posterior (VAE.logprob, vae/mnist.py:179-220): for each of B images k samples
 * z = mu + exp(lv / 2) eps and their log-density logq = sum_c -0.5 ((z - mu)^2 / exp(lv) + lv + log 2 pi) (utils/stat.py:65-85), one launch, each
 * sample's sum in double over ascending c.  mu, lv [B, z]; eps [B, k, z], or NULL: element i = element first_element + i of the draw (seed, offset),
 * the numbers ardae_philox_normal_at(out, B k z, seed, offset, NULL, first_element) would write (first_element a multiple of 4: a caller that walks
 * a set in chunks passes the chunk's first image times k z).  z_out [B, k, z], logq [B, k], eps_out [B, k, z] or NULL.  z <= 64.  The prior, the
 * decoder, the row losses and the log-mean-exp are ardae_model_decode, ardae_model_loss_rows and ardae_iwae_reduce. */
int ardae_vae_iwae_draw(const float* mu, const float* lv, const float* eps, int B, int k, int z, uint64_t seed, uint64_t offset,
                        uint64_t first_element, float* z_out, float* logq, float* eps_out, void* stream);

/* ---- Auxiliary-variable Gaussian baselines (vae.py --model auxmnist | auxtoy; models/vae/auxmnist.py, auxtoy.py; csrc/auxvae.hip):
 * ardae_model_desc.kind 14 / 15 ------
 * The Gaussian counterparts of kinds 3 / 7: q(z0 | x) q(z | z0, x) with an auxiliary decoder r(z0 | z, x).  13 is not a kind.
 *   kind 14 (MNISTAuxVAE, `vae.py --model auxmnist`, the "# hierarchical mlp" baseline of run_vae_dbmnist.sh): aux_encode.main.{layers.0..n_layers-2, fc},
 *                        aux_encode.reparam.{mean_fn, logvar_fn} [noise_dim, h]; encode.fc.{layers.*, fc} (first weight [h, input_dim + noise_dim]),
 *                        encode.reparam.{mean_fn, logvar_fn} [z_dim, h]; decode.main.*, decode.reparam.logit_fn; aux_decode.fc.{layers.*, fc} (first weight
 *                        [h, input_dim + z_dim]), aux_decode.reparam.{mean_fn, logvar_fn} [noise_dim, h].  x rescaled to 2x - 1 in all three encoders.
 *   kind 15 (ToyAuxVAE, `vae.py --model auxtoy`): the same without the rescale, decode.reparam.{mean_fn, logvar_fn}: Gaussian decoder.
 * 1 <= noise_dim <= 128 (the width of z0), z_dim >= 1 (<= 128 for ardae_vae_aux_iwae_draw), n_layers 1 .. 4; flags: only the ARDAE_MODEL_CLIP_Z0 code
 * (aux_encode's clip_logvar, codes 0 .. 10 as for kinds 3 / 7) - the other two heads take no clip.  ardae_model_param_floats / packed_floats /
 * workspace_floats (mode 0: encode_stats, 1: forward + backward, 2: decode - nz = 1 each - and mode 4: ardae_vae_aux_iwae_draw on B images x nz samples)
 * / pack / decode / loss_rows take these kinds; ardae_model_encode and ardae_model_vae_* refuse them.  The ardae_vae_* entry points above take them with
 * these meanings:
 * ardae_vae_forward: eps is ONE tensor [B, noise_dim + z_dim], row = [eps0 | eps] (kind 3's layout), or NULL: with q = (B noise_dim + 3) / 4 * 4,
 *   eps0 element i = element i and eps element j = element q + j of the draw (seed, offset [+ state.rng_offset]) - what
 *   ardae_philox_normal_at(out, B noise_dim, seed, offset, state, 0) and ardae_philox_normal_at(out, B z_dim, seed, offset, state, q) write.  eps_out has
 *   eps' shape, z_out is [B, z_dim], losses[3] = {mean_b(recon_b + beta (kld_b + aux_kld_b)), mean recon, mean (kld + aux_kld)} with
 *   aux_kld_b = -0.5 sum_c (1 - lvp + lv0 - (exp(lv0) + (mu0 - mup)^2) / exp(lvp)) (utils/vae.py:94-114; one launch, added into the head's KL rows).
 * ardae_vae_backward: with c = loss_scale / B the auxiliary decoder's head is seeded in closed form, dmup = c beta (mup - mu0) / exp(lvp),
 *   dlvp = c beta (1 - (exp(lv0) + (mu0 - mup)^2) / exp(lvp)) / 2, the first head gets dmu0 = dz0 + c beta (mu0 - mup) / exp(lvp),
 *   dlv0 = dz0 (z0 - mu0) / 2 + c beta (exp(lv0) / exp(lvp) - 1) / 2 and then the clip's derivative, and dz is the decoder's part + the auxiliary
 *   decoder's + the head seed of kinds 8 / 9.  One ardae_wgrad_batch problem list.
 * ardae_vae_encode_stats: mu0, lv0 (clipped) [B, noise_dim] of q(z0 | x).  ardae_vae_head / ardae_vae_head_fused_ok: the encode.reparam head on encode.fc's
 *   hidden rows, with kind 8's variants and policy.
 * ardae_vae_pair_kld_rows: kld[b] = -0.5 sum_c (1 - lv2 + lv1 - (exp(lv1) + (mu1 - mu2)^2) / exp(lv2)) from [B, n] statistics, n <= 128: the row values of
 *   loss_kld_gaussian_vs_gaussian, the terms in double and added over ascending c (a row's bits do not depend on B); it mirrors ardae_vae_kld_rows.
 * ardae_vae_aux_iwae_draw: VAE.logprob's three stochastic stages (vae/auxmnist.py:381-451, sample_size2 = 1) for B images x k samples: k z0's per image
 *   from mu0, lv0 [B, noise_dim] (ardae_vae_encode_stats), one z per z0 from q(z | z0, x), and ONE combined row
 *   logq [B, k] = log q(z0 | x) + log q(z | z0, x) - log r(z0 | z, x) - each a sum in double over ascending c (utils/stat.py:65-85), combined in double
 *   in that order.  z_out [B, k, z_dim].  The caller goes on with ardae_model_decode, ardae_model_loss_rows and ardae_iwae_reduce as for kind 8.
 *   eps [B, k, noise_dim + z_dim] (rows [eps0 | eps]) or NULL: with g = first_image + b, eps0 of (b, s, c) is element (g k + s) noise_dim + c of the
 *   draw (seed, offset0) and eps of (b, s, c) element (g k + s) z_dim + c of the draw (seed, offset1) - so a set walked in chunks draws the same
 *   numbers whatever the chunk length; first_image k noise_dim and first_image k z_dim must be multiples of 4.  eps_out: eps' shape, or NULL.
 *   Workspace: mode 4 with nz = k.  (ARDAE_AUX_DRAW_STAGES=1 | 2 under ARDAE_DEBUG_KNOBS=1 stops the call after that stage and leaves logq unwritten:
 *   tools/time_vae_aux_baseline.py times the stages that way.)
 * ardae_vae_aux_elbo_rows: the rows of one forward at beta = 1 (evaluate_iws' ELBO, vae.py:360): recon_rows [B] and kld_rows [B] = kld_b + aux_kld_b, the
 *   values ardae_vae_forward averages.  eps [B, noise_dim + z_dim] or NULL: eps0 of (b, c) is element (first_image + b) noise_dim + c of the draw
 *   (seed, offset0), eps of (b, c) element (first_image + b) z_dim + c of the draw (seed, offset1); first_image noise_dim and first_image z_dim must be
 *   multiples of 4.  Workspace: mode 1. */
int ardae_vae_aux_elbo_rows(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* eps, int B, uint64_t seed,
                            uint64_t offset0, uint64_t offset1, uint64_t first_image, float* workspace, size_t workspace_floats, float* recon_rows,
                            float* kld_rows, void* stream);
int ardae_vae_pair_kld_rows(const float* mu1, const float* lv1, const float* mu2, const float* lv2, int B, int n, float* kld, void* stream);
int ardae_vae_aux_iwae_draw(const ardae_model_desc* d, const float* params, const float* packed, const float* x, const float* mu0, const float* lv0,
                            const float* eps, int B, int k, uint64_t seed, uint64_t offset0, uint64_t offset1, uint64_t first_image, float* workspace,
                            size_t workspace_floats, float* z_out, float* logq, float* eps_out, void* stream);

/* ---- the hierarchical conv baseline of vae.py (models/vae/auxconv.py; csrc/auxconvvae.hip): ardae_model_desc.kind 17 ------
 * The Gaussian counterpart of kind 4, `vae.py --model auxconv` (the "# hierarchical conv" baseline of run_vae_dbmnist.sh).  16 is not a kind.
 *   kind 17 (MNISTConvAuxVAE; 28 x 28 x 1 only): aux_encode.{conv1,2,3, fc 512 -> 800, reparam.{mean_fn, logvar_fn} [noise_dim, 800]},
 *                        encode.{conv1,2,3, fc (512 + noise_dim) -> 800, reparam.* [z_dim, 800]}, kind 11's decoder, aux_decode.{conv1,2,3,
 *                        fc (512 + z_dim) -> 800, reparam.* [noise_dim, 800]}: three conv trunks on the same 2x - 1, each with its own weights; the trunk
 *                        output comes FIRST in both concatenations; no log-variance clip.
 * input_dim 784, h_dim 800, n_layers 1, 1 <= noise_dim <= 128 (the width of z0), z_dim >= 1 (<= 128 for ardae_vae_aux_iwae_draw), flags 0, any activation
 * but NONE.  Workspace modes as for kinds 14 / 15 (0: encode_stats, which returns mu0, lv0; 1: forward + backward; 2: decode; 4: ardae_vae_aux_iwae_draw).
 * Every ardae_vae_* entry point takes it with kind 14's conventions (eps rows [eps0 | eps], the Philox elements of an own draw, losses[2] = mean(kld +
 * aux_kld)); the z head has kind 11's variants and policy; ardae_vae_aux_elbo_rows and ardae_vae_aux_iwae_draw take it unchanged.
 *
 * The decoder's last two stages on their own: u1 [R, 8, 8, 32] NHWC - decode.deconv1's activated output with its zero pad - -> decode.deconv2
 * (ConvTranspose2d 32 -> 16, k5 s2 p2, 8 x 8 -> 15 x 15) + bias + activation -> decode.reparam.logit_fn (16 -> 1, 15 x 15 -> 29 x 29, cropped) + bias
 * -> logits [R, 784].
 *   variant 1: conv_tail_kernel, ONE launch, a workgroup per image: u1 and the 15 x 15 x 16 map stay in LDS, the weights come from `packed` (re-laid by
 *              ardae_model_pack) by scalar loads; every output is one FP32 FMA chain in a fixed order (input channel ascending, within it the taps
 *              ascending; then bias and activation), so a row's bits do not depend on R.  Needs no workspace (it may be NULL).
 *   variant 2: the four launches the training forward runs (linear, col2im, linear, col2im); workspace: ardae_conv_tail_workspace_floats(d, R, 2) floats.
 *   variant 0: what ardae_model_decode runs for kind 17: variant 1, unless ARDAE_CONV_TAIL_UNFUSED=1 is set under ARDAE_DEBUG_KNOBS=1 (then the mode-2
 *              workspace of the kind grows by c2, u2, c3 and the logits: ~5.2e4 floats per decoded row in place of ~1.6e4).
 * Kinds 2 / 4 / 11 and kind 17's training forward run the unfused launches.
 * ardae_conv_tail_workspace_floats: the floats `variant` needs at R rows (0 for the fused kernel, and for bad arguments). */
size_t ardae_conv_tail_workspace_floats(const ardae_model_desc* d, int R, int variant);
int ardae_conv_tail(const ardae_model_desc* d, const float* params, const float* packed, const float* u1, int R, int variant, float* workspace,
                    size_t workspace_floats, float* logits, void* stream);

/* The last stage of the residual-conv decoder on its own (kinds 12 and 19: csrc/resvae.hip, csrc/auxresvae.hip; the kernels and this entry point: csrc/resmodel.hip): y14 [R, 14, 14, 16] NHWC - the output of decode.dec.14 after its ELU -
 * -> bilinear x2 upsampling (align_corners) -> decode.dec.17 = ResConv2d(16 -> 1) -> logits [R, 784].  It reads the effective weights ardae_model_pack
 * composed into `packed`.
 *   variant 1: resconv_tail_kernel, ONE launch, a workgroup per image: the interpolation, hmid = ELU(conv3x3_0h(u28) + b) and
 *              logit = conv3x3_h1(hmid) + conv3x3_01(u28) + (b_h1 + b_01) stay on chip; every sum runs in a fixed order inside the image's workgroup, so a
 *              row's bits do not depend on R.  Needs no workspace (it may be NULL).
 *   variant 2: the launches the training forward runs (upsample, im2col, linear, im2col, two-source linear); workspace:
 *              ardae_resconv_tail_workspace_floats(d, R, 2) floats.
 *   variant 0: what ardae_model_decode runs for kind 12: variant 1, unless ARDAE_RESCONV_TAIL_UNFUSED=1 is set under ARDAE_DEBUG_KNOBS=1 (then the mode-2
 *              workspace of the kind grows by the last stage's buffers).
 * ardae_resconv_tail_workspace_floats: the floats `variant` needs at R rows (0 for the fused kernel, and for bad arguments). */
size_t ardae_resconv_tail_workspace_floats(const ardae_model_desc* d, int R, int variant);
int ardae_resconv_tail(const ardae_model_desc* d, const float* params, const float* packed, const float* y14, int R, int variant, float* workspace,
                       size_t workspace_floats, float* logits, void* stream);

/* ---- the hierarchical resconv baseline of vae.py (models/vae/auxresconv.py; csrc/auxresvae.hip): ardae_model_desc.kind 19 ------
 * The Gaussian counterpart of kind 6, `vae.py --model auxresconv` / `auxresconvct` (do_center False / True).  18 is not a kind.
 *   kind 19 (MNISTResConvAuxVAE; 28 x 28 x 1 and ELU only): ONE weight-normalised residual trunk inp_encode.enc.* (the trunk of kinds 5 / 6 / 12, on 2x - 1
 *                        unless ARDAE_MODEL_NO_CENTER) -> ctx [B, c_dim]; aux_encode.reparam.{mean_fn, logvar_fn} [noise_dim, c_dim] on ctx;
 *                        encode.fc.0 (c_dim + noise_dim) -> c_dim + ELU on cat[ctx, z0], encode.reparam.* [z_dim, c_dim]; kind 12's decoder;
 *                        aux_decode.fc.0 (c_dim + z_dim) -> c_dim + ELU on cat[ctx, z], aux_decode.reparam.* [noise_dim, c_dim].  ctx comes FIRST in
 *                        both concatenations; no log-variance clip.
 * input_dim 784, h_dim = c_dim >= 1, n_layers 1, 1 <= noise_dim <= 128 (the width of z0), z_dim >= 1 (<= 128 for ardae_vae_aux_iwae_draw), flags 0 or
 * ARDAE_MODEL_NO_CENTER, ARDAE_ACT_ELU.  Workspace modes as for kind 17 (0: encode_stats, which returns mu0, lv0; 1: forward + backward; 2: decode;
 * 4: ardae_vae_aux_iwae_draw).  Every ardae_vae_* entry point takes it with kind 14's conventions (eps rows [eps0 | eps], the Philox elements of an own
 * draw, losses[2] = mean(kld + aux_kld)); the z head has kind 12's variants and policy (ardae_vae_head_fused_ok is 0); ardae_vae_aux_elbo_rows and
 * ardae_vae_aux_iwae_draw take it unchanged; ardae_resconv_tail takes it as it takes kind 12.
 *
 * The decoder's 14 x 14 stage on its own: y8 [R, 8, 8, 32] NHWC - the output of decode.dec.8 after its ELU - -> crop to 7 x 7 -> bilinear x2 upsampling
 * (align_corners) -> decode.dec.12 = ResConv2d(32 -> 16) + ELU -> decode.dec.14 = ResConv2d(16 -> 16) + ELU -> y14 [R, 14, 14, 16] NHWC, which
 * ardae_resconv_tail reads.  It reads the effective weights and the re-laid copy ardae_model_pack left in `packed`.
 *   variant 1: resconv_mid_kernel, ONE launch, a workgroup per image: the interpolated map, both hidden maps and dec.12's output stay in LDS, the six
 *              3 x 3 convolutions run on v_mfma_f32_16x16x4_f32 in a fixed order inside the image's workgroup, so a row's bits do not depend on R.
 *              Needs no workspace (it may be NULL).
 *   variant 2: the ten launches the training forward runs (crop, upsample, and per block im2col, linear, im2col, two-source linear); workspace:
 *              ardae_resconv_mid_workspace_floats(d, R, 2) floats.
 *   variant 0: what ardae_model_decode runs for kind 19: variant 1, unless ARDAE_RESCONV_MID_UNFUSED=1 is set under ARDAE_DEBUG_KNOBS=1 (then the mode-2
 *              workspace of the kind grows by c7, u14 and the two blocks' buffers, and its columns scratch to the 14 x 14 blocks').
 * Kinds 5 / 6 / 12 and kind 19's training forward run the unfused launches.
 * ardae_resconv_mid_workspace_floats: the floats `variant` needs at R rows (0 for the fused kernel, and for bad arguments). */
size_t ardae_resconv_mid_workspace_floats(const ardae_model_desc* d, int R, int variant);
int ardae_resconv_mid(const ardae_model_desc* d, const float* params, const float* packed, const float* y8, int R, int variant, float* workspace,
                      size_t workspace_floats, float* y14, void* stream);

/* ---- evaluation / visualisation side of the model surface (csrc/eval_kernels.hip) ----------------------------
 * Decoder samples that ImplicitPosteriorVAE.forward / .generate return next to the losses (ivae/mnist.py:188-199,300,316):
 * relaxed Bernoulli (models/reparam.py:111-158, BernoulliDistribution.sample_logistic_sigmoid):
 *   sample = sigmoid((logit + log(u/(1-u) + 1e-20)) / temperature), mean = sigmoid(logit); u ~ U[0,1) from the caller
 *   (ardae_philox_uniform); sample or mean may be NULL. */
int ardae_relaxed_bernoulli(const float* logit, const float* u, int64_t n, float temperature, float* sample, float* mean,
                            void* stream);
/* models/reparam.py:42-51 (sample_gaussian; Gaussian decoder of ivae/toy.py:725-737): sample = mu + exp(logvar/2) * eps */
int ardae_gaussian_sample(const float* mu, const float* logvar, const float* eps, int64_t n, float* sample, void* stream);
/* Lower Cholesky factors of `batch` symmetric n x n matrices (n <= 64), one launch: the factorisation inside
 * MultivariateNormal(mu, cov) of the IWAE proposal (ivae/mnist.py:397-406).  Not positive definite -> NaNs in that factor. */
int ardae_cholesky_batched(const float* A, int batch, int n, float* L, void* stream);

/* ---- IWAE evaluation (csrc/iwae.hip): the proposal of logprob_w_cov_gaussian_posterior (ivae/mnist.py:378-437) in one launch ---
 * Per image b (one workgroup each, z <= 64): mu = column mean of zs[b] [ke, z]; cov = centred zc^T zc / (ke - 1) + jitter I
 * (utils/stat.py:127-158; the aux models pass jitter 1e-5, ivae/auxmnist.py:321, the others 0); L = the lower Cholesky factor of cov (the
 * factorisation of ardae_cholesky_batched); for each of the k proposal samples newz[b, j] = mu + L e_j and
 * logq[b, j] = -0.5 sum e_j^2 - sum_i log L_ii - 0.5 z log 2 pi.  e = prop_noise [B, k, z], or, when prop_noise is NULL, drawn in the
 * kernel: element first_element + (b k + j) z + i of the draw (seed, offset), the numbers ardae_philox_normal_at(out, B k z, seed,
 * offset, NULL, first_element) would write (first_element a multiple of 4; a caller that walks a set in chunks passes the chunk's first
 * image times k z and gets draws that do not depend on the chunking).  eps_out [B, k, z] (the e used), mu [B, z], chol [B, z, z] may be
 * NULL.  A covariance that is not positive definite gives NaN in that image's newz and logq (and in chol, as ardae_cholesky_batched
 * does), and touches no other image.  An image's outputs do not depend on B or on its place in the launch. */
int ardae_iwae_proposal(const float* zs, const float* prop_noise, int B, int ke, int k, int z, float jitter, uint64_t seed, uint64_t offset,
                        uint64_t first_element, float* newz, float* logq, float* eps_out, float* mu, float* chol, void* stream);
/* out[b] = log(mean_j exp(lw_j - max_j lw) + 1e-10) + max_j lw with lw_j = -recon[b, j] - prior[b, j] - logq[b, j]
 * (ivae/mnist.py:427-436); recon / prior / logq [B, k] (ardae_model_loss_rows' rows), fixed reduction order, NaN rows give NaN. */
int ardae_iwae_reduce(const float* recon, const float* prior, const float* logq, int B, int k, float* out, void* stream);

/* ---- posterior diagnostics (csrc/diag.hip): the compute of the loop's `''' visualize '''` block (ivae_ardae.py:952-1111) ---------
 * ardae_philox_normal_scaled_at: the numbers of ardae_philox_normal_at (same keying, first_element a multiple of 4), element e multiplied
 * in fp32 by scale[((first_element + e) / width) % nslots] - a [rows, nslots, width] draw whose slot s carries the noise level scale[s], so
 * that ONE sampler call with nz = nslots does model.encode(x, std=s) for every s (ivae_ardae.py:992-999,1001).  Bit-equal to the plain draw
 * followed by `noise * float(std)`; a slot whose scale is exactly 0 is +0.0f.  scale: device, [nslots]. */
int ardae_philox_normal_scaled_at(float* out, int64_t n, uint64_t seed, uint64_t offset, const void* state, uint64_t first_element, int width,
                                  int nslots, const float* scale, void* stream);
/* logvar[b, c] = log(var_r z[b, r, c] + eps), the unbiased variance over an image's nz sampler rows: torch.log(torch.var(latent, dim=1)
 * + 1e-10) of ivae_ardae.py:956-957.  z [B, nz, zd].  Mean first, then the centred squares, in fp64 and in an order that depends on
 * (nz, zd) only: no atomics, and an image's output does not depend on B or on its place in the launch.  nz == 1 gives NaN, as torch does. */
int ardae_sample_logvar(const float* z, int B, int nz, int zd, float eps, float* logvar, void* stream);
/* counts[s] += np.histogram2d(x_s, y_s, range=[[lo, hi], [lo, hi]], bins=bins)[0] for the nslots point sets
 * (x_s, y_s)[i] = (pts[i row_stride + s slot_stride + col_x], pts[i row_stride + s slot_stride + col_y]), i < n
 * (get_2d_histogram_plot, utils/visualization.py:193-204).  counts [nslots, bins, bins], first index x; it is ADDED to: zero it once per
 * set.  Edges are np.linspace's doubles (k (hi - lo) / bins + lo, product and sum rounded apart; hi for k = bins), a float32 value v
 * belongs to bin k when edge[k] <= v < edge[k + 1] compared in double, v == hi to the last bin; values outside, +-inf and NaN are dropped.
 * bins <= 128 (one 32-bit table per workgroup in LDS, flushed with 64-bit atomic adds; integer sums: the result does not depend on their
 * order). */
int ardae_hist2d(const float* pts, int64_t n, int64_t row_stride, int nslots, int64_t slot_stride, int col_x, int col_y, double lo, double hi,
                 int bins, int64_t* counts, void* stream);
/* ardae_hist2d for tables wider than one workgroup's LDS: the 256-bin heat maps of the scripts' `''' test visualize '''` blocks
 * (ivae_ardae.py:1224-1290, vae.py:677-720).  Same arguments, same contract in every respect above (np.linspace's edges, the comparison in double,
 * v == hi in the last bin, outside / +-inf / NaN dropped, counts [nslots, bins, bins] ADDED to, first index x, integer sums), with 1 <= bins <= 512.
 * The table is cut into bands of 16384 / bins x-bin rows (64 KiB of 32-bit counters: 2 bands at 129 bins, 4 at 256, 16 at 512); a workgroup owns one
 * (share of the points, slot, band), looks up the y bin of the points whose x bin falls into its band and flushes its non-zero cells with 64-bit
 * atomic adds - every point is counted by exactly one band, and the points are read once per band.  For bins <= 128 it is ardae_hist2d's result at
 * ardae_hist2d's cost (one band); callers with such tables call ardae_hist2d. */
int ardae_hist2d_wide(const float* pts, int64_t n, int64_t row_stride, int nslots, int64_t slot_stride, int col_x, int col_y, double lo, double hi,
                      int bins, int64_t* counts, void* stream);


/* ---- scalar log channel + static-binarised batches ------------------------------------------------
 * The scalars the reference logs per --log-interval (ivae_ardae.py:850-906; five .item() synchronisations per step there,
 * :756-758,774,837-841) leave the step through a device ring buffer instead: one record per step, written by ONE kernel at
 * the end of the step (graph-replayable: the slot comes from the device step state, iter = Adam's t), read in bulk by the host.
 * Record (ARDAE_LOG_RECORD_FLOATS floats): [0] iter (low 31 bits, int bit pattern), [1] model loss, [2] recon, [3] prior,
 * [4] beta, [5] cDAE loss, [6..8] mean / max / min over the B images of std (ivae_ardae.py:756-758), [9] cDAE lr,
 * [10] iter >> 31.  ring: [capacity, ARDAE_LOG_RECORD_FLOATS]. */
#define ARDAE_LOG_RECORD_FLOATS 16
int ardae_log_scalars(const float* cdae_loss, const float* model_losses, const float* std_b, int B, float beta, float d_lr,
                      const void* state, float* ring, int capacity, void* stream);
/* record [4] = beta_state's beta (a train state; `state` stays the block whose t numbers the record - the engine passes one block twice) */
int ardae_log_scalars_dev(const float* cdae_loss, const float* model_losses, const float* std_b, int B, const void* beta_state, float d_lr,
                          const void* state, float* ring, int capacity, void* stream);
/* out[b, :] = table[idx[b], :]: a batch of a statically binarised set (fixed pre-drawn rows, datasets/sbmnist.py:34-60) by
 * int64 row indices, all on the device */
int ardae_gather_rows(const float* table, const int64_t* idx, int B, int D, float* out, void* stream);


/* ---- data-parallel gradient exchange: RCCL over xGMI (SURVEY 8(b) `dp_allreduce_flat`, 8(e); kernel inventory K11) -----------
 * The reference has no collectives (single process, single device: SURVEY 2.1).  Under data parallelism each rank holds
 * a shard of the image batch and the reference's batch-mean losses (`cdae_loss.backward()` ivae_ardae.py:771,
 * `model_loss.backward()` :804, the entropy seed :826-834) become a mean over ranks of the two flat gradient buffers.
 * One communicator per rank, created once; one in-place all-reduce per buffer, issued on `stream` like any kernel
 * of this library - it may be CAPTURED into the step's HIP graph.
 * RCCL is bound at run time (dlopen; a copy already resident in the process - PyTorch's - is reused): without a usable
 * librccl.so these entry points fail with a message and everything else works.  Status codes of this group:
 * 0 ok, <0 invalid argument, 1..999 a hipError_t, 1000 + n an ncclResult_t n.                                         */
#define ARDAE_DP_UNIQUE_ID_BYTES 128
/* "RCCL <version> (<path of the bound library>)", "" when none could be bound */
const char* ardae_dp_backend(void);
/* rank 0: a fresh id (ncclGetUniqueId) into HOST memory; the caller ships the 128 bytes to every rank
 * (torch.distributed broadcast, MPI, a file ...) */
int ardae_dp_unique_id(void* host_id);
/* every rank, with its GPU selected (hipSetDevice / torch.cuda.set_device): joins the communicator; blocks until all
 * `nranks` processes have called it.  One rank per device (RCCL refuses two ranks on one GPU). */
int ardae_dp_comm_create(const void* host_id, int nranks, int rank, void** comm_out);
/* what RCCL itself reports for the communicator (ncclCommCount / ncclCommUserRank) + the device it was created on */
int ardae_dp_comm_query(void* comm, int* nranks, int* rank, int* device);
int ardae_dp_comm_destroy(void* comm);
/* buf[0..n) <- mean over ranks of buf[0..n), in place, stream-ordered (ncclAllReduce, ncclAvg).  One rank: unchanged. */
int ardae_dp_allreduce_mean(void* comm, float* buf, size_t n, void* stream);


/* ---- live per-kernel timing (bench.py roofline): HIP events around every launch on the launch stream ---------- */
typedef struct ardae_profile_entry {
  char name[96];   /* kernel name as rocprofv3 prints it (template arguments included); a suffix may follow them:
                      the per-image kernels append the block that ran, " b16" (16 x 16) or " fast" (lean 32 x 32)   */
  int calls;
  double total_ms; /* sum of event-to-event durations                                                         */
  double flops;    /* algorithmic FLOPs (2*MAC) of those launches                                             */
  double bytes;    /* algorithmic HBM bytes of those launches (operands read once + results written once)     */
} ardae_profile_entry;
int ardae_profile_enable(int on);
/* Diagnostics: a one-thread kernel that writes the device's constant 100 MHz clock (s_memrealtime) to slots[slot] when the stream
 * reaches it - an unprofiled timeline of a step (also inside captured graphs; tools / scratch use it, the product does not). */
int ardae_debug_stamp(unsigned long long* slots, int slot, void* stream);
/* synchronises, aggregates by kernel, clears the log; returns the number of distinct kernels */
int ardae_profile_report(ardae_profile_entry* entries, int max_entries);

#ifdef __cplusplus
}
#endif
#endif /* ARDAE_HIP_H */
