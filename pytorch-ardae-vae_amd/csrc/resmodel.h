// Weight-normalised residual-conv models (ardae_model_desc.kind 5: ResConvIPVAE `--model resconvct-res`, 6: MNISTResConvAuxIPVAE
// `--model auxresconvct`, 12: MNISTResConvVAE `vae.py --model resconv`); csrc/model.hip dispatches to the family.  Noise: kind 5 [rows, noise_dim]; kind 6 [rows, noise_dim + z_dim]
// (rows [eps0 | eps], noise_dim = z0_dim); the hidden1a context of kind 6 is h [B, c_dim = h_dim] (ivae/auxresconv.py:125-132).
#pragma once
#include "host_util.h"

namespace ardae {
extern const Family RES_FAMILY;

// Kind 12 (MNISTResConvVAE, `vae.py --model resconv`, models/vae/resconv.py): the same trunk and decoder with a plain Gaussian head.  csrc/model.hip
// dispatches the sizing / pack / decode queries to RESVAE_FAMILY, the ardae_vae_* entry points of csrc/vaemodel.hip dispatch here on the kind.
extern const Family RESVAE_FAMILY;
// the descriptor rules of kind 12 (input_dim 784, noise_dim 0, h_dim = c_dim >= 1, z_dim >= 1, n_layers 1, ELU, flags within ARDAE_MODEL_NO_CENTER)
int resvae_desc_check(const ardae_model_desc* d);
// whether gauss_head_kernel is this family's default head (it is not: see csrc/resmodel.hip)
bool resvae_head_fused_ok(const ardae_model_desc& d);
// the bodies of ardae_vae_forward / _backward / _encode_stats / _head for kind 12; arguments are validated by the caller
int resvae_forward(const ardae_model_desc& d, const float* params, const float* packed, const float* x, const float* eps, int B, DevFloat beta,
                   uint64_t seed, uint64_t offset, const void* state, float* workspace, size_t wsf, float* z_out, float* eps_out, float* losses,
                   hipStream_t st);
int resvae_backward(const ardae_model_desc& d, const float* params, const float* packed, const float* x, int B, DevFloat beta, float loss_scale,
                    float* workspace, size_t wsf, float* grads, float grads_beta, hipStream_t st);
int resvae_encode_stats(const ardae_model_desc& d, const float* params, const float* packed, const float* x, int B, float* workspace, size_t wsf,
                        float* mu_out, float* lv_out, hipStream_t st);
int resvae_head(const ardae_model_desc& d, const float* params, const float* packed, const float* hid, const float* eps, int B, uint64_t seed,
                uint64_t offset, const void* state, int variant, float* mu, float* lv, float* z, float* eps_out, float* kld, hipStream_t st);
}  // namespace ardae
