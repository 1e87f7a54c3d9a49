// The conv Gaussian-posterior baseline (ardae_model_desc.kind 11: models/vae/conv.py::VAE, `vae.py --model conv`); csrc/model.hip dispatches the
// sizing / pack / decode queries to the family, the ardae_vae_* entry points of csrc/vaemodel.hip dispatch here on the kind.
#pragma once
#include "host_util.h"

namespace ardae {
extern const Family CONVVAE_FAMILY;
// the descriptor rules of kind 11 (input_dim 784, h_dim 800, n_layers 1, noise_dim 0, flags 0, z_dim >= 1, any activation but NONE)
int convvae_desc_check(const ardae_model_desc* d);
// whether this family's fused head (the two MFMA products + ONE tail launch) is the default: z_dim <= 64
bool convvae_head_fused_ok(const ardae_model_desc& d);
// the bodies of ardae_vae_forward / _backward / _encode_stats / _head for kind 11; arguments are validated by the caller
int convvae_forward(const ardae_model_desc& d, const float* params, const float* packed, const float* x, const float* eps, int B, DevFloat beta,
                    uint64_t seed, uint64_t offset, const void* state, float* workspace, size_t wsf, float* z_out, float* eps_out, float* losses,
                    hipStream_t st);
int convvae_backward(const ardae_model_desc& d, const float* params, const float* packed, const float* x, int B, DevFloat beta, float loss_scale,
                     float* workspace, size_t wsf, float* grads, float grads_beta, hipStream_t st);
int convvae_encode_stats(const ardae_model_desc& d, const float* params, const float* packed, const float* x, int B, float* workspace, size_t wsf,
                         float* mu_out, float* lv_out, hipStream_t st);
int convvae_head(const ardae_model_desc& d, const float* params, const float* packed, const float* hid, const float* eps, int B, uint64_t seed,
                 uint64_t offset, const void* state, int variant, float* mu, float* lv, float* z, float* eps_out, float* kld, hipStream_t st);
}  // namespace ardae
