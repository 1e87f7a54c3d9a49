// The Gaussian-posterior VAE baselines of vae.py (ardae_model_desc.kind 8: MNISTVAE `vae.py --model mnist`, 9: ToyVAE `--model toy`);
// csrc/model.hip dispatches the sizing / pack / decode queries to the family, the ardae_vae_* entry points live in csrc/vaemodel.hip.
// The Gaussian head is declared here for the conv baseline (csrc/convvae.hip, kind 11), which runs it on its own hidden rows.
#pragma once
#include "host_util.h"

namespace ardae {
extern const Family VAE_FAMILY;
// the descriptor rules of kinds 8 / 9 (noise_dim 0, flags 0, 1 .. 4 layers, any activation but NONE); 0 or -1 with the message set
int vae_desc_check(const ardae_model_desc* d);

// encode.reparam.{mean_fn, logvar_fn} [zd, h] on hidden rows [B, h]: the Linears in the parameter buffer and their forward panels
struct GaussHead { int h, zd; Lin mean, logvar; size_t mean_f, logvar_f; };
// what gauss_head_kernel can compute at all (variant 1), and where it may be the default (rows of both matrices on 16 bytes)
bool gauss_head_fused_can(const GaussHead& H);
bool gauss_head_fused_ok(const GaussHead& H);
// mu, lv, z [B, zd], kld [B] (and eps_out: the draw used) from hid [B, h]; variant 0: fused where fused_default (unless ARDAE_VAE_HEAD_UNFUSED=1
// under ARDAE_DEBUG_KNOBS=1), 1: gauss_head_kernel, 2: the unfused launches.  eps null: element i of the draw (seed, offset [+ state.rng_offset])
int gauss_head_fwd(const GaussHead& H, bool fused_default, const float* params, const float* packed, const float* hid, const float* eps, int B,
                   uint64_t seed, uint64_t offset, const void* state, int variant, float* mu, float* lv, float* z, float* eps_out, float* kld,
                   hipStream_t st);
// the head's tail in one launch from mu, lv [B, zd] (zd <= 64): the draw or the injected eps, z, eps_out (may be null), kld [B] - bit for bit what
// ardae_philox_normal_at, the reparameterisation and the KL rows of the unfused head give on the same mu, lv
int gauss_head_tail(const float* mu, const float* lv, const float* eps, int B, int zd, uint64_t seed, uint64_t offset, const void* state, float* z,
                    float* eps_out, float* kld, hipStream_t st);
// the backward seed at the head on n = B zd elements: dmu = dz + c beta mu;  dlv = dz (z - mu) / 2 + c beta (exp(lv) - 1) / 2
int gauss_head_seed(const float* dz, const float* z, const float* mu, const float* lv, int64_t n, float c, DevFloat beta, float* dmu, float* dlv,
                    hipStream_t st);
// the Family members that refuse the implicit models' calls (there is no sampler)
int vae_no_encode(const ardae_model_desc&, const float*, const float*, const float*, const float*, int, int, float*, size_t, float*, float*, hipStream_t,
                  const float*);
int vae_no_forward(const ardae_model_desc&, const float*, const float*, const float*, const float*, int, int, DevFloat, float*, size_t, float*, float*,
                   hipStream_t);
int vae_no_backward(const ardae_model_desc&, const float*, const float*, const float*, const float*, int, int, DevFloat, float, const float*, float*,
                    size_t, float*, float, hipStream_t);
}  // namespace ardae
