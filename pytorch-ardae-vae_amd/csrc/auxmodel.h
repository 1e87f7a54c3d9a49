// The hierarchical MLP models (ardae_model_desc.kind 3: MNISTAuxIPVAE `--model auxmnist`, 7: ToyAuxIPVAE `--model auxmlp`); csrc/model.hip
// dispatches to the family.  Noise [B*nz, noise_dim + z_dim] (rows [eps0 | eps]; kind 7: two blocks) or null = zeros; hidden context [B, 2 h] (nz == 1).
#pragma once
#include "host_util.h"

namespace ardae {
extern const Family AUX_FAMILY;
// the two reparameterisation steps shared with the hierarchical conv model (csrc/auxconvmodel.hip)
//   out[r][c] = mu[g][c] + exp(lv[g][c] / 2) * eps[r * ld_eps + c],  g = r / rows_per_group   (mu, lv: [rows / rpg, cols])
// min_std / raw (the clipped aux-resconv class, ivae/auxresconv2.py:29-36,91): out = mu + exp(lv / 2) eps + min_std (raw ? raw : eps) - `eps` carries
// std * draw, the extra term the UNSCALED draw (raw [rows, cols], row stride ld_raw; NULL: eps itself, i.e. std = 1)
int launch_reparam_fwd(const float* mu, const float* lv, const float* eps, int ld_eps, int64_t rows, int cols, int rows_per_group, float* out,
                       hipStream_t st, float min_std = 0.f, const float* raw = nullptr, int ld_raw = 0);
// dlv = dz (z - mu - min_std eps) / 2   (eps: the draw of the forward call, needed only with min_std != 0)
int launch_reparam_bwd(const float* dz, const float* z, const float* mu, int64_t rows, int cols, int rows_per_group, float* dlv, hipStream_t st,
                       float min_std = 0.f, const float* eps = nullptr, int ld_eps = 0);
// NormalDistribution.clip_logvar (models/reparam.py:17-41; code: ardae_hip.h's ARDAE_MODEL_CLIP_*, 0 = none: no launch) on n raw head outputs x:
// y = c(x), or (dy given) the backward y = dy c'(x); y may be dy.  Shared with the auxiliary-variable baselines (csrc/auxvae.hip).
int launch_logvar_clip(const float* x, const float* dy, float* y, int64_t n, int code, hipStream_t st);
}  // namespace ardae
