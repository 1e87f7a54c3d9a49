// The Gaussian-posterior VAE baselines of vae.py (ardae_model_desc.kind 8: MNISTVAE `vae.py --model mnist`, 9: ToyVAE `--model toy`);
// csrc/model.hip dispatches the sizing / pack / decode queries to the family, the ardae_vae_* entry points live in csrc/vaemodel.hip.
#pragma once
#include "host_util.h"

namespace ardae {
extern const Family VAE_FAMILY;
// the descriptor rules of kinds 8 / 9 (noise_dim 0, flags 0, 1 .. 4 layers, any activation but NONE); 0 or -1 with the message set
int vae_desc_check(const ardae_model_desc* d);
}  // namespace ardae
