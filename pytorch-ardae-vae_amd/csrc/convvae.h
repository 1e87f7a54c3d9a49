// The conv Gaussian-posterior baseline (ardae_model_desc.kind 11: models/vae/conv.py::VAE, `vae.py --model conv`).  The family's row is all it
// exports: csrc/model.hip's table reaches the sizing / pack / decode queries through it, and the ardae_vae_* entry points (csrc/vaemodel.hip)
// its descriptor rules and bodies through the row's `gauss` member (csrc/vaemodel.h).
#pragma once
#include "host_util.h"

namespace ardae {
extern const Family CONVVAE_FAMILY;
}  // namespace ardae
