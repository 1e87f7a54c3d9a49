// The auxiliary-variable Gaussian baselines of vae.py (ardae_model_desc.kind 14: MNISTAuxVAE `--model auxmnist`, 15: ToyAuxVAE `--model auxtoy`);
// csrc/model.hip dispatches to the family, the ardae_vae_* entry points of csrc/vaemodel.hip through its GaussFamily row.
#pragma once
#include "host_util.h"

namespace ardae {
extern const Family AUXVAE_FAMILY;   // kinds 14 / 15
}  // namespace ardae
