// The hierarchical conv Gaussian baseline of vae.py (ardae_model_desc.kind 17: MNISTConvAuxVAE `--model auxconv`); csrc/model.hip dispatches to the
// family, the ardae_vae_* entry points through its GaussFamily row.  ardae_conv_tail (the decoder's last two stages alone) lives beside it.
#pragma once
#include "host_util.h"

namespace ardae {
extern const Family AUXCONVVAE_FAMILY;   // kind 17
}  // namespace ardae
