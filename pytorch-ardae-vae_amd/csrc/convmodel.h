// The conv models (ardae_model_desc.kind 2: ConvIPVAE `--model mnist-conv`; 4: MNISTConvAuxIPVAE `--model auxconv`, noise
// [R, noise_dim + z_dim], hidden context [B, 1600]); csrc/model.hip dispatches to the families.
#pragma once
#include "host_util.h"

namespace ardae {
extern const Family CONV_FAMILY, AUXCONV_FAMILY;
}  // namespace ardae
