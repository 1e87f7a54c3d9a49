// Weight-normalised residual-conv models (ardae_model_desc.kind 5: ResConvIPVAE `--model resconvct-res`, 6: MNISTResConvAuxIPVAE
// `--model auxresconvct`); csrc/model.hip dispatches to the family.  Noise: kind 5 [rows, noise_dim]; kind 6 [rows, noise_dim + z_dim]
// (rows [eps0 | eps], noise_dim = z0_dim); the hidden1a context of kind 6 is h [B, c_dim = h_dim] (ivae/auxresconv.py:125-132).
#pragma once
#include "host_util.h"

namespace ardae {
extern const Family RES_FAMILY;
}  // namespace ardae
