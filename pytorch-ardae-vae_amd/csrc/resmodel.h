// Weight-normalised residual-conv models (ardae_model_desc.kind 5: ResConvIPVAE `--model resconvct-res`, 6: MNISTResConvAuxIPVAE
// `--model auxresconvct`, 12: MNISTResConvVAE `vae.py --model resconv`); csrc/model.hip dispatches to the family.  Noise: kind 5 [rows, noise_dim]; kind 6 [rows, noise_dim + z_dim]
// (rows [eps0 | eps], noise_dim = z0_dim); the hidden1a context of kind 6 is h [B, c_dim = h_dim] (ivae/auxresconv.py:125-132).
#pragma once
#include "host_util.h"

namespace ardae {
extern const Family RES_FAMILY;

// Kind 12 (MNISTResConvVAE, `vae.py --model resconv`, models/vae/resconv.py): the same trunk and decoder with a plain Gaussian head.  The row is all
// it exports: the ardae_vae_* entry points (csrc/vaemodel.hip) reach its descriptor rules and bodies through the row's `gauss` member (csrc/vaemodel.h).
extern const Family RESVAE_FAMILY;
// Kind 19 (MNISTResConvAuxVAE, `vae.py --model auxresconv` / `auxresconvct`, models/vae/auxresconv.py): the Gaussian counterpart of kind 6 - kind 12's
// trunk and decoder with the two-stage posterior and the auxiliary decoder of csrc/auxvae.h's families.
extern const Family AUXRESVAE_FAMILY;
}  // namespace ardae
