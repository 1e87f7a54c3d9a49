"""The parameters of the Gaussian VAE fixtures (tests/golden/vae_*)  --  TEST INFRASTRUCTURE ONLY.

Those fixtures store a seed, not the parameters.  tools/gen_vae_golden.py loads what these recipes return into the reference's classes, and the
tests (tests/test_vae_*_baseline.py) regenerate the same numbers from the stored seed: both call the one definition here.  Each recipe is
oracle.ardae_oracle.init_params (platform-independent, numpy PCG64) on the family's layout spec, plus what the family's fixtures need on top.
"""
import torch

from ardae_amd import layout
from oracle import ardae_oracle as O


def conv(z, seed, special, dtype=torch.float32):
    """layout.conv_vae_spec(z); special restates `do_xavier=True, do_m5bias=True`: xavier-uniform Conv2d / Linear weights, their biases zero,
    ConvTranspose2d untouched, decode.reparam.logit_fn.bias = -5"""
    spec = layout.conv_vae_spec(z)
    sp = None
    if special:
        sp = {n: (("xavier",) if n.endswith("weight") else ("zeros",)) for n, _ in spec if "deconv" not in n and "logit_fn" not in n}
    p = O.init_params(spec, seed, sp, dtype)
    if special:
        p["decode.reparam.logit_fn.bias"].fill_(-5.0)
    return p


def resconv(z, c_dim, seed, special, dtype=torch.float32):
    """layout.resconv_vae_spec(z, c_dim), the weight-norm scales spread over [0.7, 1.3] so that gradients tell them apart; special restates
    `do_m5bias=True` as a setting: the last skip bias = -3 (the reference draws it from N(-3, 1e-4))"""
    p = O.init_params(layout.resconv_vae_spec(z, c_dim), seed, None, dtype)
    if special:
        p["decode.dec.17.conv_01.bias"].fill_(-3.0)
    return p


def aux(family, D, nd, h, z, L, seed, dtype=torch.float32):
    """layout.aux_vae_spec, then aux_encode's log-variance bias spread over [-5, 2.5] so that a clip acts on part of the elements ('hard' clamps
    outside [-4, 2], the softplus clips bend)"""
    p = O.init_params(layout.aux_vae_spec(family, D, nd, h, z, L), seed, None, dtype)
    p["aux_encode.reparam.logvar_fn.bias"].add_(torch.linspace(-5.0, 2.5, nd, dtype=dtype))
    return p


def auxconv(nd, z, seed, dtype=torch.float32):
    return O.init_params(layout.aux_conv_vae_spec(nd, z), seed, None, dtype)


def auxresconv(nd, z, c_dim, seed, dtype=torch.float32):
    return O.init_params(layout.aux_resconv_vae_spec(nd, z, c_dim), seed, None, dtype)
