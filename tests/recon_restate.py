"""The reconstruction DAEs (models/dae/mlp.py: DAE :21-82, ConditionalDAE :85-193) restated for tests/test_recon_dae.py and its GPU sibling: the
float64 / float32 oracle of both classes, and how their fixtures are read.  Not a test module: nothing here is collected.

The restatement takes {name: tensor} parameters and computes in the dtype its arguments come in (autograd gives the gradients)."""
import glob
import os

import torch

from score_restate import ACTS, dims, load, mlp, state_dict_of, std_of      # noqa: F401

UNCOND = ("n64_d2_softplus", "n60_d3_elu", "n64_d2_swish", "n64_d2_relu1", "n96_d8_tanh")
COND = ("b4_s16_d2", "b5_s12_d3", "b4_s16_d2_swish", "b8_s8_d2_relu1", "b6_s16_d8_tanh", "b3_s20_d3_tanh1")
COND_IDS = [f"{e}_{c}" for c in COND for e in ("x", "a")]           # x: enc_input=False (kind 13), a: enc_input=True (kind 11)


def fixture_paths(golden_dir):
    u = sorted(p for p in glob.glob(os.path.join(golden_dir, "recon_dae_n*.npz")))
    c = sorted(glob.glob(os.path.join(golden_dir, "recon_cdae_[xa]_b*.npz")))
    assert len(u) == len(UNCOND) and len(c) == len(COND_IDS)
    return u, c


def add_noise(noise, x, std, draw):
    """dae/mlp.py:12-18 in the reference's operation order; draw: normals, or uniforms in [0, 1)"""
    if noise == "gaussian":
        return x + std * draw
    assert noise == "uniform"
    return x + (2. * std * draw - std)


def network(p, act, x, ctx=None, enc_input=False):
    """x [N, d] (ctx [N, c]: one context row per sample row) -> the reconstruction [N, d]"""
    if ctx is None:
        return mlp(p, "main.", x, act)
    c = ACTS[act](mlp(p, "ctx_encode.", ctx, act))
    a = ACTS[act](mlp(p, "inp_encode.", x, act)) if enc_input else x
    return mlp(p, "dae.", torch.cat([a, c], 1), act)


def forward(p, act, noise, x, std, draw, ctx=None, enc_input=False):
    """-> x_bar, x_recon, loss, {name: grad}"""
    p = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    xbar = add_noise(noise, x, std, draw)
    recon = network(p, act, xbar, ctx, enc_input)
    loss = torch.nn.functional.mse_loss(recon, x)
    return xbar, recon.detach(), loss.detach(), dict(zip(p, torch.autograd.grad(loss, list(p.values()))))


def glogprob(p, act, x, std, ctx=None, enc_input=False):
    return (network(p, act, x, ctx, enc_input) - x) / std ** 2


def case(fx, dtype=torch.float32):
    """A fixture's (conditional, act, noise, enc_input, (B, S), (d, c, h, L), p, x [N, d], ctx [N, c] | None, std, draw [N, d]) in `dtype`"""
    act, noise = str(fx["act"]), str(fx["noise"])
    p = {k: v.to(dtype) for k, v in state_dict_of(fx).items()}
    draw = torch.tensor(fx["draw"]).to(dtype)
    if "ctx" in fx:
        B, S, d, c, h, nl = dims(fx)
        x, ctx = torch.tensor(fx["x"]).to(dtype).view(B * S, d), torch.tensor(fx["ctx"]).to(dtype).view(B * S, c)
        return True, act, noise, bool(int(fx["enc_input"])), (B, S), (d, c, h, nl), p, x, ctx, std_of(fx, dtype), draw
    N, d, h, nl = (int(v) for v in fx["shape"])
    return False, act, noise, False, (N, 1), (d, 0, h, nl), p, torch.tensor(fx["x"]).to(dtype), None, std_of(fx, dtype), draw


def glog_tol(fx, tensor_tol):
    """glogprob's bar: the division by std^2 amplifies the cancellation in recon - x, so the fixture's own fp32-to-float64 distance counts"""
    a, b = torch.tensor(fx["glog"]).double(), torch.tensor(fx["glog_f64"])
    return max(tensor_tol, 3 * float((a - b).norm() / b.norm()))
