"""What the tests of the conditional AR-DAE without an input encoder (ardae_cdae_desc.kind 16 / 17; tests/test_cardae_noenc.py and its GPU sibling)
share: the `Family` record of the two kinds and ONE float64 / float32 restatement of their network, score and denoising loss.  Not a test module:
nothing here is collected.

The network (models/graddae/mlp.py:341-483, models/resdae/mlp.py:286-413 with enc_input=False): cat[x_bar, act(ctx_encode(ctx)) repeated S times, std]
into the last MLP; the grad kind's score is the input-gradient of -neglogprob, the res kind's the MLP's output."""
import dataclasses
import functools

import torch

import ardae_amd as net
from ardae_amd import layout
from score_restate import ACTS, Family, mlp

FIXTURE_CASES = ("b4_s16_d2_softplus", "b5_s12_d3_elu", "b6_s16_d8_tanh", "b8_s8_d2_relu1", "b4_s16_d2_swish")
FIXTURE_IDS = [f"{k}_{c}" for k in ("grad", "res") for c in FIXTURE_CASES]


@dataclasses.dataclass(frozen=True, eq=False)
class NoEncFamily(Family):
    def fixture(self, golden_dir, fid):
        """The fixture with its std [B, S, 1] as the [B*S, 1] column the shared bodies take (the same numbers, row by row)"""
        fx = super().fixture(golden_dir, fid)
        fx["std"] = fx["std"].reshape(-1, 1)
        return fx


NOENC = NoEncFamily("cardae_noenc", functools.partial(layout.cdae_spec, enc_input=False),
                    {"grad": functools.partial(net.MLPGradCARDAE, enc_input=False), "res": functools.partial(net.MLPResCARDAE, enc_input=False)},
                    {"grad": 16, "res": 17}, net.ScoreConfig, True, False)


def score(kind, p, act, x, std, ctx, S=1, create_graph=False):
    """x [N, d], std [N, 1], ctx [N / S, c] -> the score [N, d], in the dtype of its arguments"""
    x = x if (kind == "res" or x.requires_grad) else x.clone().requires_grad_(True)
    hdn = torch.cat([x, ACTS[act](mlp(p, "ctx_encode.", ctx, act)).repeat_interleave(S, 0), std], 1)
    if kind == "res":
        return mlp(p, "dae.", hdn, act)
    logprob = -mlp(p, "neglogprob.", hdn, act).sum()
    return torch.autograd.grad(logprob, x, create_graph=create_graph)[0]


def grads_on_xbar(kind, p, act, xbar, std, eps, ctx, S=1):
    """mse(std g(xbar), -eps) on a GIVEN xbar -> loss, {name: grad or None}, with p's tensors as leaves"""
    p = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    xbar = xbar.detach().clone().requires_grad_(True)
    loss = torch.nn.functional.mse_loss(std * score(kind, p, act, xbar, std, ctx, S, create_graph=True), -eps)
    return loss.detach(), dict(zip(p, torch.autograd.grad(loss, list(p.values()), allow_unused=True)))
