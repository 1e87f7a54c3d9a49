"""What the CPU tests of the score-network families outside the VAE loop (tests/test_ardae_uncond.py, test_dae_plain.py, test_cond_score.py) and
their GPU siblings share, written once: the `Family` records that say what differs, fixtures, the two tolerances, and ONE float64 / float32
restatement of the score and of the denoising loss for conditional x with-sigma-column.  Not a test module: nothing here is collected.

The restatement takes {name: tensor} parameters and computes in the dtype its arguments come in (autograd gives the gradients)."""
import dataclasses
import glob
import os
from typing import Callable

import numpy as np
import torch

import ardae_amd as net
from ardae_amd import layout

LOSS_TOL, TENSOR_TOL = 2e-5, 1e-4      # loss relative; every gradient tensor and glogprob relative L2 (the bars tests/test_cdae_gpu.py states)
ACTS = {"relu": torch.relu, "softplus": torch.nn.functional.softplus, "elu": torch.nn.functional.elu, "tanh": torch.tanh,
        "leaky_relu": lambda t: torch.nn.functional.leaky_relu(t, 0.2), "swish": lambda t: t * torch.sigmoid(t)}


@dataclasses.dataclass(frozen=True, eq=False)
class Family:
    """One score-network family: the AR-DAE networks read the noise level (a sigma column in the last MLP's first layer), the plain ones do not;
    the conditional ones encode a context row per image, shared by its S samples."""
    prefix: str                # of the fixture files under tests/golden/ (None: the family's fixtures belong to tests/test_cdae_gpu.py)
    spec: Callable             # layout's spec function: (kind, d, h, L), conditional: (kind, d, c, h, L)
    classes: dict              # {"grad" | "res": the module class}
    kind_id: dict              # {"grad" | "res": ardae_cdae_desc.kind}
    config: type               # net.ScoreConfig | net.DaeConfig: what the family's engine takes
    conditional: bool
    plain: bool

    key = property(lambda self: "cdae" if self.conditional else "dae")                       # of the engine's attribute and checkpoint entry
    engine = property(lambda self: net.ArdaeCondScoreEngine if self.conditional else net.ArdaeScoreEngine)
    last = property(lambda self: {"grad": "neglogprob.", "res": "dae." if self.conditional else "main."})   # the MLP that may read sigma

    def spec_of(self, kind, d, h, nl, c=0):
        return self.spec(kind, d, c, h, nl) if self.conditional else self.spec(kind, d, h, nl)

    def module(self, kind, d, h, nl, act, c=0, **kw):
        ctx = dict(context_dim=c) if self.conditional else {}
        return self.classes[kind](input_dim=d, h_dim=h, num_hidden_layers=nl, nonlinearity=act, **ctx, **kw)

    def fixtures(self, golden_dir, kind=None):
        names = sorted(glob.glob(os.path.join(golden_dir, f"{self.prefix}_{kind or '*'}_{'b' if self.conditional else 'n'}*.npz")))
        assert len(names) == (5 if kind else 10)
        return names

    def fixture(self, golden_dir, fid):
        return load(os.path.join(golden_dir, f"{self.prefix}_{fid}.npz"))


ARDAE = Family("ardae_uncond", layout.dae_spec, {"grad": net.MLPGradARDAE, "res": net.MLPResARDAE}, {"grad": 2, "res": 3}, net.ScoreConfig, False, False)
DAE = Family("dae_plain", layout.dae_plain_spec, {"grad": net.MLPGradDAE, "res": net.MLPResDAE}, {"grad": 6, "res": 7}, net.DaeConfig, False, True)
CARDAE = Family(None, layout.cdae_spec, {"grad": net.MLPGradCARDAE, "res": net.MLPResCARDAE}, {"grad": 0, "res": 1}, net.ScoreConfig, True, False)
CDAE = Family("cdae_plain", layout.cdae_plain_spec, {"grad": net.MLPGradCDAE, "res": net.MLPResCDAE}, {"grad": 10, "res": 11}, net.DaeConfig, True, True)
AR_SIBLING = {DAE: ARDAE, CDAE: CARDAE}      # the family with the sigma column on top: the same function where that column is zero


def load(path):
    return dict(np.load(path))


def state_dict_of(fx):
    return {k[3:]: torch.tensor(v) for k, v in fx.items() if k.startswith("sd/")}


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / (b.norm() + 1e-300))


def meta(fx):
    """An unconditional fixture's (kind, act, N, d, h, L)"""
    N, d, h, nl = (int(v) for v in fx["shape"])
    return str(fx["kind"]), str(fx["act"]), N, d, h, nl


def dims(fx):
    """A conditional fixture's (B, S, d, c, h, L)"""
    B, S, d, c, h, nl = (int(v) for v in fx["shape"])
    return B, S, d, c, h, nl


def std_of(fx, dtype=torch.float32):
    """The fixture's noise level as the reference took it: a Python float, or a [N, 1] tensor."""
    return float(fx["std"]) if fx["std"].ndim == 0 else torch.tensor(fx["std"]).to(dtype)


def inputs_of(fx, dtype):
    """A conditional fixture's (x [B*S, d], ctx [B, c], eps)"""
    B, S, d, c, _, _ = dims(fx)
    return torch.tensor(fx["x"]).to(dtype).view(B * S, d), torch.tensor(fx["ctx"]).to(dtype).view(B, c), torch.tensor(fx["eps"]).to(dtype)


# ---- the test-side oracle: the networks restated (models/layers.py:477-515 MLP; models/graddae/mlp.py:243-247,269-339 for the conditional ones:
# two MLPs with an activated output, an MLP on their concatenation; the context row of image b serves its S samples) ------------------------------
def mlp(p, prefix, hdn, act):
    n = len([k for k in p if k.startswith(prefix + "layers.") and k.endswith("weight")])
    for i in range(n):
        hdn = ACTS[act](hdn @ p[f"{prefix}layers.{i}.weight"].t() + p[f"{prefix}layers.{i}.bias"])
    return hdn @ p[prefix + "fc.weight"].t() + p[prefix + "fc.bias"]


def score(kind, p, act, x, std=None, ctx=None, S=1, create_graph=False):
    """x [N, d] -> the score [N, d].  std [N, 1]: the noise level the last MLP reads (the AR-DAE kinds; None: the plain ones).  ctx [N / S, c]: the
    conditional kinds."""
    x = x if (kind == "res" or x.requires_grad) else x.clone().requires_grad_(True)
    hdn = [x] if ctx is None else [ACTS[act](mlp(p, "inp_encode.", x, act)), ACTS[act](mlp(p, "ctx_encode.", ctx, act)).repeat_interleave(S, 0)]
    hdn = torch.cat(hdn + ([] if std is None else [std]), 1)
    if kind == "res":
        return mlp(p, "main." if ctx is None else "dae.", hdn, act)
    logprob = -mlp(p, "neglogprob.", hdn, act).sum()
    return torch.autograd.grad(logprob, x, create_graph=create_graph)[0]


def grads_on_xbar(kind, p, act, xbar, std, eps, column, ctx=None, S=1):
    """mse(std g(xbar), -eps) on a GIVEN xbar -> loss, {name: grad or None}, with p's tensors as leaves.  std: a number or a tensor that broadcasts
    against [N, d]; column: the network reads it too (the AR-DAE kinds)."""
    p = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    xbar = xbar.detach().clone().requires_grad_(True)
    loss = torch.nn.functional.mse_loss(std * score(kind, p, act, xbar, std if column else None, ctx, S, create_graph=True), -eps)
    return loss.detach(), dict(zip(p, torch.autograd.grad(loss, list(p.values()), allow_unused=True)))


def loss_and_grads(kind, p, act, x, std, eps, column, ctx=None, S=1):
    """The denoising loss on xbar = x + std eps, as grads_on_xbar"""
    return grads_on_xbar(kind, p, act, x + std * eps, std, eps, column, ctx, S)


def cast(dtype, p, *tensors):
    """(p, *tensors) in `dtype`; None stays None"""
    return ({k: v.to(dtype) for k, v in p.items()},) + tuple(None if t is None else t.to(dtype) for t in tensors)
