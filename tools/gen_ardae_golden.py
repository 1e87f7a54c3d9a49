"""Golden vectors of the UNCONDITIONAL AR-DAE score networks (ardae_cdae_desc.kind 2 / 3)  --  TEST INFRASTRUCTURE.

Runs only where the reference checkout is available (it never travels to the GPU box):

    python tools/gen_ardae_golden.py [--reference DIR] [--only cases|quality]

Like oracle/gen_golden.py it imports the reference's own classes (models.MLPGradARDAE = models/graddae/mlp.py::ARDAE,
models.MLPResARDAE = models/resdae/mlp.py::ARDAE) behind inert stubs for the plotting imports and stores THEIR outputs:

  tests/golden/ardae_uncond_<kind>_<case>.npz   per kind and shape (N, d, h, L, act):
      sd/<name>            the reference's state_dict (default nn.Linear init under a fixed seed)
      x, std, eps          inputs; eps is what the reference drew (seed, call forward, re-seed, redraw randn_like)
      loss, g/<name>       forward(x, std)[1] and every parameter's .grad after loss.backward()  ("g/<name>/none": .grad is None)
      glog0, glog          glogprob(x) (std = None: zeros) and glogprob(x, std)
      loss64, g64/.., glog0_64, glog_64      the same calls on the same inputs after .double()
      traj_<opt>/...       6 steps of the training cell of notebooks/ardae_toy.ipynb with torch.optim.RMSprop(lr 1e-3, momentum 0.5)
                           and torch.optim.SGD: per step x, std, eps, the loss, and every parameter after the step
  tests/golden/ardae_uncond_quality.npz         8 seeds per kind of that training cell on x ~ N(0, I_2) (B 256, nsigma 10, delta 1,
      h 64, 3 layers, softplus, torch.optim.Adam(lr 0.005), 600 steps): mean loss of the last 100 steps and the relative L2 error of
      glogprob(x_t, s) against the exact score -x_t / (1 + s^2) of the sigma-smoothed Gaussian on 4096 fixed points, s in {.25, .5, 1}

Fixtures hold tensors and names only.
"""
import argparse
import contextlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import gen_golden as G  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
# (N, d, h, L, act)
CASES = {"n64_d2_softplus": (64, 2, 64, 3, "softplus"), "n96_d8_tanh": (96, 8, 64, 3, "tanh"), "n60_d3_elu": (60, 3, 100, 2, "elu"),
         "n64_d2_relu1": (64, 2, 64, 1, "relu"), "n64_d2_swish": (64, 2, 64, 3, "swish")}
TRAJ_STEPS = 6
OPTIMS = {"rmsprop": lambda ps: torch.optim.RMSprop(ps, lr=1e-3, momentum=0.5), "sgd": lambda ps: torch.optim.SGD(ps, lr=1e-2)}
QUALITY = dict(B=256, nsigma=10, delta=1.0, h=64, L=3, act="softplus", lr=0.005, steps=600, tail=100, seeds=list(range(8)), points=4096,
               levels=(0.25, 0.5, 1.0))


@contextlib.contextmanager
def injected_draw(eps):
    """The next torch.randn_like returns `eps` (the fp64 evaluation must see the fp32 call's draw, not one of its own)."""
    orig = torch.randn_like
    torch.randn_like = lambda t, *a, **k: eps.to(t.dtype)
    try:
        yield
    finally:
        torch.randn_like = orig


def build(net, kind, d, h, L, act):
    ctor = net.MLPGradARDAE if kind == "grad" else net.MLPResARDAE
    return ctor(input_dim=d, h_dim=h, num_hidden_layers=L, nonlinearity=act)


def forward_with_draw(dae, x, std, seed):
    """(loss, eps): the reference's own draw, recovered by replaying the seed."""
    torch.manual_seed(seed)
    _, loss = dae(x.clone(), std)
    torch.manual_seed(seed)
    eps = torch.randn_like(x)
    with injected_draw(eps):
        _, again = dae(x.clone(), std)
    assert torch.equal(loss.detach(), again.detach()), "the replayed draw is not the one the reference used"
    return loss, eps


def evaluate(dae, x, std, eps, tag, fx):
    with injected_draw(eps):
        _, loss = dae(x.clone(), std)
    dae.zero_grad()
    for p in dae.parameters():
        p.grad = None
    loss.backward()
    fx["loss" + tag] = loss.detach().numpy()
    for n, p in dae.named_parameters():
        if p.grad is None:
            fx[f"g{tag}/{n}/none"] = np.zeros(0)
        else:
            fx[f"g{tag}/{n}"] = p.grad.detach().numpy().copy()
    fx["glog0" + ("_64" if tag else "")] = dae.glogprob(x.clone()).detach().numpy()
    fx["glog" + ("_64" if tag else "")] = dae.glogprob(x.clone(), std).detach().numpy()


def gen_case(net, kind, name, shape, seed):
    N, d, h, L, act = shape
    torch.manual_seed(seed)
    dae = build(net, kind, d, h, L, act)
    sd0 = {k: v.clone() for k, v in dae.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    x, std = torch.randn(N, d, generator=g), 0.5 * torch.randn(N, 1, generator=g)
    fx = {"shape": np.array([N, d, h, L]), "act": np.array(act), "kind": np.array(kind), "x": x.numpy(), "std": std.numpy()}
    for k, v in sd0.items():
        fx["sd/" + k] = v.numpy().copy()
    loss, eps = forward_with_draw(dae, x, std, seed + 2)
    fx["eps"] = eps.numpy()
    evaluate(dae, x, std, eps, "", fx)
    assert float(fx["loss"]) == float(loss.detach())
    dae64 = build(net, kind, d, h, L, act).double()
    dae64.load_state_dict({k: v.double() for k, v in sd0.items()})
    evaluate(dae64, x.double(), std.double(), eps.double(), "64", fx)
    # the training cell of notebooks/ardae_toy.ipynb, 6 steps per optimiser, from the same initial parameters
    for oname, make in OPTIMS.items():
        dae.load_state_dict(sd0)
        opt = make(dae.parameters())
        fx[f"traj_{oname}/lr"] = np.array(opt.param_groups[0]["lr"])
        for s in range(TRAJ_STEPS):
            xs, ss = torch.randn(N, d, generator=g), 0.5 * torch.randn(N, 1, generator=g)
            opt.zero_grad()
            loss, eps_s = forward_with_draw(dae, xs, ss, seed + 10 + s)
            loss.backward()
            opt.step()
            pre = f"traj_{oname}/{s}/"
            fx[pre + "x"], fx[pre + "std"], fx[pre + "eps"], fx[pre + "loss"] = xs.numpy(), ss.numpy(), eps_s.numpy(), loss.detach().numpy()
            for k, v in dae.state_dict().items():
                fx[pre + "p/" + k] = v.numpy().copy()
    path = os.path.join(GOLDEN, f"ardae_uncond_{kind}_{name}.npz")
    np.savez_compressed(path, **fx)
    print(f"{path}: {os.path.getsize(path)} bytes, loss {float(fx['loss']):.6f} (fp64 {float(fx['loss64']):.6f})")


def gen_quality(net):
    q = QUALITY
    B, ns, d = q["B"], q["nsigma"], 2
    xt = torch.randn(q["points"], d, generator=torch.Generator().manual_seed(12345))
    fx = {k: np.array(v) for k, v in q.items()}
    fx["x_t"] = xt.numpy()
    for kind in ("grad", "res"):
        losses, errs = [], []
        for seed in q["seeds"]:
            torch.manual_seed(1000 + seed)
            dae = build(net, kind, d, q["h"], q["L"], q["act"])
            opt = torch.optim.Adam(dae.parameters(), lr=q["lr"])
            hist = []
            for _ in range(q["steps"]):
                opt.zero_grad()
                x = torch.randn(B, d)
                sigma = q["delta"] * torch.randn(B * ns, 1)
                x = x.unsqueeze(1).expand(B, ns, d).contiguous().view(B * ns, d)
                _, loss = dae(x, sigma)
                loss.backward()
                opt.step()
                hist.append(float(loss))
            losses.append(float(np.mean(hist[-q["tail"]:])))
            row = []
            for s in q["levels"]:
                sc = dae.glogprob(xt.clone(), torch.full((q["points"], 1), s)).detach()
                exact = -xt / (1.0 + s * s)
                row.append(float((sc - exact).norm() / exact.norm()))
            errs.append(row)
            print(kind, seed, losses[-1], row, flush=True)
        fx[f"{kind}/loss"], fx[f"{kind}/score_err"] = np.array(losses), np.array(errs)
    path = os.path.join(GOLDEN, "ardae_uncond_quality.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=G.REF)
    ap.add_argument("--only", choices=["cases", "quality"])
    a = ap.parse_args()
    G.REF = a.reference
    net, _ = G.import_reference()
    torch.set_num_threads(8)
    if a.only != "quality":
        for ki, kind in enumerate(("grad", "res")):
            for ci, (name, shape) in enumerate(CASES.items()):
                gen_case(net, kind, name, shape, 100 * ki + 10 * ci + 7)
    if a.only != "cases":
        gen_quality(net)


if __name__ == "__main__":
    main()
