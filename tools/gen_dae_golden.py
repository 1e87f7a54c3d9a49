"""Golden vectors of the PLAIN DAE score networks (ardae_cdae_desc.kind 6 / 7)  --  TEST INFRASTRUCTURE.

Runs only where the reference checkout is available (it never travels to the GPU box):

    python tools/gen_dae_golden.py [--reference DIR] [--only cases|traj]

Like tools/gen_ardae_golden.py it imports the reference's own classes (models.MLPGradDAE = models/graddae/mlp.py::DAE,
models.MLPResDAE = models/resdae/mlp.py::DAE) through oracle.gen_golden.import_reference() and stores THEIR outputs:

  tests/golden/dae_plain_<kind>_<case>.npz      per kind and shape (N, d, h, L, act) - the shapes of the ardae_uncond_* set:
      kind, act, shape
      sd/<name>            the reference's state_dict (default nn.Linear init under a fixed seed)
      x, std, eps          inputs; std is a scalar in half of the cases and a [N, 1] tensor in the other half; eps is what the reference
                           drew (seed, call forward, re-seed, redraw randn_like)
      loss, g/<name>       forward(x, std)[1] and every parameter's .grad after loss.backward()  ("g/<name>/none": .grad is None)
      glog                 glogprob(x)
      loss_f64, g_f64/.., glog_f64      the same calls on the same inputs after .double()
  tests/golden/dae_plain_traj_<kind>.npz        6 steps of the training cell of notebooks/dae_toy.ipynb on injected eps: B 16 x num_sigma 4,
      d 2, h 64, 3 layers, softplus, torch.optim.Adam(lr 0.005), sigma from sigma_max 1.0 to sigma_min 0.1 with sigma_annealing = 4 (the ramp
      ends inside the run):  cfg/<name>, sd/<name>, and per step s:  <s>/x [B, d], <s>/eps, <s>/sigma (the Python float), <s>/loss,
      <s>/p/<name> after the step; the same loop in float64 on the same x / eps / sigma under <s>/loss_f64, <s>/p_f64/<name>

Fixtures hold tensors, names and settings only.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from oracle import gen_golden as G  # noqa: E402
from gen_ardae_golden import CASES, forward_with_draw, injected_draw  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SCALAR_STD = {"n64_d2_softplus": 0.5, "n60_d3_elu": 0.3, "n64_d2_swish": None, "n64_d2_relu1": None, "n96_d8_tanh": 1.25}     # None: a [N, 1] tensor
TRAJ = dict(B=16, nsigma=4, d=2, h=64, L=3, act="softplus", lr=0.005, sigma_max=1.0, sigma_min=0.1, sigma_annealing=4, steps=6)


def build(net, kind, d, h, L, act):
    ctor = net.MLPGradDAE if kind == "grad" else net.MLPResDAE
    return ctor(input_dim=d, h_dim=h, num_hidden_layers=L, nonlinearity=act)


def evaluate(dae, x, std, eps, tag, fx):
    with injected_draw(eps):
        _, loss = dae(x.clone(), std)
    for p in dae.parameters():
        p.grad = None
    loss.backward()
    fx["loss" + tag] = loss.detach().numpy()
    for n, p in dae.named_parameters():
        if p.grad is None:
            fx[f"g{tag}/{n}/none"] = np.zeros(0)
        else:
            fx[f"g{tag}/{n}"] = p.grad.detach().numpy().copy()
    fx["glog" + tag] = dae.glogprob(x.clone()).detach().numpy()


def gen_case(net, kind, name, shape, seed):
    N, d, h, L, act = shape
    torch.manual_seed(seed)
    dae = build(net, kind, d, h, L, act)
    sd0 = {k: v.clone() for k, v in dae.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    x, std_t = torch.randn(N, d, generator=g), 0.5 * torch.randn(N, 1, generator=g)
    std = std_t if SCALAR_STD[name] is None else SCALAR_STD[name]
    fx = {"shape": np.array([N, d, h, L]), "act": np.array(act), "kind": np.array(kind), "x": x.numpy(),
          "std": std.numpy() if torch.is_tensor(std) else np.array(std, dtype=np.float64)}
    for k, v in sd0.items():
        fx["sd/" + k] = v.numpy().copy()
    loss, eps = forward_with_draw(dae, x, std, seed + 2)
    fx["eps"] = eps.numpy()
    evaluate(dae, x, std, eps, "", fx)
    assert float(fx["loss"]) == float(loss.detach())
    dae64 = build(net, kind, d, h, L, act).double()
    dae64.load_state_dict({k: v.double() for k, v in sd0.items()})
    evaluate(dae64, x.double(), std.double() if torch.is_tensor(std) else std, eps.double(), "_f64", fx)
    path = os.path.join(GOLDEN, f"dae_plain_{kind}_{name}.npz")
    np.savez_compressed(path, **fx)
    print(f"{path}: {os.path.getsize(path)} bytes, loss {float(fx['loss']):.6f} (fp64 {float(fx['loss_f64']):.6f})")


def gen_traj(net, kind, seed):
    """The training cell of notebooks/dae_toy.ipynb (sigma schedule, broadcast, forward, backward, torch.optim.Adam), eps injected."""
    t = TRAJ
    B, ns, d = t["B"], t["nsigma"], t["d"]
    torch.manual_seed(seed)
    dae = build(net, kind, d, t["h"], t["L"], t["act"])
    sd0 = {k: v.clone() for k, v in dae.state_dict().items()}
    dae64 = build(net, kind, d, t["h"], t["L"], t["act"]).double()
    dae64.load_state_dict({k: v.double() for k, v in sd0.items()})
    fx = {"cfg/" + k: np.array(v) for k, v in t.items()}
    fx["kind"] = np.array(kind)
    for k, v in sd0.items():
        fx["sd/" + k] = v.numpy().copy()
    g = torch.Generator().manual_seed(seed + 1)
    opts = [(dae, torch.optim.Adam(dae.parameters(), lr=t["lr"]), torch.float32, ""), (dae64, torch.optim.Adam(dae64.parameters(), lr=t["lr"]), torch.float64, "_f64")]
    for i_ep in range(t["steps"]):
        perc = min((i_ep + 1) / float(t["sigma_annealing"]), 1.0)
        sigma = t["sigma_max"] * (1 - perc) + t["sigma_min"] * perc
        xb = 0.5 * torch.randn(B, d, generator=g)
        eps = torch.randn(B * ns, d, generator=g)
        pre = f"{i_ep}/"
        fx[pre + "x"], fx[pre + "eps"], fx[pre + "sigma"] = xb.numpy(), eps.numpy(), np.array(sigma, dtype=np.float64)
        for m, opt, dtype, tag in opts:
            x = xb.to(dtype).unsqueeze(1).expand(B, ns, d).contiguous().view(B * ns, d)
            opt.zero_grad()
            with injected_draw(eps):
                _, loss = m(x, sigma)
            loss.backward()
            opt.step()
            fx[pre + "loss" + tag] = loss.detach().numpy()
            for k, v in m.state_dict().items():
                fx[f"{pre}p{tag}/{k}"] = v.numpy().copy()
    path = os.path.join(GOLDEN, f"dae_plain_traj_{kind}.npz")
    np.savez_compressed(path, **fx)
    print(f"{path}: {os.path.getsize(path)} bytes, losses {[round(float(fx[f'{s}/loss']), 5) for s in range(t['steps'])]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=G.REF)
    ap.add_argument("--only", choices=["cases", "traj"])
    a = ap.parse_args()
    G.REF = a.reference
    net, _ = G.import_reference()
    torch.set_num_threads(8)
    for ki, kind in enumerate(("grad", "res")):
        if a.only != "traj":
            for ci, (name, shape) in enumerate(CASES.items()):
                gen_case(net, kind, name, shape, 1000 + 100 * ki + 10 * ci + 7)
        if a.only != "cases":
            gen_traj(net, kind, 2000 + ki)


if __name__ == "__main__":
    main()
