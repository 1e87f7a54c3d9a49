"""Golden vectors of the PLAIN CONDITIONAL DAE score networks (ardae_cdae_desc.kind 10 / 11)  --  TEST INFRASTRUCTURE.

Runs only where the reference checkout is available (it never travels to the GPU box):

    python tools/gen_cond_dae_golden.py [--reference DIR] [--only cases|traj]

Like tools/gen_dae_golden.py it imports the reference's own classes (models.MLPGradCDAE = models/graddae/mlp.py::ConditionalDAE,
models.MLPResCDAE = models/resdae/mlp.py::ConditionalDAE) through oracle.gen_golden.import_reference() and stores THEIR outputs:

  tests/golden/cdae_plain_<kind>_<case>.npz     per kind and shape (B, S, d, c, h, L, act):
      kind, act, shape
      sd/<name>            the reference's state_dict (default nn.Linear init under a fixed seed; the constructor calls no reset_parameters)
      x [B, S, d], ctx [B, 1, c], std, eps [B*S, d]      inputs; std is a scalar in three cases and a [B*S, 1] tensor in two; eps is what the
                           reference drew (seed, call forward, re-seed, redraw randn_like)
      loss, g/<name>       forward(x, ctx, std)[1] and every parameter's .grad after loss.backward()  ("g/<name>/none": .grad is None)
      glog                 glogprob(x, ctx)
      loss_f64, g_f64/.., glog_f64      the same calls on the same inputs after .double()
  tests/golden/cdae_plain_traj_<kind>.npz       6 steps of the cDAE update of ivae_ardae.py:752-779 with one annealed noise level per step, on
      injected samples and eps: B 4 x S 8 x nsigma 2, d 2, c 3, h 48, 2 layers (the network's parameters are stored 12 times: the file stays
      under 1 MiB), softplus, std_scale 1.5, torch.optim.Adam(lr 0.005), sigma from sigma_max 1.0 to sigma_min 0.1 with sigma_annealing = 4
      (the ramp ends inside the run):  cfg/<name>, sd/<name>, and per step s:
      <s>/latent [B, S, d], <s>/mean [B, d], <s>/ctx [B, c], <s>/eps [B*S*nsigma, d], <s>/sigma (the Python float), <s>/loss, <s>/p/<name> after
      the step; the same loop in float64 on the same inputs under <s>/loss_f64, <s>/p_f64/<name>

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
from gen_ardae_golden import injected_draw  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
# (B, S, d, c, h, L, act), std (None: a [B*S, 1] tensor)
CASES = {"b4_s16_d2_softplus": ((4, 16, 2, 2, 64, 3, "softplus"), 0.5),
         "b5_s12_d3_elu": ((5, 12, 3, 5, 100, 2, "elu"), None),            # N = 60: a ragged tile
         "b6_s16_d8_tanh": ((6, 16, 8, 24, 64, 2, "tanh"), 1.25),
         "b8_s8_d2_relu1": ((8, 8, 2, 2, 64, 1, "relu"), 0.3),             # L = 1: the encoders are one `fc` each
         "b4_s16_d2_swish": ((4, 16, 2, 3, 64, 3, "swish"), None)}
TRAJ = dict(B=4, S=8, nsigma=2, d=2, c=3, h=48, L=2, act="softplus", std_scale=1.5, lr=0.005, sigma_max=1.0, sigma_min=0.1, sigma_annealing=4,
            steps=6)


def build(net, kind, d, c, h, L, act):
    ctor = net.MLPGradCDAE if kind == "grad" else net.MLPResCDAE
    return ctor(input_dim=d, context_dim=c, h_dim=h, num_hidden_layers=L, nonlinearity=act)


def forward_with_draw(dae, x, ctx, std, seed):
    """(loss, eps): the reference's own draw, recovered by replaying the seed."""
    torch.manual_seed(seed)
    _, loss = dae(x.clone(), ctx, std)
    torch.manual_seed(seed)
    eps = torch.randn_like(x.view(-1, x.size(-1)))
    with injected_draw(eps):
        _, again = dae(x.clone(), ctx, std)
    assert torch.equal(loss.detach(), again.detach()), "the replayed draw is not the one the reference used"
    return loss, eps


def evaluate(dae, x, ctx, std, eps, tag, fx):
    with injected_draw(eps):
        _, loss = dae(x.clone(), ctx, std)
    for p in dae.parameters():
        p.grad = None
    loss.backward()
    fx["loss" + tag] = loss.detach().numpy()
    for n, p in dae.named_parameters():
        if p.grad is None:
            fx[f"g{tag}/{n}/none"] = np.zeros(0)
        else:
            fx[f"g{tag}/{n}"] = p.grad.detach().numpy().copy()
    fx["glog" + tag] = dae.glogprob(x.clone(), ctx).detach().numpy()


def gen_case(net, kind, name, shape, scalar_std, seed):
    B, S, d, c, h, L, act = shape
    torch.manual_seed(seed)
    dae = build(net, kind, d, c, h, L, act)
    sd0 = {k: v.clone() for k, v in dae.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    x, ctx, std_t = torch.randn(B, S, d, generator=g), torch.randn(B, 1, c, generator=g), 0.5 * torch.randn(B * S, 1, generator=g)
    std = std_t if scalar_std is None else scalar_std
    fx = {"shape": np.array([B, S, d, c, h, L]), "act": np.array(act), "kind": np.array(kind), "x": x.numpy(), "ctx": ctx.numpy(),
          "std": std.numpy() if torch.is_tensor(std) else np.array(std, dtype=np.float64)}
    for k, v in sd0.items():
        fx["sd/" + k] = v.numpy().copy()
    loss, eps = forward_with_draw(dae, x, ctx, std, seed + 2)
    fx["eps"] = eps.numpy()
    evaluate(dae, x, ctx, std, eps, "", fx)
    assert float(fx["loss"]) == float(loss.detach())
    dae64 = build(net, kind, d, c, h, L, act).double()
    dae64.load_state_dict({k: v.double() for k, v in sd0.items()})
    evaluate(dae64, x.double(), ctx.double(), std.double() if torch.is_tensor(std) else std, eps.double(), "_f64", fx)
    path = os.path.join(GOLDEN, f"cdae_plain_{kind}_{name}.npz")
    np.savez_compressed(path, **fx)
    print(f"{path}: {os.path.getsize(path)} bytes, loss {float(fx['loss']):.6f} (fp64 {float(fx['loss_f64']):.6f})")


def gen_traj(net, kind, seed):
    """ivae_ardae.py:752-779 with the plain cDAE: centre and scale the samples, repeat each nsigma times, forward at the step's one noise level,
    backward, torch.optim.Adam; samples, means, contexts and eps injected."""
    t = TRAJ
    B, S, ns, d, c = t["B"], t["S"], t["nsigma"], t["d"], t["c"]
    torch.manual_seed(seed)
    dae = build(net, kind, d, c, t["h"], t["L"], t["act"])
    sd0 = {k: v.clone() for k, v in dae.state_dict().items()}
    dae64 = build(net, kind, d, c, t["h"], t["L"], t["act"]).double()
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
        mean = torch.randn(B, d, generator=g)
        latent = mean[:, None, :] + 0.5 * torch.randn(B, S, d, generator=g)
        ctx = torch.randn(B, c, generator=g)
        eps = torch.randn(B * S * ns, d, generator=g)
        pre = f"{i_ep}/"
        fx[pre + "latent"], fx[pre + "mean"], fx[pre + "ctx"], fx[pre + "eps"] = latent.numpy(), mean.numpy(), ctx.numpy(), eps.numpy()
        fx[pre + "sigma"] = np.array(sigma, dtype=np.float64)
        for m, opt, dtype, tag in opts:
            u = t["std_scale"] * (latent.to(dtype) - mean.to(dtype)[:, None, :])
            u = u.unsqueeze(2).expand(B, S, ns, d).contiguous().view(B, S * ns, d)
            opt.zero_grad()
            with injected_draw(eps):
                _, loss = m(u, ctx.to(dtype).view(B, 1, c), sigma)
            loss.backward()
            opt.step()
            fx[pre + "loss" + tag] = loss.detach().numpy()
            for k, v in m.state_dict().items():
                fx[f"{pre}p{tag}/{k}"] = v.numpy().copy()
    path = os.path.join(GOLDEN, f"cdae_plain_traj_{kind}.npz")
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
            for ci, (name, (shape, std)) in enumerate(CASES.items()):
                gen_case(net, kind, name, shape, std, 3000 + 100 * ki + 10 * ci + 7)
        if a.only != "cases":
            gen_traj(net, kind, 4000 + ki)


if __name__ == "__main__":
    main()
