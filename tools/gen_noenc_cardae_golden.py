"""Golden vectors of the CONDITIONAL AR-DAE WITHOUT AN INPUT ENCODER (ardae_cdae_desc.kind 16 / 17)  --  TEST INFRASTRUCTURE.

Runs only where the reference checkout is available (it never travels to the GPU box):

    python tools/gen_noenc_cardae_golden.py [--reference DIR] [--only cases|traj]

Like tools/gen_cond_dae_golden.py it imports the reference's own classes (models.MLPGradCARDAE = models/graddae/mlp.py::ConditionalARDAE,
models.MLPResCARDAE = models/resdae/mlp.py::ConditionalARDAE, both with enc_input=False) through oracle.gen_golden.import_reference() and
stores THEIR outputs:

  tests/golden/cardae_noenc_<kind>_<case>.npz     per kind and shape (B, S, d, c, h, L, act):
      kind, act, shape
      sd/<name>            the reference's state_dict (default nn.Linear init under a fixed seed; the constructor calls no reset_parameters)
      x [B, S, d], ctx [B, 1, c], std [B, S, 1] (always a tensor: ConditionalARDAE asserts one), eps [B*S, d]     inputs; eps is what the
                           reference drew (seed, call forward, re-seed, redraw randn_like)
      loss, g/<name>       forward(x, ctx, std)[1] and every parameter's .grad after loss.backward()  ("g/<name>/none": .grad is None)
      glog0, glog          glogprob(x, ctx) (std = 0) and glogprob(x, ctx, std)
      loss_f64, g_f64/.., glog0_f64, glog_f64      the same calls on the same inputs after .double()
  tests/golden/cardae_noenc_traj_<kind>.npz       6 steps of the cDAE update of ivae_ardae.py:752-779 on injected samples, means, contexts, xi
      and eps: B 4 x S 8 x nsigma 2, d 2, c 3, h 48, 2 layers, softplus, std_scale 1.5, delta 0.1, torch.optim.Adam(lr 0.001):
      cfg/<name>, sd/<name>, and per step s: <s>/latent [B, S, d], <s>/mean [B, d], <s>/ctx [B, c], <s>/xi [B*S*nsigma], <s>/eps [B*S*nsigma, d],
      <s>/loss, <s>/p/<name> after the step; the same loop in float64 on the same inputs under <s>/loss_f64, <s>/p_f64/<name>

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
from gen_cond_dae_golden import CASES, forward_with_draw  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
TRAJ = dict(B=4, S=8, nsigma=2, d=2, c=3, h=48, L=2, act="softplus", std_scale=1.5, delta=0.1, lr=0.001, steps=6)


def build(net, kind, d, c, h, L, act):
    ctor = net.MLPGradCARDAE if kind == "grad" else net.MLPResCARDAE
    return ctor(input_dim=d, context_dim=c, h_dim=h, num_hidden_layers=L, nonlinearity=act, enc_input=False)


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
    fx["glog0" + tag] = dae.glogprob(x.clone(), ctx).detach().numpy()
    fx["glog" + tag] = dae.glogprob(x.clone(), ctx, std.reshape(-1, 1)).detach().numpy()


def gen_case(net, kind, name, shape, seed):
    B, S, d, c, h, L, act = shape
    torch.manual_seed(seed)
    dae = build(net, kind, d, c, h, L, act)
    sd0 = {k: v.clone() for k, v in dae.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    x, ctx, std = torch.randn(B, S, d, generator=g), torch.randn(B, 1, c, generator=g), 0.5 * torch.randn(B, S, 1, generator=g)
    fx = {"shape": np.array([B, S, d, c, h, L]), "act": np.array(act), "kind": np.array(kind), "x": x.numpy(), "ctx": ctx.numpy(), "std": std.numpy()}
    for k, v in sd0.items():
        fx["sd/" + k] = v.numpy().copy()
    loss, eps = forward_with_draw(dae, x, ctx, std, seed + 2)
    fx["eps"] = eps.numpy()
    evaluate(dae, x, ctx, std, eps, "", fx)
    assert float(fx["loss"]) == float(loss.detach())
    dae64 = build(net, kind, d, c, h, L, act).double()
    dae64.load_state_dict({k: v.double() for k, v in sd0.items()})
    evaluate(dae64, x.double(), ctx.double(), std.double(), eps.double(), "_f64", fx)
    path = os.path.join(GOLDEN, f"cardae_noenc_{kind}_{name}.npz")
    np.savez_compressed(path, **fx)
    print(f"{path}: {os.path.getsize(path)} bytes, loss {float(fx['loss']):.6f} (fp64 {float(fx['loss_f64']):.6f})")


def gen_traj(net, kind, seed):
    """ivae_ardae.py:752-779: centre and scale the samples, std = delta * mean_d std_S(u) * xi per row, repeat each sample nsigma times, forward,
    backward, torch.optim.Adam; samples, means, contexts, xi and eps injected."""
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
        mean = torch.randn(B, d, generator=g)
        latent = mean[:, None, :] + 0.5 * torch.randn(B, S, d, generator=g)
        ctx = torch.randn(B, c, generator=g)
        xi = torch.randn(B * S * ns, generator=g)
        eps = torch.randn(B * S * ns, d, generator=g)
        pre = f"{i_ep}/"
        fx[pre + "latent"], fx[pre + "mean"], fx[pre + "ctx"], fx[pre + "xi"], fx[pre + "eps"] = latent.numpy(), mean.numpy(), ctx.numpy(), xi.numpy(), eps.numpy()
        for m, opt, dtype, tag in opts:
            u = t["std_scale"] * (latent.to(dtype) - mean.to(dtype)[:, None, :])
            std = t["delta"] * u.std(dim=1, keepdim=True).mean(dim=2, keepdim=True).expand(B, S * ns, 1) * xi.to(dtype).view(B, S * ns, 1)
            u = u.unsqueeze(2).expand(B, S, ns, d).contiguous().view(B, S * ns, d)
            opt.zero_grad()
            with injected_draw(eps):
                _, loss = m(u, ctx.to(dtype).view(B, 1, c), std)
            loss.backward()
            opt.step()
            fx[pre + "loss" + tag] = loss.detach().numpy()
            for k, v in m.state_dict().items():
                fx[f"{pre}p{tag}/{k}"] = v.numpy().copy()
    path = os.path.join(GOLDEN, f"cardae_noenc_traj_{kind}.npz")
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
            for ci, (name, (shape, _)) in enumerate(CASES.items()):
                gen_case(net, kind, name, shape, 5000 + 100 * ki + 10 * ci + 7)
        if a.only != "cases":
            gen_traj(net, kind, 6000 + ki)


if __name__ == "__main__":
    main()
