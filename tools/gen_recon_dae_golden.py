"""Golden vectors of the RECONSTRUCTION DAEs (models.MLPDAE / models.MLPCDAE; ardae_cdae_desc.kind 7 / 11 / 13)  --  TEST INFRASTRUCTURE.

Runs only where the reference checkout is available (it never travels to the GPU box):

    python tools/gen_recon_dae_golden.py [--reference DIR] [--only cases|traj]

Like tools/gen_dae_golden.py and tools/gen_cond_dae_golden.py it imports the reference's own classes (models.MLPDAE = models/dae/mlp.py::DAE,
models.MLPCDAE = models/dae/mlp.py::ConditionalDAE) through oracle.gen_golden.import_reference() and stores THEIR outputs:

  tests/golden/recon_dae_<case>.npz            per shape (N, d, h, L, act) - the shapes of the ardae_uncond_* set; the noise type alternates
      act, noise, shape
      sd/<name>            the reference's state_dict (default nn.Linear init under a fixed seed)
      x, std, draw         inputs; std is a float >= 0.3 in three cases and a [N, 1] tensor with |std| >= 0.05 in two; draw is what the reference
                           drew (seed, call forward, re-seed, redraw randn_like / rand_like): normals, or uniforms in [0, 1)
      xbar                 add_noise(x, std) on that draw
      x_recon, loss, g/<name>      forward(x, std) and every parameter's .grad after loss.backward()
      glog                 glogprob(x, std)
      x_recon_f64, loss_f64, g_f64/.., glog_f64      the same calls on the same inputs after .double()
  tests/golden/recon_cdae_<enc>_<case>.npz     enc = x (enc_input=False) | a (enc_input=True); per shape (B, S, d, c, h, L, act) - the shapes of the
      cdae_plain_* set and one L = 1 case each.  As above with ctx [B, S, c]: one context row PER SAMPLE ROW in half of the cases ("rows" = 1), a
      [B, 1, c] context repeated over S in the other half ("rows" = 0).
  tests/golden/recon_dae_traj_<noise>.npz      6 steps of a dae_toy-style loop with MLPDAE on injected draws: B 16 x num_sigma 4, d 2, h 64, 3 layers,
      softplus, torch.optim.Adam(lr 0.005), sigma from 1.0 to 0.1 with sigma_annealing = 4 (the ramp ends inside the run):  cfg/<name>, sd/<name>,
      and per step s:  <s>/x [B, d], <s>/eps (the raw draw), <s>/sigma (the Python float), <s>/loss, <s>/p/<name> after the step; the same loop
      in float64 under <s>/loss_f64, <s>/p_f64/<name>
  tests/golden/recon_cdae_traj_<noise>.npz     the same with MLPCDAE(enc_input=False) on centred, scaled samples (ivae_ardae.py:752-779): B 4 x S 16 x
      nsigma 4, d 2, c 3, h 48, 2 layers (the parameters are stored 12 times: the file stays under 1 MiB), std_scale 1.5; per step <s>/latent [B, S, d], <s>/mean [B, d], <s>/ctx [B, c] (one context per image)

Fixtures hold tensors, names and settings only.
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
sys.path.insert(0, HERE)
from oracle import gen_golden as G  # noqa: E402
from gen_ardae_golden import CASES as SHAPES, injected_draw  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
# name -> noise, std (None: a [N, 1] tensor)
CASES = {"n64_d2_softplus": ("gaussian", 0.5), "n60_d3_elu": ("uniform", 0.3), "n64_d2_swish": ("gaussian", None), "n64_d2_relu1": ("uniform", None),
         "n96_d8_tanh": ("gaussian", 1.25)}
# name -> (B, S, d, c, h, L, act), std (None: a [B*S, 1] tensor), per-row contexts; enc_input False and True for each; noise alternates over the list
CCASES = {"b4_s16_d2": ((4, 16, 2, 2, 64, 3, "softplus"), 0.5, True),
          "b5_s12_d3": ((5, 12, 3, 5, 100, 2, "elu"), None, False),           # N = 60: a ragged tile
          "b4_s16_d2_swish": ((4, 16, 2, 3, 64, 3, "swish"), None, True),
          "b8_s8_d2_relu1": ((8, 8, 2, 2, 64, 1, "relu"), 0.3, False),        # L = 1: ctx_encode is one Linear
          "b6_s16_d8_tanh": ((6, 16, 8, 24, 64, 2, "tanh"), 1.25, True),
          "b3_s20_d3_tanh1": ((3, 20, 3, 4, 32, 1, "tanh"), 0.4, False)}
TRAJ = dict(B=16, nsigma=4, d=2, h=64, L=3, act="softplus", lr=0.005, sigma_max=1.0, sigma_min=0.1, sigma_annealing=4, steps=6)
CTRAJ = dict(B=4, S=16, nsigma=4, d=2, c=3, h=48, L=2, act="softplus", std_scale=1.5, lr=0.005, sigma_max=1.0, sigma_min=0.1, sigma_annealing=4, steps=6)


@contextlib.contextmanager
def injected_uniform(u):
    """injected_draw's twin for add_uniform_noise: the next torch.rand_like returns `u`."""
    orig = torch.rand_like
    torch.rand_like = lambda t, *a, **k: u.to(t.dtype)
    try:
        yield
    finally:
        torch.rand_like = orig


def injected(noise, draw):
    return injected_draw(draw) if noise == "gaussian" else injected_uniform(draw)


def tensor_std(n, g):
    """[n, 1] with 0.05 <= |std| (the score divides by std^2)"""
    s = 0.5 * torch.randn(n, 1, generator=g)
    return torch.where(s.abs() < 0.05, torch.full_like(s, 0.05), s)


def forward_with_draw(dae, noise, args, std, seed):
    """(loss, draw): the reference's own draw, recovered by replaying the seed."""
    x = args[0]
    torch.manual_seed(seed)
    _, loss = dae(*args, std)
    torch.manual_seed(seed)
    rows = x.reshape(-1, x.size(-1))
    draw = torch.randn_like(rows) if noise == "gaussian" else torch.rand_like(rows)
    with injected(noise, draw):
        _, again = dae(*args, std)
    assert torch.equal(loss.detach(), again.detach()), "the replayed draw is not the one the reference used"
    return loss, draw


def evaluate(dae, noise, args, std, draw, tag, fx):
    with injected(noise, draw):
        x_recon, loss = dae(*args, std)
    for p in dae.parameters():
        p.grad = None
    loss.backward()
    fx["loss" + tag], fx["x_recon" + tag] = loss.detach().numpy(), x_recon.detach().numpy()
    for n, p in dae.named_parameters():
        fx[f"g{tag}/{n}"] = p.grad.detach().numpy().copy()
    fx["glog" + tag] = dae.glogprob(*args, std).detach().numpy()
    with injected(noise, draw):
        rows = args[0].reshape(-1, args[0].size(-1))
        fx["xbar" + tag] = dae.add_noise(rows, std).detach().numpy()


def finish(build, noise, args, std, fx, seed, path):
    dae = build()
    sd0 = {k: v.clone() for k, v in dae.state_dict().items()}
    for k, v in sd0.items():
        fx["sd/" + k] = v.numpy().copy()
    fx["noise"] = np.array(noise)
    fx["std"] = std.numpy() if torch.is_tensor(std) else np.array(std, dtype=np.float64)
    loss, draw = forward_with_draw(dae, noise, args, std, seed)
    fx["draw"] = draw.numpy()
    evaluate(dae, noise, args, std, draw, "", fx)
    assert float(fx["loss"]) == float(loss.detach())
    dae64 = build().double()
    dae64.load_state_dict({k: v.double() for k, v in sd0.items()})
    evaluate(dae64, noise, tuple(a.double() for a in args), std.double() if torch.is_tensor(std) else std, draw.double(), "_f64", fx)
    np.savez_compressed(path, **fx)
    print(f"{path}: {os.path.getsize(path)} bytes, {noise}, loss {float(fx['loss']):.6f} (fp64 {float(fx['loss_f64']):.6f})")


def gen_case(net, name, seed):
    N, d, h, L, act = SHAPES[name]
    noise, scalar_std = CASES[name]
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed + 1)
    x, std_t = torch.randn(N, d, generator=g), tensor_std(N, g)
    fx = {"shape": np.array([N, d, h, L]), "act": np.array(act), "x": x.numpy()}
    build = lambda: net.MLPDAE(input_dim=d, h_dim=h, num_hidden_layers=L, nonlinearity=act, noise_type=noise)
    finish(build, noise, (x,), std_t if scalar_std is None else scalar_std, fx, seed + 2, os.path.join(GOLDEN, f"recon_dae_{name}.npz"))


def gen_ccase(net, name, enc_input, noise, seed):
    (B, S, d, c, h, L, act), scalar_std, per_row = CCASES[name]
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed + 1)
    x, std_t = torch.randn(B, S, d, generator=g), tensor_std(B * S, g)
    ctx = torch.randn(B, S, c, generator=g) if per_row else torch.randn(B, 1, c, generator=g).expand(B, S, c).contiguous()
    fx = {"shape": np.array([B, S, d, c, h, L]), "act": np.array(act), "enc_input": np.array(int(enc_input)), "rows": np.array(int(per_row)),
          "x": x.numpy(), "ctx": ctx.numpy()}
    build = lambda: net.MLPCDAE(input_dim=d, context_dim=c, h_dim=h, num_hidden_layers=L, nonlinearity=act, noise_type=noise, enc_input=enc_input)
    finish(build, noise, (x, ctx), std_t if scalar_std is None else scalar_std, fx, seed + 2,
           os.path.join(GOLDEN, f"recon_cdae_{'a' if enc_input else 'x'}_{name}.npz"))


def gen_traj(net, noise, conditional, seed):
    """The training cell of notebooks/dae_toy.ipynb with MLPDAE, or the cDAE update of ivae_ardae.py:752-779 with MLPCDAE(enc_input=False): sigma
    schedule, broadcast, forward, backward, torch.optim.Adam; samples and draws injected."""
    t = CTRAJ if conditional else TRAJ
    B, ns, d = t["B"], t["nsigma"], t["d"]
    if conditional:
        S, c = t["S"], t["c"]
        build = lambda: net.MLPCDAE(input_dim=d, context_dim=c, h_dim=t["h"], num_hidden_layers=t["L"], nonlinearity=t["act"], noise_type=noise, enc_input=False)
    else:
        build = lambda: net.MLPDAE(input_dim=d, h_dim=t["h"], num_hidden_layers=t["L"], nonlinearity=t["act"], noise_type=noise)
    torch.manual_seed(seed)
    dae = build()
    sd0 = {k: v.clone() for k, v in dae.state_dict().items()}
    dae64 = build().double()
    dae64.load_state_dict({k: v.double() for k, v in sd0.items()})
    fx = {"cfg/" + k: np.array(v) for k, v in t.items()}
    fx["noise"] = np.array(noise)
    for k, v in sd0.items():
        fx["sd/" + k] = v.numpy().copy()
    g = torch.Generator().manual_seed(seed + 1)
    opts = [(dae, torch.optim.Adam(dae.parameters(), lr=t["lr"]), torch.float32, ""), (dae64, torch.optim.Adam(dae64.parameters(), lr=t["lr"]), torch.float64, "_f64")]
    for i_ep in range(t["steps"]):
        perc = min((i_ep + 1) / float(t["sigma_annealing"]), 1.0)
        sigma = t["sigma_max"] * (1 - perc) + t["sigma_min"] * perc
        pre = f"{i_ep}/"
        if conditional:
            mean = torch.randn(B, d, generator=g)
            latent = mean[:, None, :] + 0.5 * torch.randn(B, S, d, generator=g)
            ctx = torch.randn(B, c, generator=g)
            fx[pre + "latent"], fx[pre + "mean"], fx[pre + "ctx"] = latent.numpy(), mean.numpy(), ctx.numpy()
            rows = B * S * ns
        else:
            xb = 0.5 * torch.randn(B, d, generator=g)
            fx[pre + "x"] = xb.numpy()
            rows = B * ns
        draw = torch.randn(rows, d, generator=g) if noise == "gaussian" else torch.rand(rows, d, generator=g)
        fx[pre + "eps"], fx[pre + "sigma"] = draw.numpy(), np.array(sigma, dtype=np.float64)
        for m, opt, dtype, tag in opts:
            if conditional:
                u = t["std_scale"] * (latent.to(dtype) - mean.to(dtype)[:, None, :])
                u = u.unsqueeze(2).expand(B, S, ns, d).contiguous().view(B, S * ns, d)
                args = (u, ctx.to(dtype).view(B, 1, c).expand(B, S * ns, c).contiguous())
            else:
                args = (xb.to(dtype).unsqueeze(1).expand(B, ns, d).contiguous().view(B * ns, d),)
            opt.zero_grad()
            with injected(noise, draw):
                _, loss = m(*args, sigma)
            loss.backward()
            opt.step()
            fx[pre + "loss" + tag] = loss.detach().numpy()
            for k, v in m.state_dict().items():
                fx[f"{pre}p{tag}/{k}"] = v.numpy().copy()
    path = os.path.join(GOLDEN, f"recon_{'cdae' if conditional else 'dae'}_traj_{noise}.npz")
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
    if a.only != "traj":
        for ci, name in enumerate(CASES):
            gen_case(net, name, 5000 + 10 * ci + 7)
        for ci, name in enumerate(CCASES):
            for ei, enc_input in enumerate((False, True)):
                gen_ccase(net, name, enc_input, ("gaussian", "uniform")[(ci + ei) % 2], 6000 + 100 * ei + 10 * ci + 7)
    if a.only != "cases":
        for ni, noise in enumerate(("gaussian", "uniform")):
            gen_traj(net, noise, False, 7000 + ni)
            gen_traj(net, noise, True, 7100 + ni)


if __name__ == "__main__":
    main()
