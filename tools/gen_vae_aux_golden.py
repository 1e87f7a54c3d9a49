"""Golden vectors of the auxiliary-variable Gaussian baselines (ardae_model_desc.kind 14 / 15, `vae.py --model auxmnist | auxtoy`)  --  TEST INFRASTRUCTURE.

Runs only where the reference checkout is available (it never travels to the GPU box):

    python tools/gen_vae_aux_golden.py [--reference DIR] [--only cases|traj|counts]

Like tools/gen_vae_resconv_golden.py it imports the reference's own classes (models.MNISTAuxVAE = models/vae/auxmnist.py::VAE, models.ToyAuxVAE =
models/vae/auxtoy.py::VAE) through oracle.gen_golden.import_reference() and stores THEIR outputs.  The parameters are NOT stored: they come from
`aux_params` below - oracle.ardae_oracle.init_params(layout.aux_vae_spec(...), seed), then aux_encode's log-variance bias spread over [-5, 2.5]
so that a clip is active on part of the elements - are loaded into the reference class, and the tests regenerate them from the seed.

  tests/golden/vae_<case>.npz   per case (family, B, input_dim, h_dim, noise_dim, z_dim, n_layers, act, clip):
      family, act, clip, seed, shape = [B, D, h, noise, z, L]; names, shapes: the reference's state_dict keys and shapes ("300,884")
      x, eps [B, noise + z] (rows [eps0 | eps]), dec_noise: inputs and the draws of VAE.forward as the reference made them, recovered by replaying the
                           seed in call order (aux_encode's, encode's, aux_decode's - a sample forward() drops -, the decoder's)
      mu0, lv0             aux_encode(x)'s statistics (the log-variance clipped)
      b1/.., b03/..        beta 1.0 and 0.3: x_sample, mean, z, loss, recon, kld (forward's six outputs; kld = kld + aux_kld) and every parameter's
                           .grad of loss / input_dim:  g/<name> in full for tensors of at most FULL_ELEMS elements, else gs/<name> =
                           [L2 norm, sum, first 8 elements]
      *_f64                the same calls on the same inputs after .double()
      lp/eps [B, 16, noise + z], lp/value_f64, lp/value      logprob(x, sample_size=16) on injected draws in float64 (and float32)
  tests/golden/vae_traj_auxmnist.npz, vae_traj_auxtoy.npz     4 steps of vae.py's loop body (:396-417) on injected draws under the vendored
      Adam(lr 1e-3, betas (0.5, 0.999)) with beta_init 1e-4, beta_fin 1, beta_annealing 2 (the ramp ends inside the run):  cfg/<name>, the header, and
      per step s:  <s>/x, <s>/eps, <s>/beta, <s>/loss, <s>/recon, <s>/kld, <s>/ps/<name> = [L2 norm, sum, first 8] of the parameter after the step;
      the same loop in float64 under <s>/loss_f64, ..., <s>/ps_f64/<name>
  tests/golden/vae_aux_param_counts.npz   the parameter counts of the reference's classes at the recipe's widths

Fixtures hold tensors, names and settings only; a fixture larger than PART_BYTES is written as several files (gen_vae_golden.save_split).
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
from oracle import ardae_oracle as O  # noqa: E402
import gen_vae_golden as V  # noqa: E402
from ardae_amd import layout  # noqa: E402

# case -> (family, B, D, h, noise, z, L, act, clip, seed)
CASES = {"auxmnist_n100_z32_b3": ("mnist", 3, 784, 300, 100, 32, 2, "softplus", "none", 7107),      # the recipe's widths; noise > 64
         "auxmnist_n10_z6_b5_spm6": ("mnist", 5, 36, 40, 10, 6, 1, "elu", "spm6", 7117),             # widths off the 4-float grid, L = 1, a clip
         "auxtoy_n2_z2_b7": ("toy", 7, 2, 64, 2, 2, 1, "tanh", "none", 7127),
         "auxtoy_n5_z3_b4_hard": ("toy", 4, 2, 24, 5, 3, 3, "relu", "hard", 7137)}
TRAJ = {"mnist": ("mnist", 6, 36, 40, 10, 6, 2, "softplus", "none", 7201), "toy": ("toy", 10, 2, 24, 5, 3, 2, "tanh", "hard", 7211)}
TRAJ_CFG = dict(lr=1e-3, beta1=0.5, beta_init=1e-4, beta_fin=1.0, beta_annealing=2, steps=4)
COUNTS = {"auxmnist_784_100_300_32_2": ("mnist", 784, 100, 300, 32, 2), "auxtoy_2_2_64_2_1": ("toy", 2, 2, 64, 2, 1)}
FULL_ELEMS = 16384


def aux_params(family, D, nd, h, z, L, seed, dtype=torch.float32):
    """The parameters of a case: oracle.init_params on layout.aux_vae_spec, aux_encode's log-variance bias spread over [-5, 2.5] (a clip then acts on
    part of the elements: 'hard' clamps outside [-4, 2], the softplus clips bend)."""
    p = O.init_params(layout.aux_vae_spec(family, D, nd, h, z, L), seed, None, dtype)
    p["aux_encode.reparam.logvar_fn.bias"].add_(torch.linspace(-5.0, 2.5, nd, dtype=dtype))
    return p


def summary(t):
    t = t.detach().reshape(-1)
    return np.concatenate([np.array([t.norm().item(), t.sum().item()], dtype=t.numpy().dtype), t[:8].numpy()])


def build(net, case, params, dtype):
    family, _, D, h, nd, z, L, act, clip, _ = case
    if family == "mnist":
        m = net.MNISTAuxVAE(input_dim=D, noise_dim=nd, h_dim=h, z_dim=z, nonlinearity=act, num_hidden_layers=L, clip_logvar=clip)
    else:
        m = net.ToyAuxVAE(input_dim=D, noise_dim=nd, h_dim=h, z_dim=z, nonlinearity=act, num_hidden_layers=L, clip_logvar=clip)
    m = m.to(dtype)
    assert [(n, tuple(p.shape)) for n, p in m.named_parameters()] == [(n, tuple(s)) for n, s in layout.aux_vae_spec(family, D, nd, h, z, L)]
    m.load_state_dict({k: v.to(dtype).clone() for k, v in params.items()})
    return m


def synth_x(family, B, D, g):
    return torch.bernoulli(torch.full((B, D), 0.3), generator=g) if family == "mnist" else torch.randn(B, D, generator=g)


def draws_kw(family, eps, nd, dec=None):
    """forward()'s draws in call order: aux_encode.sample, encode.sample, aux_decode.sample (dropped), then the decoder's (uniform | normal)"""
    normals = [eps[:, :nd].contiguous(), eps[:, nd:].contiguous(), None]
    if family == "mnist":
        return dict(normals=normals, uniforms=[dec])
    return dict(normals=normals + [dec])


def forward_with_draws(model, family, x, seed):
    """(eps [B, noise + z], dec_noise): the reference's own draws of one forward, recovered by replaying the seed in call order."""
    B, nd, zd, D = x.size(0), model.noise_dim, model.z_dim, model.input_dim
    torch.manual_seed(seed)
    out = model(x.clone())
    torch.manual_seed(seed)
    eps0, eps, dropped = torch.randn(B, nd), torch.randn(B, zd), torch.randn(B, nd)
    dec = torch.rand(B, D) if family == "mnist" else torch.randn(B, D)
    both = torch.cat([eps0, eps], 1)
    kw = draws_kw(family, both, nd, dec)
    kw["normals"][2] = dropped
    with V.injected_draws(**kw):
        again = model(x.clone())
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(out, again)), "the replayed draws are not the ones the reference used"
    return both, dec


def evaluate(model, family, x, eps, dec, lp_eps, tag, fx):
    B, D, nd = x.size(0), model.input_dim, model.noise_dim
    with torch.no_grad():
        _, mu0, lv0, _ = model.aux_encode(x.clone())
    fx["mu0" + tag], fx["lv0" + tag] = mu0.numpy(), lv0.numpy()
    for b, beta in V.BETAS.items():
        with V.injected_draws(**draws_kw(family, eps, nd, dec)):
            xs, mean, z, loss, recon, kld = model(x.clone(), beta=beta)
        for p in model.parameters():
            p.grad = None
        (loss / float(D)).backward()
        for name, v in (("x_sample", xs.reshape(B, D)), ("mean", mean.reshape(B, D)), ("z", z), ("loss", loss), ("recon", recon), ("kld", kld)):
            fx[f"{b}/{name}{tag}"] = v.detach().numpy().copy()
        for n, p in model.named_parameters():
            if p.numel() <= FULL_ELEMS:
                fx[f"{b}/g{tag}/{n}"] = p.grad.detach().numpy().copy()
            else:
                fx[f"{b}/gs{tag}/{n}"] = summary(p.grad)
    # logprob's draws in call order: aux_encode's own sample (dropped), the k z0's, encode._forward_all's sample (dropped), the z's
    k = lp_eps.size(1)
    lp0, lp1 = lp_eps[:, :, :nd].reshape(B * k, nd), lp_eps[:, :, nd:].reshape(B * k, 1, -1)
    with torch.no_grad(), V.injected_draws(normals=[None, lp0, None, lp1]):
        fx["lp/value" + tag] = model.logprob(x.clone(), sample_size=k).numpy()


def header(model, case):
    family, B, D, h, nd, z, L, act, clip, seed = case
    sd = model.state_dict()
    return {"family": np.array(family), "act": np.array(act), "clip": np.array(clip), "shape": np.array([B, D, h, nd, z, L]), "seed": np.array(seed),
            "names": np.array(list(sd)), "shapes": np.array([",".join(str(d) for d in v.shape) for v in sd.values()])}


def gen_case(net, name, case):
    family, B, D, h, nd, z, L, act, clip, seed = case
    params = aux_params(family, D, nd, h, z, L, seed)
    model = build(net, case, params, torch.float32)
    g = torch.Generator().manual_seed(seed + 1)
    x = synth_x(family, B, D, g)
    lp_eps = torch.randn(B, V.LP_K, nd + z, generator=g)
    fx = header(model, case)
    fx.update({"x": x.numpy(), "lp/eps": lp_eps.numpy()})
    eps, dec = forward_with_draws(model, family, x, seed + 2)
    fx["eps"], fx["dec_noise"] = eps.numpy(), dec.numpy()
    evaluate(model, family, x, eps, dec, lp_eps, "", fx)
    evaluate(build(net, case, params, torch.float64), family, x.double(), eps.double(), dec.double(), lp_eps.double(), "_f64", fx)
    nparts, total = V.save_split(f"vae_{name}", fx)
    print(f"vae_{name}: {nparts} file(s), {total} bytes, loss {float(fx['b1/loss']):.6f} (fp64 {float(fx['b1/loss_f64']):.6f}), "
          f"kld {float(fx['b1/kld_f64']):.6f}, logprob {float(fx['lp/value_f64']):.6f}, lv0 in [{fx['lv0_f64'].min():.3f}, {fx['lv0_f64'].max():.3f}]")


def gen_traj(net, rutils, key):
    """vae.py:396-417: beta from annealing_func on the zero-based i_ep, forward, loss / input_dim, backward, the vendored Adam."""
    case = TRAJ[key]
    family, B, D, h, nd, z, L, act, clip, seed = case
    t = TRAJ_CFG
    params = aux_params(family, D, nd, h, z, L, seed)
    model, m64 = build(net, case, params, torch.float32), build(net, case, params, torch.float64)
    fx = {"cfg/" + k: np.array(v) for k, v in t.items()}
    fx.update(header(model, case))
    g = torch.Generator().manual_seed(seed + 1)
    adam = lambda m: rutils.Adam(m.parameters(), lr=t["lr"], betas=(t["beta1"], 0.999))      # noqa: E731
    runs = [(model, adam(model), torch.float32, ""), (m64, adam(m64), torch.float64, "_f64")]
    for i_ep in range(t["steps"]):
        beta = rutils.annealing_func(t["beta_init"], t["beta_fin"], t["beta_annealing"], i_ep)
        xb, eps = synth_x(family, B, D, g), torch.randn(B, nd + z, generator=g)
        pre = f"{i_ep}/"
        fx[pre + "x"], fx[pre + "eps"], fx[pre + "beta"] = xb.numpy(), eps.numpy(), np.array(beta, dtype=np.float64)
        for m, opt, dtype, tag in runs:
            opt.zero_grad()
            with V.injected_draws(normals=draws_kw(family, eps, nd)["normals"]):
                _, _, _, loss, recon, kld = m(xb.to(dtype), beta=beta)
            (loss * (1. / float(D))).backward()
            opt.step()
            fx[pre + "loss" + tag], fx[pre + "recon" + tag], fx[pre + "kld" + tag] = loss.detach().numpy(), recon.numpy(), kld.numpy()
            for k, v in m.state_dict().items():
                fx[f"{pre}ps{tag}/{k}"] = summary(v)
    nparts, total = V.save_split(f"vae_traj_aux{key}", fx)
    print(f"vae_traj_aux{key}: {nparts} file(s), {total} bytes, losses {[round(float(fx[f'{s}/loss']), 5) for s in range(t['steps'])]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=G.REF)
    ap.add_argument("--only", choices=["cases", "traj", "counts"])
    a = ap.parse_args()
    G.REF = a.reference
    net, rutils = G.import_reference()
    torch.set_num_threads(8)
    if a.only in (None, "counts"):
        fx = {}
        for k, (family, D, nd, h, z, L) in COUNTS.items():
            ctor = net.MNISTAuxVAE if family == "mnist" else net.ToyAuxVAE
            fx[k] = np.array(sum(p.numel() for p in ctor(input_dim=D, noise_dim=nd, h_dim=h, z_dim=z, num_hidden_layers=L).parameters()))
        print("vae_aux_param_counts:", V.save_split("vae_aux_param_counts", fx), {k: int(v) for k, v in fx.items()})
    if a.only in (None, "cases"):
        for name, case in CASES.items():
            gen_case(net, name, case)
    if a.only in (None, "traj"):
        for key in TRAJ:
            gen_traj(net, rutils, key)


if __name__ == "__main__":
    main()
