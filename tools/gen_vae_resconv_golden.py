"""Golden vectors of the residual-conv Gaussian-posterior baseline (ardae_model_desc.kind 12, `vae.py --model resconv`)  --  TEST INFRASTRUCTURE.

Runs only where the reference checkout is available (it never travels to the GPU box):

    python tools/gen_vae_resconv_golden.py [--reference DIR] [--only cases|traj|counts]

Like tools/gen_vae_conv_golden.py it imports the reference's own class (models.MNISTResConvVAE = models/vae/resconv.py::VAE) through
oracle.gen_golden.import_reference() and stores ITS outputs.  The parameters (1 813 487 at z 32, c_dim 450) are NOT stored: they come from
oracle.ardae_oracle.init_params(layout.resconv_vae_spec(z, c_dim), seed) (`resconv_params` below: weight-norm scales spread over [0.7, 1.3] so
that gradients tell them apart), are loaded into the reference class, and the tests regenerate them from the seed.  `special` restates
`do_m5bias=True` as a setting: decode.dec.17.conv_01.bias = -3 (the reference draws it from N(-3, 1e-4)); the trajectory starts from it.

  tests/golden/vae_resconv_<case>.npz   per case (B, z_dim, c_dim, do_center):
      seed, special, act ('elu'), shape = [B, z, c_dim], do_center; names, shapes: the reference's state_dict keys and shapes ("16,1,3,3")
      x, eps, dec_noise    Bernoulli images and the two draws of VAE.forward as the reference made them (recovered by replaying the seed in call order)
      mu, lv               encode(x)'s statistics
      b1/.., b03/..        beta 1.0 and 0.3: x_sample, mean, z, loss, recon, kld (forward's six outputs; x_sample / mean as [B, 784]) and every
                           parameter's .grad of loss / 784:  g/<name> in full for tensors of at most FULL_ELEMS elements, else gs/<name> =
                           [L2 norm, sum, first 8 elements]
      *_f64                the same calls on the same inputs after .double()
      lp/eps, lp/value_f64, lp/value      logprob(x, sample_size=16) on injected draws [B, 16, z] in float64 (and float32)
  tests/golden/vae_traj_resconv.npz     4 steps of vae.py's loop body (:396-417) at B 3, z 32, c_dim 450 on injected eps under the vendored Adam(lr 1e-3,
      betas (0.9, 0.999)) with beta_init 1e-4, beta_fin 1, beta_annealing 2 (the ramp ends inside the run):  cfg/<name>, seed, special, and per step s:
      <s>/x, <s>/eps, <s>/beta, <s>/loss, <s>/recon, <s>/kld, <s>/ps/<name> = [L2 norm, sum, first 8] of the parameter after the step; the same
      loop in float64 under <s>/loss_f64, ..., <s>/ps_f64/<name>
  tests/golden/vae_resconv_param_counts.npz   the parameter count of the reference's class at z 32, c_dim 450

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

# case -> (B, z_dim, c_dim, do_center, special, seed);  z6_c42: head rows off the 16-byte grid, and the class's other mode (the trunk sees 2x - 1)
CASES = {"z32_b3": (3, 32, 450, False, False, 6107), "z6_c42_b5_ct": (5, 6, 42, True, False, 6117)}
TRAJ = (3, 32, 450, False, True, 6201)
TRAJ_CFG = dict(lr=1e-3, beta1=0.9, beta_init=1e-4, beta_fin=1.0, beta_annealing=2, steps=4)
FULL_ELEMS = 16384
D = 784


def resconv_params(z, c_dim, seed, special, dtype=torch.float32):
    """The parameters of a case: oracle.init_params on layout.resconv_vae_spec(z, c_dim); special: do_m5bias as a setting (the last skip bias = -3)."""
    p = O.init_params(layout.resconv_vae_spec(z, c_dim), seed, None, dtype)
    if special:
        p["decode.dec.17.conv_01.bias"].fill_(-3.0)
    return p


def summary(t):
    t = t.detach().reshape(-1)
    return np.concatenate([np.array([t.norm().item(), t.sum().item()], dtype=t.numpy().dtype), t[:8].numpy()])


def build(net, z, c_dim, do_center, params, dtype):
    m = net.MNISTResConvVAE(input_height=28, input_channels=1, z_dim=z, c_dim=c_dim, nonlinearity="elu", do_center=do_center).to(dtype)
    assert [(n, tuple(p.shape)) for n, p in m.named_parameters()] == [(n, tuple(s)) for n, s in layout.resconv_vae_spec(z, c_dim)]
    m.load_state_dict({k: v.to(dtype).clone() for k, v in params.items()})
    return m


def forward_with_draws(model, x, seed):
    """(eps, dec_noise): the reference's own draws of one forward, recovered by replaying the seed in call order."""
    torch.manual_seed(seed)
    out = model(x.clone())
    torch.manual_seed(seed)
    eps, dec = torch.randn(x.size(0), model.z_dim), torch.rand(x.size(0), D)
    with V.injected_draws(normals=[eps], uniforms=[dec]):
        again = model(x.clone())
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(out, again)), "the replayed draws are not the ones the reference used"
    return eps, dec


def evaluate(model, x, eps, dec, lp_eps, tag, fx):
    B = x.size(0)
    with V.injected_draws(normals=[eps]):
        _, mu, lv = model.encode(x.clone())
    fx["mu" + tag], fx["lv" + tag] = mu.detach().numpy(), lv.detach().numpy()
    for b, beta in V.BETAS.items():
        with V.injected_draws(normals=[eps], uniforms=[dec]):
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
    with torch.no_grad(), V.injected_draws(normals=[None, lp_eps]):      # (the first draw is encode()'s own sample, which logprob drops)
        fx["lp/value" + tag] = model.logprob(x.clone(), sample_size=V.LP_K).numpy()


def header(model, B, z, c_dim, do_center, special, seed):
    sd = model.state_dict()
    return {"act": np.array("elu"), "shape": np.array([B, z, c_dim]), "do_center": np.array(int(do_center)), "seed": np.array(seed),
            "special": np.array(int(special)), "names": np.array(list(sd)), "shapes": np.array([",".join(str(d) for d in v.shape) for v in sd.values()])}


def gen_case(net, name, case):
    B, z, c_dim, do_center, special, seed = case
    params = resconv_params(z, c_dim, seed, special)
    model = build(net, z, c_dim, do_center, params, torch.float32)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.bernoulli(torch.full((B, D), 0.3), generator=g)
    lp_eps = torch.randn(B, V.LP_K, z, generator=g)
    fx = header(model, B, z, c_dim, do_center, special, seed)
    fx.update({"x": x.numpy(), "lp/eps": lp_eps.numpy()})
    eps, dec = forward_with_draws(model, x, seed + 2)
    fx["eps"], fx["dec_noise"] = eps.numpy(), dec.numpy()
    evaluate(model, x, eps, dec, lp_eps, "", fx)
    evaluate(build(net, z, c_dim, do_center, params, torch.float64), x.double(), eps.double(), dec.double(), lp_eps.double(), "_f64", fx)
    nparts, total = V.save_split(f"vae_resconv_{name}", fx)
    print(f"vae_resconv_{name}: {nparts} file(s), {total} bytes, loss {float(fx['b1/loss']):.6f} (fp64 {float(fx['b1/loss_f64']):.6f}), "
          f"logprob {float(fx['lp/value_f64']):.6f}")


def gen_traj(net, rutils):
    """vae.py:396-417: beta from annealing_func on the zero-based i_ep, forward, loss / 784, backward, the vendored Adam."""
    B, z, c_dim, do_center, special, seed = TRAJ
    t = TRAJ_CFG
    params = resconv_params(z, c_dim, seed, special)
    model, m64 = build(net, z, c_dim, do_center, params, torch.float32), build(net, z, c_dim, do_center, params, torch.float64)
    fx = {"cfg/" + k: np.array(v) for k, v in t.items()}
    fx.update(header(model, B, z, c_dim, do_center, special, seed))
    g = torch.Generator().manual_seed(seed + 1)
    adam = lambda m: rutils.Adam(m.parameters(), lr=t["lr"], betas=(t["beta1"], 0.999))      # noqa: E731
    runs = [(model, adam(model), torch.float32, ""), (m64, adam(m64), torch.float64, "_f64")]
    for i_ep in range(t["steps"]):
        beta = rutils.annealing_func(t["beta_init"], t["beta_fin"], t["beta_annealing"], i_ep)
        xb, eps = torch.bernoulli(torch.full((B, D), 0.3), generator=g), torch.randn(B, z, generator=g)
        pre = f"{i_ep}/"
        fx[pre + "x"], fx[pre + "eps"], fx[pre + "beta"] = xb.numpy(), eps.numpy(), np.array(beta, dtype=np.float64)
        for m, opt, dtype, tag in runs:
            opt.zero_grad()
            with V.injected_draws(normals=[eps]):
                _, _, _, loss, recon, kld = m(xb.to(dtype), beta=beta)
            (loss * (1. / float(D))).backward()
            opt.step()
            fx[pre + "loss" + tag], fx[pre + "recon" + tag], fx[pre + "kld" + tag] = loss.detach().numpy(), recon.numpy(), kld.numpy()
            for k, v in m.state_dict().items():
                fx[f"{pre}ps{tag}/{k}"] = summary(v)
    nparts, total = V.save_split("vae_traj_resconv", fx)
    print(f"vae_traj_resconv: {nparts} file(s), {total} bytes, losses {[round(float(fx[f'{s}/loss']), 5) for s in range(t['steps'])]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=G.REF)
    ap.add_argument("--only", choices=["cases", "traj", "counts"])
    a = ap.parse_args()
    G.REF = a.reference
    net, rutils = G.import_reference()
    torch.set_num_threads(8)
    if a.only in (None, "counts"):
        fx = {"resconv_32_450": np.array(sum(p.numel() for p in net.MNISTResConvVAE(z_dim=32, c_dim=450).parameters()))}
        print("vae_resconv_param_counts:", V.save_split("vae_resconv_param_counts", fx), {k: int(v) for k, v in fx.items()})
    if a.only in (None, "cases"):
        for name, case in CASES.items():
            gen_case(net, name, case)
    if a.only in (None, "traj"):
        gen_traj(net, rutils)


if __name__ == "__main__":
    main()
