"""Golden vectors of the hierarchical resconv Gaussian baseline (ardae_model_desc.kind 19, `vae.py --model auxresconv` / `auxresconvct`)  --  TEST INFRASTRUCTURE.

Runs only where the reference checkout is available (it never travels to the GPU box):

    python tools/gen_vae_auxresconv_golden.py [--reference DIR] [--only cases|traj|counts]

Like tools/gen_vae_auxconv_golden.py it imports the reference's own class (models.MNISTResConvAuxVAE = models/vae/auxresconv.py::VAE) through
oracle.gen_golden.import_reference() and stores ITS outputs.  The parameters are NOT stored: they come from
oracle.ardae_oracle.init_params(layout.aux_resconv_vae_spec(noise, z, c_dim), seed), are loaded into the reference class, and the tests regenerate them
from the seed.

  tests/golden/vae_<case>.npz   per case (B, noise, z, c_dim, do_center):
      act, seed, shape = [B, noise, z, c_dim], do_center; names, shapes: the reference's state_dict keys and shapes ("450,550")
      x, eps [B, noise + z] (rows [eps0 | eps]), dec_noise: inputs and the draws of VAE.forward as the reference made them, recovered by replaying the
                           seed in call order (aux_encode's, encode's, aux_decode's - a sample forward() drops -, the decoder's)
      mu0, lv0             aux_encode(inp_encode(x))'s statistics
      b1/.., b03/..        beta 1.0 and 0.3: x_sample, mean, z, loss, recon, kld (forward's six outputs; kld = kld + aux_kld) and every parameter's
                           .grad of loss / 784:  g/<name> in full for tensors of at most FULL_ELEMS elements, else gs/<name> = [L2 norm, sum, first 8]
      *_f64                the same calls on the same inputs after .double()
      lp/eps [B, 16, noise + z], lp/value_f64, lp/value      logprob(x, sample_size=16) on injected draws in float64 (and float32)
  tests/golden/vae_traj_auxresconv.npz     4 steps of vae.py's loop body (:396-417) on injected draws under the vendored Adam with TRAJ_CFG's ramp
      (beta_init 1e-4, beta_fin 1, beta_annealing 2: the ramp ends inside the run), in the layout of the aux trajectory fixtures
  tests/golden/vae_auxresconv_param_counts.npz   the parameter count of the reference's class at the recipe's widths

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
from gen_vae_aux_golden import FULL_ELEMS, TRAJ_CFG, summary  # noqa: E402
from ardae_amd import layout  # noqa: E402

D = 784
# case -> (B, noise, z, c_dim, do_center, seed)
CASES = {"auxresconv_n100_z32_c450_b3": (3, 100, 32, 450, True, 7507),      # the recipe's widths (`auxresconvct`: the trunk sees 2x - 1)
         "auxresconv_n10_z6_c42_b5": (5, 10, 6, 42, False, 7517)}           # widths off the 4-float grid, the class's other mode
TRAJ = (6, 10, 6, 42, True, 7601)
COUNTS = {"auxresconv_100_32_450": (100, 32, 450)}


def build(net, case, params, dtype):
    _, nd, z, c, ct, _ = case
    m = net.MNISTResConvAuxVAE(input_height=28, input_channels=1, z0_dim=nd, z_dim=z, c_dim=c, nonlinearity="elu", do_center=ct).to(dtype)
    assert [(n, tuple(p.shape)) for n, p in m.named_parameters()] == [(n, tuple(s)) for n, s in layout.aux_resconv_vae_spec(nd, z, c)]
    m.load_state_dict({k: v.to(dtype).clone() for k, v in params.items()})
    return m


def draws_kw(eps, nd, dec=None):
    """forward()'s draws in call order: aux_encode.sample, encode.sample, aux_decode.sample (dropped), then the decoder's uniform"""
    return dict(normals=[eps[:, :nd].contiguous(), eps[:, nd:].contiguous(), None], uniforms=[dec])


def forward_with_draws(model, x, nd, zd, seed):
    """(eps [B, noise + z], dec_noise): the reference's own draws of one forward, recovered by replaying the seed in call order."""
    B = x.size(0)
    torch.manual_seed(seed)
    out = model(x.clone())
    torch.manual_seed(seed)
    eps0, eps, dropped = torch.randn(B, nd), torch.randn(B, zd), torch.randn(B, nd)
    dec = torch.rand(B, D)
    both = torch.cat([eps0, eps], 1)
    kw = draws_kw(both, nd, dec)
    kw["normals"][2] = dropped
    with V.injected_draws(**kw):
        again = model(x.clone())
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(out, again)), "the replayed draws are not the ones the reference used"
    return both, dec


def evaluate(model, x, eps, dec, lp_eps, nd, tag, fx):
    B = x.size(0)
    with torch.no_grad():
        _, mu0, lv0 = model.aux_encode(model.inp_encode(x.clone()))
    fx["mu0" + tag], fx["lv0" + tag] = mu0.numpy(), lv0.numpy()
    for b, beta in V.BETAS.items():
        with V.injected_draws(**draws_kw(eps, nd, dec)):
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
    # logprob's draws in call order: aux_encode's own sample (dropped), the k z0's, encode's own sample (dropped), the z's, aux_decode's (dropped)
    k = lp_eps.size(1)
    lp0, lp1 = lp_eps[:, :, :nd].reshape(B * k, nd), lp_eps[:, :, nd:].reshape(B * k, 1, -1)
    with torch.no_grad(), V.injected_draws(normals=[None, lp0, None, lp1]):
        fx["lp/value" + tag] = model.logprob(x.clone(), sample_size=k).numpy()


def header(model, case):
    B, nd, z, c, ct, seed = case
    sd = model.state_dict()
    return {"act": np.array("elu"), "shape": np.array([B, nd, z, c]), "do_center": np.array(int(ct)), "seed": np.array(seed), "names": np.array(list(sd)),
            "shapes": np.array([",".join(str(d) for d in v.shape) for v in sd.values()])}


def gen_case(net, name, case):
    B, nd, z, c, ct, seed = case
    params = O.init_params(layout.aux_resconv_vae_spec(nd, z, c), seed)
    model = build(net, case, params, torch.float32)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.bernoulli(torch.full((B, D), 0.3), generator=g)
    lp_eps = torch.randn(B, V.LP_K, nd + z, generator=g)
    fx = header(model, case)
    fx.update({"x": x.numpy(), "lp/eps": lp_eps.numpy()})
    eps, dec = forward_with_draws(model, x, nd, z, seed + 2)
    fx["eps"], fx["dec_noise"] = eps.numpy(), dec.numpy()
    evaluate(model, x, eps, dec, lp_eps, nd, "", fx)
    evaluate(build(net, case, params, torch.float64), x.double(), eps.double(), dec.double(), lp_eps.double(), nd, "_f64", fx)
    nparts, total = V.save_split(f"vae_{name}", fx)
    print(f"vae_{name}: {nparts} file(s), {total} bytes, loss {float(fx['b1/loss']):.6f} (fp64 {float(fx['b1/loss_f64']):.6f}), "
          f"kld {float(fx['b1/kld_f64']):.6f}, logprob {float(fx['lp/value_f64']):.6f}")


def gen_traj(net, rutils):
    """vae.py:396-417: beta from annealing_func on the zero-based i_ep, forward, loss / 784, backward, the vendored Adam."""
    case = TRAJ
    B, nd, z, c, ct, seed = case
    t = TRAJ_CFG
    params = O.init_params(layout.aux_resconv_vae_spec(nd, z, c), seed)
    model, m64 = build(net, case, params, torch.float32), build(net, case, params, torch.float64)
    fx = {"cfg/" + k: np.array(v) for k, v in t.items()}
    fx.update(header(model, case))
    g = torch.Generator().manual_seed(seed + 1)
    adam = lambda m: rutils.Adam(m.parameters(), lr=t["lr"], betas=(t["beta1"], 0.999))      # noqa: E731
    runs = [(model, adam(model), torch.float32, ""), (m64, adam(m64), torch.float64, "_f64")]
    for i_ep in range(t["steps"]):
        beta = rutils.annealing_func(t["beta_init"], t["beta_fin"], t["beta_annealing"], i_ep)
        xb, eps = torch.bernoulli(torch.full((B, D), 0.3), generator=g), torch.randn(B, nd + z, generator=g)
        pre = f"{i_ep}/"
        fx[pre + "x"], fx[pre + "eps"], fx[pre + "beta"] = xb.numpy(), eps.numpy(), np.array(beta, dtype=np.float64)
        for m, opt, dtype, tag in runs:
            opt.zero_grad()
            with V.injected_draws(normals=draws_kw(eps, nd)["normals"]):
                _, _, _, loss, recon, kld = m(xb.to(dtype), beta=beta)
            (loss * (1. / float(D))).backward()
            opt.step()
            fx[pre + "loss" + tag], fx[pre + "recon" + tag], fx[pre + "kld" + tag] = loss.detach().numpy(), recon.numpy(), kld.numpy()
            for k, v in m.state_dict().items():
                fx[f"{pre}ps{tag}/{k}"] = summary(v)
    nparts, total = V.save_split("vae_traj_auxresconv", fx)
    print(f"vae_traj_auxresconv: {nparts} file(s), {total} bytes, losses {[round(float(fx[f'{s}/loss']), 5) for s in range(t['steps'])]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=G.REF)
    ap.add_argument("--only", choices=["cases", "traj", "counts"])
    a = ap.parse_args()
    G.REF = a.reference
    net, rutils = G.import_reference()
    torch.set_num_threads(8)
    if a.only in (None, "counts"):
        fx = {k: np.array(sum(p.numel() for p in net.MNISTResConvAuxVAE(z0_dim=nd, z_dim=z, c_dim=c).parameters())) for k, (nd, z, c) in COUNTS.items()}
        print("vae_auxresconv_param_counts:", V.save_split("vae_auxresconv_param_counts", fx), {k: int(v) for k, v in fx.items()})
    if a.only in (None, "cases"):
        for name, case in CASES.items():
            gen_case(net, name, case)
    if a.only in (None, "traj"):
        gen_traj(net, rutils)


if __name__ == "__main__":
    main()
