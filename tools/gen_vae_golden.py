"""Golden vectors of the Gaussian-posterior VAE baselines (ardae_model_desc.kind 8 / 9, vae.py)  --  TEST INFRASTRUCTURE.

Runs only where the reference checkout is available (it never travels to the GPU box):

    python tools/gen_vae_golden.py [--reference DIR] [--only cases|traj]

Like tools/gen_dae_golden.py it imports the reference's own classes (models.MNISTVAE = models/vae/mnist.py::VAE, models.ToyVAE =
models/vae/toy.py::VAE) through oracle.gen_golden.import_reference() and stores THEIR outputs:

  tests/golden/vae_<family>_<case>.npz      per family and shape (B, input_dim, h_dim, z_dim, n_layers, act):
      family, act, shape
      sd/<name>            the reference's state_dict (default init of the class under a fixed seed)
      x, eps, dec_noise    inputs and the two draws of VAE.forward as the reference made them (seed, call forward, re-seed, redraw in call
                           order: randn_like for the posterior, then rand_like (mnist) / randn_like (toy) for the decoder sample)
      mu, lv               encode(x)'s statistics
      b1/.., b03/..        beta 1.0 and 0.3: x_sample, mean, z, loss, recon, kld (forward's six outputs) and g/<name>, every parameter's
                           .grad of loss / input_dim
      *_f64                the same calls on the same inputs after .double()
      lp/eps, lp/value_f64, lp/value      logprob(x, sample_size=16) on injected draws [B, 16, z] in float64 (and float32)
  tests/golden/vae_traj_<family>.npz        5 steps of vae.py's loop body (:396-417) on injected eps under the vendored Adam(lr 1e-3, betas
      (0.5, 0.999)) with a beta ramp that ends inside the run (beta_init 1e-4, beta_fin 1, beta_annealing 3):  cfg/<name>, sd/<name>, and
      per step s:  <s>/x, <s>/eps, <s>/beta (the Python float), <s>/loss, <s>/recon, <s>/kld, <s>/p/<name> after the step; the same loop
      in float64 under <s>/loss_f64, <s>/p_f64/<name>

  tests/golden/vae_param_counts.npz         the parameter counts of the reference's classes at the recipe widths (COUNTS), from the classes

The d36_h300_z32 case keeps all four gradient sets (fp32 and float64, beta 1 and 0.3) although it is 6 MB in nine parts: it is the one fixture with
the recipe's ragged K (h 300) at the reference's own precision, the fp32 sets are what the device is compared with at the project's tolerances, the
float64 sets what pins the test-side restatement there, and the two betas separate the KL path's gradients from the reconstruction's.
A fixture larger than PART_BYTES is written as several files, <name>.npz, <name>.p1.npz, ...; a loader reads them all into one dict
(tests/test_vae_baseline.py::load).  Fixtures hold tensors, names and settings only.
"""
import argparse
import contextlib
import glob
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import gen_golden as G  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
PART_BYTES = 900_000
# family, case -> (B, input_dim, h_dim, z_dim, n_layers, act)
CASES = {("mnist", "d64_h40_z6"): (6, 64, 40, 6, 2, "softplus"), ("mnist", "d36_h300_z32"): (6, 36, 300, 32, 2, "softplus"),
         ("toy", "h40_relu"): (10, 2, 40, 2, 2, "relu"), ("toy", "h40_tanh"): (10, 2, 40, 2, 2, "tanh")}
TRAJ = {"mnist": CASES["mnist", "d64_h40_z6"], "toy": CASES["toy", "h40_relu"]}
TRAJ_CFG = dict(lr=1e-3, beta1=0.5, beta_init=1e-4, beta_fin=1.0, beta_annealing=3, steps=5)
COUNTS = {"mnist_784_300_32_2": ("mnist", 784, 300, 32, 2), "toy_2_256_2_2": ("toy", 2, 256, 2, 2)}
BETAS = {"b1": 1.0, "b03": 0.3}
LP_K = 16


@contextlib.contextmanager
def injected_draws(normals=(), uniforms=()):
    """The i-th torch.randn_like / torch.rand_like call returns normals[i] / uniforms[i] (None or past the end: a draw of torch's own)."""
    orig_n, orig_u = torch.randn_like, torch.rand_like
    calls = {"n": 0, "u": 0}

    def patched(kind, given, orig):
        def f(t, *a, **k):
            i = calls[kind]
            calls[kind] += 1
            return given[i].to(t.dtype).view_as(t) if i < len(given) and given[i] is not None else orig(t, *a, **k)
        return f
    torch.randn_like, torch.rand_like = patched("n", list(normals), orig_n), patched("u", list(uniforms), orig_u)
    try:
        yield
    finally:
        torch.randn_like, torch.rand_like = orig_n, orig_u


def build(net, family, D, h, z, L, act):
    if family == "mnist":
        return net.MNISTVAE(input_dim=D, h_dim=h, z_dim=z, nonlinearity=act, num_hidden_layers=L)
    return net.ToyVAE(input_dim=D, h_dim=h, z_dim=z, nonlinearity=act, num_hidden_layers=L)


def draws_kw(family, eps, dec):
    return dict(normals=[eps], uniforms=[dec]) if family == "mnist" else dict(normals=[eps, dec])


def synth_x(family, B, D, g):
    return torch.bernoulli(torch.full((B, D), 0.3), generator=g) if family == "mnist" else torch.randn(B, D, generator=g)


def forward_with_draws(model, family, x, seed):
    """(eps, dec_noise): the reference's own draws of one forward, recovered by replaying the seed in call order."""
    torch.manual_seed(seed)
    out = model(x.clone())
    torch.manual_seed(seed)
    eps = torch.randn(x.size(0), model.z_dim)
    dec = torch.rand(x.size(0), model.input_dim) if family == "mnist" else torch.randn(x.size(0), model.input_dim)
    with injected_draws(**draws_kw(family, eps, dec)):
        again = model(x.clone())
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(out, again)), "the replayed draws are not the ones the reference used"
    return eps, dec


def evaluate(model, family, x, eps, dec, lp_eps, tag, fx):
    D = model.input_dim
    with injected_draws(normals=[eps]):
        _, mu, lv = model.encode(x.clone())
    fx["mu" + tag], fx["lv" + tag] = mu.detach().numpy(), lv.detach().numpy()
    for b, beta in BETAS.items():
        with injected_draws(**draws_kw(family, eps, dec)):
            xs, mean, z, loss, recon, kld = model(x.clone(), beta=beta)
        for p in model.parameters():
            p.grad = None
        (loss / float(D)).backward()
        for name, v in (("x_sample", xs), ("mean", mean), ("z", z), ("loss", loss), ("recon", recon), ("kld", kld)):
            fx[f"{b}/{name}{tag}"] = v.detach().numpy().copy()
        for n, p in model.named_parameters():
            fx[f"{b}/g{tag}/{n}"] = p.grad.detach().numpy().copy()
    with torch.no_grad(), injected_draws(normals=[None, lp_eps]):      # (the first draw is encode()'s own sample, which logprob drops)
        fx["lp/value" + tag] = model.logprob(x.clone(), sample_size=LP_K).numpy()


def save_split(name, fx):
    """<name>.npz, and <name>.p1.npz, ... where the arrays exceed PART_BYTES; stale parts of an earlier run are removed first."""
    for old in glob.glob(os.path.join(GOLDEN, name + ".p*.npz")):
        os.remove(old)
    parts, size = [{}], 0
    for k, v in fx.items():
        v = np.asarray(v)
        if parts[-1] and size + v.nbytes > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = v
        size += v.nbytes
    total = 0
    for i, part in enumerate(parts):
        path = os.path.join(GOLDEN, f"{name}.npz" if i == 0 else f"{name}.p{i}.npz")
        np.savez_compressed(path, **part)
        assert os.path.getsize(path) < (1 << 20), path
        total += os.path.getsize(path)
    return len(parts), total


def gen_case(net, family, name, shape, seed):
    B, D, h, z, L, act = shape
    torch.manual_seed(seed)
    model = build(net, family, D, h, z, L, act)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    x = synth_x(family, B, D, g)
    lp_eps = torch.randn(B, LP_K, z, generator=g)
    fx = {"family": np.array(family), "act": np.array(act), "shape": np.array([B, D, h, z, L]), "x": x.numpy(), "lp/eps": lp_eps.numpy()}
    for k, v in sd0.items():
        fx["sd/" + k] = v.numpy().copy()
    eps, dec = forward_with_draws(model, family, x, seed + 2)
    fx["eps"], fx["dec_noise"] = eps.numpy(), dec.numpy()
    evaluate(model, family, x, eps, dec, lp_eps, "", fx)
    m64 = build(net, family, D, h, z, L, act).double()
    m64.load_state_dict({k: v.double() for k, v in sd0.items()})
    evaluate(m64, family, x.double(), eps.double(), dec.double(), lp_eps.double(), "_f64", fx)
    nparts, total = save_split(f"vae_{family}_{name}", fx)
    print(f"vae_{family}_{name}: {nparts} file(s), {total} bytes, loss {float(fx['b1/loss']):.6f} (fp64 {float(fx['b1/loss_f64']):.6f}), "
          f"logprob {float(fx['lp/value_f64']):.6f}")


def gen_traj(net, rutils, family, seed):
    """vae.py:396-417: beta from annealing_func on the zero-based i_ep, forward, loss / input_dim, backward, the vendored Adam."""
    B, D, h, z, L, act = TRAJ[family]
    t = TRAJ_CFG
    torch.manual_seed(seed)
    model = build(net, family, D, h, z, L, act)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    m64 = build(net, family, D, h, z, L, act).double()
    m64.load_state_dict({k: v.double() for k, v in sd0.items()})
    fx = {"cfg/" + k: np.array(v) for k, v in t.items()}
    fx.update({"family": np.array(family), "act": np.array(act), "shape": np.array([B, D, h, z, L])})
    for k, v in sd0.items():
        fx["sd/" + k] = v.numpy().copy()
    g = torch.Generator().manual_seed(seed + 1)
    adam = lambda m: rutils.Adam(m.parameters(), lr=t["lr"], betas=(t["beta1"], 0.999))      # noqa: E731
    runs = [(model, adam(model), torch.float32, ""), (m64, adam(m64), torch.float64, "_f64")]
    for i_ep in range(t["steps"]):
        beta = rutils.annealing_func(t["beta_init"], t["beta_fin"], t["beta_annealing"], i_ep)
        xb, eps = synth_x(family, B, D, g), torch.randn(B, z, generator=g)
        pre = f"{i_ep}/"
        fx[pre + "x"], fx[pre + "eps"], fx[pre + "beta"] = xb.numpy(), eps.numpy(), np.array(beta, dtype=np.float64)
        for m, opt, dtype, tag in runs:
            opt.zero_grad()
            with injected_draws(normals=[eps]):
                _, _, _, loss, recon, kld = m(xb.to(dtype), beta=beta)
            (loss * (1. / float(D))).backward()
            opt.step()
            fx[pre + "loss" + tag], fx[pre + "recon" + tag], fx[pre + "kld" + tag] = loss.detach().numpy(), recon.numpy(), kld.numpy()
            for k, v in m.state_dict().items():
                fx[f"{pre}p{tag}/{k}"] = v.numpy().copy()
    nparts, total = save_split(f"vae_traj_{family}", fx)
    print(f"vae_traj_{family}: {nparts} file(s), {total} bytes, losses {[round(float(fx[f'{s}/loss']), 5) for s in range(t['steps'])]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=G.REF)
    ap.add_argument("--only", choices=["cases", "traj", "counts"])
    a = ap.parse_args()
    G.REF = a.reference
    net, rutils = G.import_reference()
    torch.set_num_threads(8)
    if a.only in (None, "counts"):
        fx = {k: np.array(sum(p.numel() for p in build(net, f, D, h, z, nl, "softplus").parameters())) for k, (f, D, h, z, nl) in COUNTS.items()}
        print("vae_param_counts:", save_split("vae_param_counts", fx), {k: int(v) for k, v in fx.items()})
    if a.only in (None, "cases"):
        for ci, ((family, name), shape) in enumerate(CASES.items()):
            gen_case(net, family, name, shape, 3000 + 10 * ci + 7)
    if a.only in (None, "traj"):
        for fi, family in enumerate(("mnist", "toy")):
            gen_traj(net, rutils, family, 4000 + fi)


if __name__ == "__main__":
    main()
