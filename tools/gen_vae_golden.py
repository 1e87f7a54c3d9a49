"""Golden vectors of the Gaussian-posterior VAE baselines (the reference's vae.py; ardae_model_desc.kind 8 / 9 / 11 / 12 / 14 / 15 / 17 / 19)  --
TEST INFRASTRUCTURE.

Runs only where the reference checkout is available (it never travels to the GPU box):

    python tools/gen_vae_golden.py [--reference DIR] [--family NAME ...] [--only cases|traj|counts]

It imports the reference's own classes through oracle.gen_golden.import_reference() and stores THEIR outputs.  FAMILIES below holds what differs
between the eight families; everything else is common:

  tests/golden/<case>.npz          per case of a family (the names are the keys of its `cases`):
      the header           the family's `fields` in their order; `shape` holds the case's `shape` entries; booleans are stored as 0 / 1
      names, shapes        the reference's state_dict keys and shapes ("16,1,5,5"), where the parameters come from a recipe; those families store
                           `seed` and NOT the parameters: oracle.fixture_params makes them from the seed, they are loaded into the reference
                           class (names and shapes asserted), and the tests regenerate them with the same call
      x, lp/eps            Bernoulli(0.3) images (toy families: normals) and logprob's draws [B, 16, noise + z]
      sd/<name>            mnist and toy only: the reference's state_dict, the default init of the class under torch.manual_seed(seed)
      eps, dec_noise       the draws of VAE.forward as the reference made them: seed, call forward, re-seed, redraw in call order (randn_like for the
                           posterior, then rand_like - toy families: randn_like - for the decoder sample) and check that forward on the injected
                           draws returns the same.  Aux families draw aux_encode's, encode's, aux_decode's (a sample forward() drops), then the
                           decoder's; eps is [B, noise + z], rows [eps0 | eps]
      mu, lv               encode(x)'s statistics; aux families: mu0, lv0 of aux_encode(x) (the log-variance clipped); auxresconv:
                           aux_encode(inp_encode(x))
      b1/.., b03/..        beta 1.0 and 0.3: x_sample, mean (both as [B, D]), z, loss, recon, kld (forward's six outputs; aux families: kld = kld +
                           aux_kld) and every parameter's .grad of loss / D:  g/<name> in full for tensors of at most FULL_ELEMS elements, else
                           gs/<name> = [L2 norm, sum, first 8 elements]; mnist and toy store every gradient in full
      *_f64                the same calls on the same inputs after .double()
      lp/value_f64, lp/value      logprob(x, sample_size=16) on the injected draws in float64 (and float32)
  tests/golden/vae_traj_<family>.npz     `steps` steps of vae.py's loop body (:396-417: beta from annealing_func on the zero-based i_ep, forward,
      loss / D, backward) on injected draws under the vendored Adam(lr, betas (beta1, 0.999)) with a beta ramp that ends inside the run:
      cfg/<name> (the family's `traj_cfg`), the header (and sd/<name>), and per step s:  <s>/x, <s>/eps, <s>/beta (the Python float), <s>/loss,
      <s>/recon, <s>/kld, <s>/ps/<name> = [L2 norm, sum, first 8] of the parameter after the step (mnist and toy: <s>/p/<name>, the parameter); the
      same loop in float64 under <s>/loss_f64, ..., <s>/ps_f64/<name>
  tests/golden/<counts file>.npz         the parameter counts of the reference's classes at the recipes' widths, from the classes

A fixture larger than PART_BYTES is written as several files, <name>.npz, <name>.p1.npz, ...; a loader reads them all into one dict
(tests/vae_restate.py::load).  save_split walks the fixture in insertion order, so the order in which keys enter it decides which part an array
lands in.  Fixtures hold tensors, names and settings only.

  mnist, toy       models.MNISTVAE = models/vae/mnist.py::VAE, models.ToyVAE = models/vae/toy.py::VAE.  The seeds come from the position in PLAIN.
                   vae_mnist_d36_h300_z32 keeps all four gradient sets (fp32 and float64, beta 1 and 0.3) although it is 6 MB in nine parts: it is
                   the one fixture with the recipe's ragged K (h 300) at the reference's own precision, the fp32 sets are what the device is compared
                   with at the project's tolerances, the float64 sets what pins the test-side restatement there, and the two betas separate the KL
                   path's gradients from the reconstruction's.
  conv             models.MNISTConvVAE = models/vae/conv.py::VAE, 703 405 parameters.  z6 / tanh: a head whose rows miss the 16-byte grid (the
                   unfused path), a second activation through the trunk.  The trajectory starts from the `special` init.
  resconv          models.MNISTResConvVAE = models/vae/resconv.py::VAE, 1 813 487 parameters at z 32, c_dim 450.  z6_c42: head rows off the 16-byte
                   grid, and the class's other mode (do_center: the trunk sees 2x - 1).  The trajectory starts from `special` and runs Adam at beta1 0.9.
  auxmnist, auxtoy models.MNISTAuxVAE = models/vae/auxmnist.py::VAE, models.ToyAuxVAE = models/vae/auxtoy.py::VAE; `family` is stored as mnist | toy.
                   n100_z32: the recipe's widths, noise > 64; n10_z6_spm6: widths off the 4-float grid, L = 1, a clip.
  auxconv          models.MNISTConvAuxVAE = models/vae/auxconv.py::VAE, 2 027 965 parameters at the recipe's widths.  n10_z6_elu: widths off the
                   4-float grid; act'(0) != 0: the zero pad's gradient must be cut.
  auxresconv       models.MNISTResConvAuxVAE = models/vae/auxresconv.py::VAE (`vae.py --model auxresconv` / `auxresconvct`).  n100_z32_c450: the
                   recipe's widths with do_center; n10_z6_c42: widths off the 4-float grid, the class's other mode.
"""
import contextlib
import glob
import os

import numpy as np
import torch

from golden_common import GOLDEN, open_reference
from oracle import fixture_params as P

PART_BYTES = 900_000
FULL_ELEMS = 16384
BETAS = {"b1": 1.0, "b03": 0.3}
LP_K = 16
TRAJ_CFG = dict(lr=1e-3, beta1=0.5, beta_init=1e-4, beta_fin=1.0, beta_annealing=2, steps=4)
# family, case -> (B, D, h, z, L, act); a case's seed is 3000 + 10 * (its position here) + 7, a trajectory's 4000 + (the family's position)
PLAIN = {("mnist", "d64_h40_z6"): (6, 64, 40, 6, 2, "softplus"), ("mnist", "d36_h300_z32"): (6, 36, 300, 32, 2, "softplus"),
         ("toy", "h40_relu"): (10, 2, 40, 2, 2, "relu"), ("toy", "h40_tanh"): (10, 2, 40, 2, 2, "tanh")}


def plain(kind, ctor, traj, counts):
    return dict(ctor=ctor, kind=kind, toy=kind == "toy", keys=("B", "D", "h", "z", "L", "act", "seed"), params=None, full=True,
                kw=lambda c: dict(input_dim=c["D"], h_dim=c["h"], z_dim=c["z"], nonlinearity=c["act"], num_hidden_layers=c["L"]),
                fields=("family", "act", "shape"), shape=("B", "D", "h", "z", "L"), stats=lambda m, x: m.encode(x),
                cases={f"vae_{k}_{n}": s + (3000 + 10 * ci + 7,) for ci, ((k, n), s) in enumerate(PLAIN.items()) if k == kind},
                traj=PLAIN[kind, traj] + (4000 + ("mnist", "toy").index(kind),), traj_cfg=dict(TRAJ_CFG, beta_annealing=3, steps=5),
                counts_file="vae_param_counts", counts=counts)


def auxmlp(kind, ctor, cases, traj, counts):
    return dict(ctor=ctor, kind=kind, toy=kind == "toy", keys=("B", "D", "h", "noise", "z", "L", "act", "clip", "seed"),
                kw=lambda c: dict(input_dim=c["D"], noise_dim=c["noise"], h_dim=c["h"], z_dim=c["z"], nonlinearity=c["act"], num_hidden_layers=c["L"],
                                  clip_logvar=c["clip"]),
                params=lambda c: P.aux(kind, c["D"], c["noise"], c["h"], c["z"], c["L"], c["seed"]),
                fields=("family", "act", "clip", "shape", "seed"), shape=("B", "D", "h", "noise", "z", "L"), stats=lambda m, x: m.aux_encode(x),
                cases=cases, traj=traj, counts_file="vae_aux_param_counts", counts=counts)


# What differs between the families.  ctor: the reference class; keys: what a case tuple holds (`noise`: an aux family); kw: its constructor keywords;
# params: the recipe (None: the class's default init, stored as sd/<name>); fields, shape: the header; stats: the statistics call; toy: normal
# inputs and a normal decoder draw; full: gradients and trajectory parameters stored in full; counts: key -> constructor keywords
FAMILIES = {
    "mnist": plain("mnist", "MNISTVAE", "d64_h40_z6", {"mnist_784_300_32_2": dict(input_dim=784, h_dim=300, z_dim=32, num_hidden_layers=2)}),
    "toy": plain("toy", "ToyVAE", "h40_relu", {"toy_2_256_2_2": dict(input_dim=2, h_dim=256, z_dim=2, num_hidden_layers=2)}),
    "conv": dict(ctor="MNISTConvVAE", keys=("B", "z", "act", "special", "seed"),
                 kw=lambda c: dict(input_height=28, input_channels=1, z_dim=c["z"], nonlinearity=c["act"]),
                 params=lambda c: P.conv(c["z"], c["seed"], c["special"]),
                 fields=("act", "shape", "seed", "special"), shape=("B", "z"), stats=lambda m, x: m.encode(x),
                 cases={"vae_conv_z32_b3": (3, 32, "softplus", False, 5107), "vae_conv_z6_b5": (5, 6, "tanh", False, 5117)},
                 traj=(3, 32, "softplus", True, 5201), counts_file="vae_conv_param_counts", counts={"conv_32": dict(z_dim=32)}),
    "resconv": dict(ctor="MNISTResConvVAE", keys=("B", "z", "c_dim", "do_center", "special", "seed", "act"),
                    kw=lambda c: dict(input_height=28, input_channels=1, z_dim=c["z"], c_dim=c["c_dim"], nonlinearity=c["act"], do_center=c["do_center"]),
                    params=lambda c: P.resconv(c["z"], c["c_dim"], c["seed"], c["special"]),
                    fields=("act", "shape", "do_center", "seed", "special"), shape=("B", "z", "c_dim"), stats=lambda m, x: m.encode(x),
                    cases={"vae_resconv_z32_b3": (3, 32, 450, False, False, 6107, "elu"), "vae_resconv_z6_c42_b5_ct": (5, 6, 42, True, False, 6117, "elu")},
                    traj=(3, 32, 450, False, True, 6201, "elu"), traj_cfg=dict(TRAJ_CFG, beta1=0.9),
                    counts_file="vae_resconv_param_counts", counts={"resconv_32_450": dict(z_dim=32, c_dim=450)}),
    "auxmnist": auxmlp("mnist", "MNISTAuxVAE",
                       {"vae_auxmnist_n100_z32_b3": (3, 784, 300, 100, 32, 2, "softplus", "none", 7107),
                        "vae_auxmnist_n10_z6_b5_spm6": (5, 36, 40, 10, 6, 1, "elu", "spm6", 7117)}, (6, 36, 40, 10, 6, 2, "softplus", "none", 7201),
                       {"auxmnist_784_100_300_32_2": dict(input_dim=784, noise_dim=100, h_dim=300, z_dim=32, num_hidden_layers=2)}),
    "auxtoy": auxmlp("toy", "ToyAuxVAE",
                     {"vae_auxtoy_n2_z2_b7": (7, 2, 64, 2, 2, 1, "tanh", "none", 7127), "vae_auxtoy_n5_z3_b4_hard": (4, 2, 24, 5, 3, 3, "relu", "hard", 7137)},
                     (10, 2, 24, 5, 3, 2, "tanh", "hard", 7211), {"auxtoy_2_2_64_2_1": dict(input_dim=2, noise_dim=2, h_dim=64, z_dim=2, num_hidden_layers=1)}),
    "auxconv": dict(ctor="MNISTConvAuxVAE", keys=("B", "noise", "z", "act", "seed"),
                    kw=lambda c: dict(z0_dim=c["noise"], z_dim=c["z"], nonlinearity=c["act"]),
                    params=lambda c: P.auxconv(c["noise"], c["z"], c["seed"]),
                    fields=("act", "shape", "seed"), shape=("B", "noise", "z"), stats=lambda m, x: m.aux_encode(x),
                    cases={"vae_auxconv_n100_z32_b3": (3, 100, 32, "softplus", 7307), "vae_auxconv_n10_z6_b5_elu": (5, 10, 6, "elu", 7317)},
                    traj=(6, 10, 6, "softplus", 7401), counts_file="vae_auxconv_param_counts", counts={"auxconv_100_32": dict(z0_dim=100, z_dim=32)}),
    "auxresconv": dict(ctor="MNISTResConvAuxVAE", keys=("B", "noise", "z", "c_dim", "do_center", "seed", "act"),
                       kw=lambda c: dict(input_height=28, input_channels=1, z0_dim=c["noise"], z_dim=c["z"], c_dim=c["c_dim"], nonlinearity=c["act"],
                                         do_center=c["do_center"]),
                       params=lambda c: P.auxresconv(c["noise"], c["z"], c["c_dim"], c["seed"]),
                       fields=("act", "shape", "do_center", "seed"), shape=("B", "noise", "z", "c_dim"),
                       stats=lambda m, x: m.aux_encode(m.inp_encode(x)),
                       cases={"vae_auxresconv_n100_z32_c450_b3": (3, 100, 32, 450, True, 7507, "elu"),
                              "vae_auxresconv_n10_z6_c42_b5": (5, 10, 6, 42, False, 7517, "elu")},
                       traj=(6, 10, 6, 42, True, 7601, "elu"), counts_file="vae_auxresconv_param_counts",
                       counts={"auxresconv_100_32_450": dict(z0_dim=100, z_dim=32, c_dim=450)}),
}


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


def summary(t):
    t = t.detach().reshape(-1)
    return np.concatenate([np.array([t.norm().item(), t.sum().item()], dtype=t.numpy().dtype), t[:8].numpy()])


def case_of(fam, values):
    """A case tuple as a dict over the family's keys, with D (784 for the image families) and noise (0 outside the aux families)"""
    return dict({"D": 784, "noise": 0}, **dict(zip(fam["keys"], values)))


def builder(net, fam, c):
    """-> (parameters, build): build(dtype) is the reference class in that dtype holding the case's fp32 parameters"""
    ctor, kw = getattr(net, fam["ctor"]), fam["kw"](c)
    if fam["params"]:
        params = fam["params"](c)
    else:
        torch.manual_seed(c["seed"])
        params = {k: v.clone() for k, v in ctor(**kw).state_dict().items()}

    def build(dtype):
        m = ctor(**kw).to(dtype)
        assert [(n, tuple(p.shape)) for n, p in m.named_parameters()] == [(n, tuple(v.shape)) for n, v in params.items()]
        m.load_state_dict({k: v.to(dtype).clone() for k, v in params.items()})
        return m
    return params, build


def header(fam, c, params):
    vals = dict(c, family=fam.get("kind"), shape=[c[k] for k in fam["shape"]])
    fx = {k: np.array(int(vals[k]) if isinstance(vals[k], bool) else vals[k]) for k in fam["fields"]}
    if fam["params"]:
        fx["names"], fx["shapes"] = np.array(list(params)), np.array([",".join(str(d) for d in v.shape) for v in params.values()])
    return fx


def stored_params(fam, params):
    return {} if fam["params"] else {"sd/" + k: v.numpy().copy() for k, v in params.items()}


def synth_x(fam, B, D, g):
    return torch.randn(B, D, generator=g) if fam.get("toy") else torch.bernoulli(torch.full((B, D), 0.3), generator=g)


def draws(fam, nd, eps, dec=None, dropped=None):
    """forward()'s draws in call order: [aux_encode.sample,] encode.sample, [aux_decode.sample (which forward drops),] then the decoder's
    (uniform; toy: normal).  None: a draw of torch's own."""
    normals = [eps[:, :nd].contiguous(), eps[:, nd:].contiguous(), dropped] if nd else [eps]
    return dict(normals=normals + [dec]) if fam.get("toy") else dict(normals=normals, uniforms=[dec])


def forward_with_draws(model, fam, c, x, seed):
    """(eps [B, noise + z], dec_noise): the reference's own draws of one forward, recovered by replaying the seed in call order."""
    (B, D), nd, z = x.shape, c["noise"], c["z"]
    torch.manual_seed(seed)
    out = model(x.clone())
    torch.manual_seed(seed)
    eps0, eps, dropped = (torch.randn(B, nd), torch.randn(B, z), torch.randn(B, nd)) if nd else (torch.zeros(B, 0), torch.randn(B, z), None)
    dec = torch.randn(B, D) if fam.get("toy") else torch.rand(B, D)
    both = torch.cat([eps0, eps], 1)
    with injected_draws(**draws(fam, nd, both, dec, dropped)):
        again = model(x.clone())
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(out, again)), "the replayed draws are not the ones the reference used"
    return both, dec


def evaluate(model, fam, c, x, eps, dec, lp_eps, tag, fx):
    (B, D), nd, aux = x.shape, c["noise"], "0" if c["noise"] else ""
    with torch.no_grad():
        _, mu, lv = fam["stats"](model, x.clone())[:3]
    fx["mu" + aux + tag], fx["lv" + aux + tag] = mu.numpy(), lv.numpy()
    for b, beta in BETAS.items():
        with injected_draws(**draws(fam, nd, eps, dec)):
            xs, mean, z, loss, recon, kld = model(x.clone(), beta=beta)
        for p in model.parameters():
            p.grad = None
        (loss / float(D)).backward()
        for name, v in (("x_sample", xs.reshape(B, D)), ("mean", mean.reshape(B, D)), ("z", z), ("loss", loss), ("recon", recon), ("kld", kld)):
            fx[f"{b}/{name}{tag}"] = v.detach().numpy().copy()
        for n, p in model.named_parameters():
            if fam.get("full") or p.numel() <= FULL_ELEMS:
                fx[f"{b}/g{tag}/{n}"] = p.grad.detach().numpy().copy()
            else:
                fx[f"{b}/gs{tag}/{n}"] = summary(p.grad)
    # logprob's draws in call order: encode()'s own sample (which logprob drops), then the k z's; an aux family: aux_encode's own sample (dropped),
    # the k z0's, encode's own sample (dropped), the z's
    lp0, lp1 = lp_eps[:, :, :nd].reshape(B * LP_K, nd), lp_eps[:, :, nd:].reshape(B * LP_K, 1, -1)
    with torch.no_grad(), injected_draws(normals=[None, lp0, None, lp1] if nd else [None, lp_eps]):
        fx["lp/value" + tag] = model.logprob(x.clone(), sample_size=LP_K).numpy()


def gen_case(net, fam, name, c):
    B, D, nd, z, seed = c["B"], c["D"], c["noise"], c["z"], c["seed"]
    params, build = builder(net, fam, c)
    model = build(torch.float32)
    g = torch.Generator().manual_seed(seed + 1)
    x = synth_x(fam, B, D, g)
    lp_eps = torch.randn(B, LP_K, nd + z, generator=g)
    fx = header(fam, c, params)
    fx.update({"x": x.numpy(), "lp/eps": lp_eps.numpy()})
    fx.update(stored_params(fam, params))
    eps, dec = forward_with_draws(model, fam, c, x, seed + 2)
    fx["eps"], fx["dec_noise"] = eps.numpy(), dec.numpy()
    evaluate(model, fam, c, x, eps, dec, lp_eps, "", fx)
    evaluate(build(torch.float64), fam, c, x.double(), eps.double(), dec.double(), lp_eps.double(), "_f64", fx)
    nparts, total = save_split(name, fx)
    print(f"{name}: {nparts} file(s), {total} bytes, loss {float(fx['b1/loss']):.6f} (fp64 {float(fx['b1/loss_f64']):.6f}), "
          f"kld {float(fx['b1/kld_f64']):.6f}, logprob {float(fx['lp/value_f64']):.6f}"
          + (f", lv0 in [{fx['lv0_f64'].min():.3f}, {fx['lv0_f64'].max():.3f}]" if nd else ""))


def gen_traj(net, rutils, fam, name, c):
    """vae.py:396-417: beta from annealing_func on the zero-based i_ep, forward, loss / D, backward, the vendored Adam."""
    B, D, nd, z, seed = c["B"], c["D"], c["noise"], c["z"], c["seed"]
    t = fam.get("traj_cfg", TRAJ_CFG)
    params, build = builder(net, fam, c)
    model, m64 = build(torch.float32), build(torch.float64)
    fx = {"cfg/" + k: np.array(v) for k, v in t.items()}
    fx.update(header(fam, c, params))
    fx.update(stored_params(fam, params))
    g = torch.Generator().manual_seed(seed + 1)
    adam = lambda m: rutils.Adam(m.parameters(), lr=t["lr"], betas=(t["beta1"], 0.999))      # noqa: E731
    runs = [(model, adam(model), torch.float32, ""), (m64, adam(m64), torch.float64, "_f64")]
    for i_ep in range(t["steps"]):
        beta = rutils.annealing_func(t["beta_init"], t["beta_fin"], t["beta_annealing"], i_ep)
        xb, eps = synth_x(fam, B, D, g), torch.randn(B, nd + z, generator=g)
        pre = f"{i_ep}/"
        fx[pre + "x"], fx[pre + "eps"], fx[pre + "beta"] = xb.numpy(), eps.numpy(), np.array(beta, dtype=np.float64)
        for m, opt, dtype, tag in runs:
            opt.zero_grad()
            with injected_draws(normals=draws(fam, nd, eps)["normals"]):
                _, _, _, loss, recon, kld = m(xb.to(dtype), beta=beta)
            (loss * (1. / float(D))).backward()
            opt.step()
            fx[pre + "loss" + tag], fx[pre + "recon" + tag], fx[pre + "kld" + tag] = loss.detach().numpy(), recon.numpy(), kld.numpy()
            for k, v in m.state_dict().items():
                if fam.get("full"):
                    fx[f"{pre}p{tag}/{k}"] = v.numpy().copy()
                else:
                    fx[f"{pre}ps{tag}/{k}"] = summary(v)
    nparts, total = save_split(name, fx)
    print(f"{name}: {nparts} file(s), {total} bytes, losses {[round(float(fx[f'{s}/loss']), 5) for s in range(t['steps'])]}")


def main():
    chosen, only, net, rutils = open_reference(FAMILIES, ["cases", "traj", "counts"])
    if only in (None, "counts"):
        # (a counts file may hold several families: it is written whole)
        for name in dict.fromkeys(FAMILIES[f]["counts_file"] for f in chosen):
            fx = {k: np.array(sum(p.numel() for p in getattr(net, fam["ctor"])(**kw).parameters()))
                  for fam in FAMILIES.values() if fam["counts_file"] == name for k, kw in fam["counts"].items()}
            print(f"{name}:", save_split(name, fx), {k: int(v) for k, v in fx.items()})
    for f in chosen:
        fam = FAMILIES[f]
        if only in (None, "cases"):
            for name, values in fam["cases"].items():
                gen_case(net, fam, name, case_of(fam, values))
        if only in (None, "traj"):
            gen_traj(net, rutils, fam, "vae_traj_" + f, case_of(fam, fam["traj"]))


if __name__ == "__main__":
    main()
