"""Golden vectors of the energy-function fit (notebooks/ardae_fit.ipynb)  --  TEST INFRASTRUCTURE.

Runs only where the reference checkout is available (it never travels to the GPU box):

    python tools/gen_fit_golden.py [--reference DIR] [--only energy|traj|quality]

It imports the reference's own utils/energy.py, utils/lr_scheduler.py::StepLR, utils/msc.py::annealing_func and score-network classes
(models.MLPGradARDAE / MLPResARDAE) and stores THEIR outputs; the loop of the notebook is written here as plain torch.

  tests/golden/fit_energy.npz     x [4096 + K, 2]: uniform points in [-8, 8]^2 and hand-picked ones (origin, |x_i| = 6 exactly, beyond 6 on
      both axes, the modes, far tails); per function `energy_func1..4` and `regularization_func`: e64 / g64 (energies, autograd
      gradients in float64 at x.double()) and e32 / g32 (the same calls in float32); `normal_energy_func` on xn [4096, 3] with mu / logvar.
  tests/golden/fit_traj_<case>.npz   6 iterations of the notebook's loop on injected draws, in fp32:
      cfg/<key>                      the case and its schedule (CASES, SCHEDULE below)
      sd_gen/<name>, sd_dae/<name>   initial state_dicts
      z [6, U + 1, B, z_dim], sigma [6, U, B * nsigma] (= delta * randn), eps [6, U, B * nsigma, d]
      model_loss, dae_loss, alpha, lr [6]; <i>/gen/<name>, <i>/dae/<name>: every parameter after iteration i
  tests/golden/fit_traj_<case>_f64.npz   the same run in float64 from the same state and draws: the scalars in float64, the parameters
      rounded to fp32 once (a file of float64 parameters would exceed the size limit of a committed file)
  tests/golden/fit_quality.npz    8 seeds of a short fit (own draws): mean energy and per-axis standard deviation of 4096 final samples,
      and the same statistics of the untrained generators.

Fixtures hold tensors, names and settings only.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from oracle import gen_golden as G  # noqa: E402
import gen_score_golden as A  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
ACTS = {"relu": nn.ReLU, "tanh": nn.Tanh, "softplus": nn.Softplus, "elu": nn.ELU}
ITERS = 6
# B, nsigma, z_dim, h, L, act, energy, dae kind, dae h, dae L; the schedules cross a boundary (lr at 2, 4) and the end of the annealing (4)
CASES = {"e4_res": dict(B=64, nsigma=4, z_dim=10, h=64, L=3, act="relu", energy=4, dae="res", dae_h=64, dae_L=3),
         "e1_grad": dict(B=40, nsigma=3, z_dim=3, h=100, L=2, act="tanh", energy=1, dae="grad", dae_h=100, dae_L=2)}
SCHEDULE = dict(U=2, delta=0.1, lr=1e-3, beta1=0.5, lr_step_size=2, lr_gamma=0.5, lr_min=1e-10, alpha_init=0.01, alpha_fin=1.0, alpha_annealing=4,
                d_momentum=0.5)
# energy_func1 (a ring with two modes): a compact target, so the seeds agree closely; on energy_func4's long ridge the trained seeds' mean
# energies spread by 0.14 - 0.17 and the gate below (trained vs untrained) stayed under 10 standard deviations at 800 and 1500 steps
QUALITY = dict(B=128, nsigma=10, z_dim=4, h=64, L=3, act="relu", energy=1, dae="res", dae_h=64, dae_L=3, steps=1000, U=2, delta=0.1, lr=1e-3,
               beta1=0.5, lr_step_size=400, lr_gamma=0.5, lr_min=1e-10, alpha_init=0.01, alpha_fin=1.0, alpha_annealing=400, d_momentum=0.5,
               seeds=list(range(8)), points=4096)
HAND_POINTS = [(0., 0.), (6., 6.), (-6., 6.), (6., -6.), (-6., -6.), (6., 0.), (0., -6.), (7.5, -7.25), (-7., 7.75), (6.5, 6.25), (-7.75, -6.5),
               (2., 0.), (-2., 0.), (0., 2.), (1., 1.), (3., -1.), (-1., -1.), (1., -2.), (0., 7.5), (0., -7.5), (4., 7.875), (-3., -7.)]


def generator(c):
    layers, w = [], c["z_dim"]
    for _ in range(c["L"]):
        layers += [nn.Linear(w, c["h"]), ACTS[c["act"]]()]
        w = c["h"]
    m = nn.Module()
    m.main = nn.Sequential(*layers, nn.Linear(c["h"], 2))
    return m


def fit_loop(net, ru, c, gen, dae, iters, noise=None, record=None):
    """The training cell of notebooks/ardae_fit.ipynb.  noise: {'z', 'sigma', 'eps'} injected draws (else torch.randn)."""
    B, ns, U, d = c["B"], c["nsigma"], c["U"], 2
    energy = getattr(ru, f"energy_func{c['energy']}")
    dt = next(gen.parameters()).dtype
    g_opt = torch.optim.Adam(gen.parameters(), lr=c["lr"], betas=(c["beta1"], 0.999))
    sched = ru.StepLR(g_opt, step_size=c["lr_step_size"], gamma=c["lr_gamma"], min_lr=c["lr_min"])
    d_opt = torch.optim.RMSprop(dae.parameters(), lr=c["lr"], momentum=c["d_momentum"])
    for i in range(iters):
        alpha = ru.annealing_func(c["alpha_init"], c["alpha_fin"], c["alpha_annealing"], i)
        for u in range(U):
            d_opt.zero_grad()
            z = noise["z"][i, u].to(dt) if noise else torch.randn(B, c["z_dim"], dtype=dt)
            out = gen.main(z)
            sigma = noise["sigma"][i, u].to(dt).view(-1, 1) if noise else c["delta"] * torch.randn(B * ns, 1, dtype=dt)
            rows = out.detach().unsqueeze(1).expand(B, ns, d).reshape(B * ns, d)
            if noise:
                with A.injected_draw(noise["eps"][i, u]):
                    _, dae_loss = dae(rows, std=sigma)
            else:
                _, dae_loss = dae(rows, std=sigma)
            dae_loss.backward()
            d_opt.step()
        g_opt.zero_grad()
        z = noise["z"][i, U].to(dt) if noise else torch.randn(B, c["z_dim"], dtype=dt)
        out = gen.main(z)
        model_loss = torch.mean(energy(out))
        (0 + alpha * model_loss).backward(retain_graph=True)
        grad = dae.glogprob(out.detach(), std=torch.zeros(B, 1, dtype=dt))
        out.backward(grad.detach() / float(B))
        lr = g_opt.param_groups[0]["lr"]
        g_opt.step()
        sched.step()
        if record is not None:
            record(i, float(model_loss.detach()), float(dae_loss.detach()), alpha, lr, gen, dae)


def gen_energy(ru):
    g = torch.Generator().manual_seed(20240)
    x = torch.cat([(torch.rand(4096, 2, generator=g) * 16 - 8), torch.tensor(HAND_POINTS)]).float()
    fx = {"x": x.numpy(), "n_uniform": np.array(4096)}
    funcs = {f"energy_func{k}": getattr(ru, f"energy_func{k}") for k in (1, 2, 3, 4)}
    funcs["regularization_func"] = ru.regularization_func
    xn = (2.0 * torch.randn(4096, 3, generator=g)).float()
    mu, logvar = 0.3, -0.7
    fx["xn"], fx["normal_mu"], fx["normal_logvar"] = xn.numpy(), np.array(mu), np.array(logvar)
    funcs["normal_energy_func"] = lambda t: ru.normal_energy_func(t, mu, logvar)
    for name, f in funcs.items():
        pts = xn if name == "normal_energy_func" else x
        for tag, dt in (("64", torch.float64), ("32", torch.float32)):
            p = pts.to(dt).requires_grad_(True)
            e = f(p)
            (gr,) = torch.autograd.grad(e.sum(), p)
            fx[f"{name}/e{tag}"], fx[f"{name}/g{tag}"] = e.detach().reshape(-1).numpy(), gr.numpy()
        g64, g32 = fx[f"{name}/g64"], fx[f"{name}/g32"].astype(np.float64)
        assert np.isfinite(g64).all() and np.isfinite(g32).all(), name
        print(f"{name}: fp32 gradient relL2 {np.linalg.norm(g32 - g64) / np.linalg.norm(g64):.2e}, worst element "
              f"{np.max(np.abs(g32 - g64) / np.maximum(1, np.abs(g64))):.2e} of max(1, |g|); origin gradient {g64[4096] if pts is x else None}")
    path = os.path.join(GOLDEN, "fit_energy.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes")


def gen_traj(net, ru, name, case, seed):
    c = dict(case, **SCHEDULE)
    B, ns, U, zd = c["B"], c["nsigma"], c["U"], c["z_dim"]
    torch.manual_seed(seed)
    gen = generator(c)
    dae = A.build(net, A.score_class(c["dae"], "ARDAE"), (c["B"], 2, c["dae_h"], c["dae_L"], "softplus"))
    sd_gen = {k: v.clone() for k, v in gen.state_dict().items()}
    sd_dae = {k: v.clone() for k, v in dae.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    noise = {"z": torch.randn(ITERS, U + 1, B, zd, generator=g), "sigma": c["delta"] * torch.randn(ITERS, U, B * ns, generator=g),
             "eps": torch.randn(ITERS, U, B * ns, 2, generator=g)}
    fx = {"cfg/" + k: np.array(v) for k, v in c.items()}
    fx.update({k: v.numpy() for k, v in noise.items()})
    for k, v in sd_gen.items():
        fx["sd_gen/" + k] = v.numpy().copy()
    for k, v in sd_dae.items():
        fx["sd_dae/" + k] = v.numpy().copy()
    for tag, dt in (("", torch.float32), ("_f64", torch.float64)):
        gen.load_state_dict(sd_gen); dae.load_state_dict(sd_dae)
        gen, dae = gen.to(dt), dae.to(dt)
        out = fx if not tag else {}
        rows = []

        def record(i, ml, dl, alpha, lr, gen_, dae_):
            rows.append((ml, dl, alpha, lr))
            for k, v in gen_.state_dict().items():
                out[f"{i}/gen/{k}"] = v.float().numpy().copy()
            for k, v in dae_.state_dict().items():
                out[f"{i}/dae/{k}"] = v.float().numpy().copy()
        fit_loop(net, ru, c, gen, dae, ITERS, noise, record)
        for j, key in enumerate(("model_loss", "dae_loss", "alpha", "lr")):
            out[key] = np.array([r[j] for r in rows])
        print(name, tag, "model_loss", out["model_loss"], "dae_loss", out["dae_loss"], "alpha", out["alpha"], "lr", out["lr"])
        gen, dae = gen.float(), dae.float()
        path = os.path.join(GOLDEN, f"fit_traj_{name}{tag}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")


def gen_quality(net, ru):
    q = QUALITY
    energy = getattr(ru, f"energy_func{q['energy']}")
    fx = {"cfg/" + k: np.array(v) for k, v in q.items()}

    def statistics(gen, seed):
        z = torch.randn(q["points"], q["z_dim"], generator=torch.Generator().manual_seed(9000 + seed))
        with torch.no_grad():
            x = gen.main(z)
            return [float(energy(x).mean())] + x.std(0).tolist()
    trained, untrained = [], []
    for seed in q["seeds"]:
        t0 = time.time()
        torch.manual_seed(3000 + seed)
        gen = generator(q)
        dae = A.build(net, A.score_class(q["dae"], "ARDAE"), (q["B"], 2, q["dae_h"], q["dae_L"], "softplus"))
        untrained.append(statistics(gen, seed))
        fit_loop(net, ru, q, gen, dae, q["steps"])
        trained.append(statistics(gen, seed))
        print(f"seed {seed}: untrained {untrained[-1]}, trained {trained[-1]}  ({time.time() - t0:.1f} s)", flush=True)
    fx["trained"], fx["untrained"] = np.array(trained), np.array(untrained)     # [seeds, 3]: mean energy, std of axis 0, std of axis 1
    t, u = fx["trained"][:, 0], fx["untrained"][:, 0]
    gap, spread = abs(t.mean() - u.mean()), max(t.std(ddof=1), u.std(ddof=1))
    print(f"mean energy: trained {t.mean():.4f} +- {t.std(ddof=1):.4f}, untrained {u.mean():.4f} +- {u.std(ddof=1):.4f}")
    assert gap > 10 * spread, "trained and untrained generators are not told apart by the mean energy: change the configuration"
    path = os.path.join(GOLDEN, "fit_quality.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=G.REF)
    ap.add_argument("--only", choices=["energy", "traj", "quality"])
    a = ap.parse_args()
    G.REF = a.reference
    net, ru = G.import_reference()
    torch.set_num_threads(8)
    if a.only in (None, "energy"):
        gen_energy(ru)
    if a.only in (None, "traj"):
        for i, (name, case) in enumerate(CASES.items()):
            gen_traj(net, ru, name, case, 500 + 10 * i)
    if a.only in (None, "quality"):
        gen_quality(net, ru)


if __name__ == "__main__":
    main()
