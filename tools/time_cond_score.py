"""Time the conditional score update outside the VAE loop on the device  --  reported, not gated.

    python tools/time_cond_score.py [--steps 30] [--engine-steps 200] [--repeats 3] [--rounds 3] [--out profiles/cond_score_timing.json]

Shapes (B contexts x S samples, z, context width, h, layers; softplus, nsigma 1): the cDAE update of BASELINE config #2 (512 x 256, z 32, h 256,
3 layers), its 64-image shard, and a toy shape (z 2).  Per shape and for kinds 0 (`net.MLPGradCARDAE`, ScoreConfig, the vendored Adam) and 10
(`net.MLPGradCDAE`, DaeConfig, torch.optim.Adam's arithmetic), milliseconds per update through four routes, alternated in one process:
`ArdaeCondScoreEngine.step` replayed, the same engine eager (graph=False), the drop-in module with `net.Adam` (centring, statistics and noise
levels in torch), and a plain PyTorch autograd restatement of the network with `torch.optim.Adam`.  And the plain kinds' perturbation: the
draw form `ardae_latent_noise_perturb_draw` against its two launches `ardae_philox_normal_at` + `ardae_latent_noise_perturb`, as launches and
inside the replayed engine step.  Device events around `steps` calls, everything warmed, median [min .. max] over rounds x repeats.
`draw_form_decision` records the rule: the draw form is the engine's default only if its median is not above the two launches' at every shape.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ardae_amd as net  # noqa: E402
from ardae_amd import _lib as L  # noqa: E402

SHAPES = {"config2_cdae_update": (512, 256, 32, 32, 256, 3), "config2_64image_shard": (64, 256, 32, 32, 256, 3), "toy_z2": (256, 16, 2, 2, 128, 3)}
SIGMA = (5.0, 0.05, 4000)
DELTA, STD_SCALE, LR = 0.1, 100.0, 1e-4


def timed_all(fn, steps, repeats, warmup=10):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / steps)
    return out


def spread(samples):
    return {"median": statistics.median(samples), "min": min(samples), "max": max(samples), "samples": samples}


def module(plain, z, c, h, nl):
    cls = net.MLPGradCDAE if plain else net.MLPGradCARDAE
    return cls(input_dim=z, context_dim=c, h_dim=h, num_hidden_layers=nl, nonlinearity="softplus").cuda()


def engine(plain, B, S, z, c, h, nl, graph=True, draw_form=None):
    cfg = net.DaeConfig(*SIGMA, nsigma=1, lr=LR) if plain else net.ScoreConfig(delta=DELTA, nsigma=1, lr=LR, optimizer="adam")
    kw = {"draw_form": draw_form} if plain else {}
    return net.ArdaeCondScoreEngine(module(plain, z, c, h, nl), cfg, B, S, std_scale=STD_SCALE, graph=graph, **kw)


class TorchCDAE(torch.nn.Module):
    """The conditional energy network as the reference writes it (two encoders, an MLP on their concatenation [and sigma]) under autograd."""

    def __init__(self, plain, z, c, h, nl):
        super().__init__()
        def mlp(din, dout, n, act_out):
            layers, w = [], din
            for _ in range(n):
                layers += [torch.nn.Linear(w, h), torch.nn.Softplus()]
                w = h
            return torch.nn.Sequential(*layers, torch.nn.Linear(w, dout), *([torch.nn.Softplus()] if act_out else []))
        self.plain = plain
        self.ctx_encode, self.inp_encode = mlp(c, h, nl - 1, True), mlp(z, h, nl - 1, True)
        self.neglogprob = mlp(2 * h + (0 if plain else 1), 1, nl, False)

    def forward(self, u, ctx, std):
        """u [B, S, z], ctx [B, c], std: a float or [B, S, 1]"""
        B, S, z = u.shape
        eps = torch.randn(B * S, z, device=u.device)
        std = std.reshape(B * S, 1) if torch.is_tensor(std) else std
        xbar = (u.reshape(B * S, z) + std * eps).requires_grad_(True)
        hdn = [self.inp_encode(xbar), self.ctx_encode(ctx).repeat_interleave(S, 0)] + ([] if self.plain else [std])
        g = torch.autograd.grad(-self.neglogprob(torch.cat(hdn, 1)).sum(), xbar, create_graph=True)[0]
        return torch.nn.functional.mse_loss(std * g, -eps)


def loop(plain, forward, opt, latent, ctx, mean):
    """ivae_ardae.py:752-779 around a forward: centre and scale, the noise level(s) on the host / in torch, backward, optimiser."""
    it = [0]

    def step():
        opt.zero_grad()
        u = STD_SCALE * (latent - mean[:, None, :])
        if plain:
            std = net.dae_sigma(*SIGMA, it[0])
        else:
            std = DELTA * u.std(dim=1, keepdim=True).mean(dim=2, keepdim=True) * torch.randn(u.size(0), u.size(1), 1, device=u.device)
        forward(u, ctx, std).backward()
        opt.step()
        it[0] += 1
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--engine-steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cond_score_timing.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "engine_steps": a.engine_steps, "repeats": a.repeats, "rounds": a.rounds, "unit": "ms",
           "shapes": {}, "perturbation": {}}

    def measure(routes, steps):
        samples = {k: [] for k in routes}
        for k, fn in routes.items():            # one untimed window per route
            timed_all(fn, steps[k], 1)
        for _ in range(a.rounds):               # alternate the routes
            for k, fn in routes.items():
                samples[k] += timed_all(fn, steps[k], a.repeats)
        return {k: spread(v) for k, v in samples.items()}

    show = lambda row: ", ".join(f"{k} {v['median']:.4f} [{v['min']:.4f} .. {v['max']:.4f}]" for k, v in row.items() if isinstance(v, dict))
    for name, (B, S, z, c, h, nl) in SHAPES.items():
        mean = torch.randn(B, z, device="cuda")
        latent = (mean[:, None, :] + 0.01 * torch.randn(B, S, z, device="cuda")).contiguous()
        ctx = torch.randn(B, c, device="cuda")
        for plain in (False, True):
            replayed, eager = engine(plain, B, S, z, c, h, nl), engine(plain, B, S, z, c, h, nl, graph=False)
            m, tm = module(plain, z, c, h, nl), TorchCDAE(plain, z, c, h, nl).cuda()
            routes = {"engine_replayed": lambda: replayed.step(latent, ctx, mean), "engine_eager": lambda: eager.step(latent, ctx, mean),
                      "module_net_adam": loop(plain, lambda u, cc, s: m(u, cc.view(B, 1, c), s)[1], net.Adam(m.parameters(), lr=LR, betas=(0.5, 0.999)), latent, ctx, mean),
                      "torch_autograd": loop(plain, tm, torch.optim.Adam(tm.parameters(), lr=LR, betas=(0.5, 0.999)), latent, ctx, mean)}
            row = {"B": B, "S": S, "rows": B * S, "z": z, "c": c, "h": h, "layers": nl, "kind": 10 if plain else 0}
            if not plain:
                row["front_end"] = "first_layer" if replayed.fused_first else "draw" if replayed.fused_draw else "unfused"
            row.update(measure(routes, {k: a.engine_steps if k.startswith("engine") else a.steps for k in routes}))
            res["shapes"][f"{name}/kind{row['kind']}"] = row
            print(f"{name}/kind{row['kind']}: " + show(row), flush=True)
        # the plain kinds' perturbation: the draw form against its two launches
        N = B * S
        xbar, sg, eps = (torch.empty(s, device="cuda") for s in ((N, z), (N,), (N, z)))
        state = torch.zeros(4, dtype=torch.int64, device="cuda")
        L.call("ardae_dae_state_advance", state, 16, LR, 0.9, 0.999, *SIGMA)

        def two():
            L.call("ardae_philox_normal_at", eps, N * z, 7, 1, state, 0)
            L.call("ardae_latent_noise_perturb", latent, mean, eps, B, S, 1, z, STD_SCALE, 0.0, state, xbar, sg)
        draw = lambda: L.call("ardae_latent_noise_perturb_draw", latent, mean, B, S, 1, z, STD_SCALE, 0.0, state, 7, 1, 0, xbar, sg, eps)
        e_two, e_draw = engine(True, B, S, z, c, h, nl, draw_form=False), engine(True, B, S, z, c, h, nl, draw_form=True)
        assert e_draw.draw_form and not e_two.draw_form
        routes = {"two_launches": two, "draw_form": draw, "engine_replayed_two_launches": lambda: e_two.step(latent, ctx, mean),
                  "engine_replayed_draw_form": lambda: e_draw.step(latent, ctx, mean)}
        row = {"rows": N, "z": z}
        row.update(measure(routes, {k: a.engine_steps for k in routes}))
        res["perturbation"][name] = row
        print(f"{name}/perturbation: " + show(row), flush=True)
    above = [k for k, v in res["perturbation"].items() if v["draw_form"]["median"] > v["two_launches"]["median"]]
    res["draw_form_decision"] = {"rule": "default only if the draw form's median is not above the two launches' at every measured shape",
                                 "draw_form_above_two_launches_at": above, "draw_form_is_default": not above,
                                 "engine_default": bool(net.ArdaeCondScoreEngine.DRAW_FORM_DEFAULT)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["draw_form_decision"]))


if __name__ == "__main__":
    main()
