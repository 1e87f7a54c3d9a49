"""Time the AR-DAE half of the two notebook loops on the device  --  reported, not gated.

    python tools/time_ardae_fit.py [--steps 200] [--repeats 5] [--out profiles/ardae_uncond_timing.json]

Per notebook shape (ardae_toy.ipynb: 256 x 10 rows, h 128; ardae_fit.ipynb: 1024 x 10 rows, h 256; d 2, 3 hidden layers, softplus) and
kind: milliseconds per `ArdaeScoreEngine.step` with the fused front end (draw + perturbation + first layer in one kernel) and with the
unfused one (two draws, scale, perturbation, first layer as launches of their own), alternated in one process; per `score()` on the
batch; and per step of a plain PyTorch autograd loop of the same network on the same device (the notebooks' own code path: broadcast,
randn, double backward through autograd, torch.optim.RMSprop).  Device events around `steps` calls, median of `repeats`.
The WHOLE iteration of ardae_fit.ipynb at the notebook's shape (batch 1024 x 10 sigma levels, z_dim 10, generator and score network three
256-wide hidden layers, two AR-DAE updates per generator update) is timed three ways, alternated in one process: `ArdaeFitEngine` with
the fused generator front end (draw + first layer in one kernel), the same engine without it, and the route a caller had before that
engine existed - a torch generator under autograd with torch.optim.Adam, `ArdaeScoreEngine.step` for the AR-DAE updates and
`engine.score` for the entropy gradient - on the same device.  Medians and spreads (min .. max over rounds x repeats) are recorded.
A path that did not exist has no earlier time to compare with; the 28 ms per iteration in ardae_fit.ipynb's own log is another GPU,
another stack and a whole iteration (two AR-DAE updates, the sampler's update), and is not a baseline for these numbers.
`--profile-kernels`: runs only a few fused steps at the large shape (for a kernel trace run of its own).
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

SHAPES = {"ardae_toy": (256, 10, 2, 128, 3), "ardae_fit": (1024, 10, 2, 256, 3)}


def timed(fn, steps, repeats, warmup=20):
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
    return statistics.median(out)


class TorchARDAE(torch.nn.Module):
    """The network as the notebooks write it (nn.Sequential on [x_bar | sigma]) for the plain-autograd column."""

    def __init__(self, kind, d, h, nl):
        super().__init__()
        layers, w = [], d + 1
        for _ in range(nl):
            layers += [torch.nn.Linear(w, h), torch.nn.Softplus()]
            w = h
        self.kind, self.main = kind, torch.nn.Sequential(*layers, torch.nn.Linear(h, 1 if kind == "grad" else d))

    def forward(self, x, std):
        eps = torch.randn_like(x)
        xbar = x + std * eps
        if self.kind == "grad":
            xbar.requires_grad = True
            g = torch.autograd.grad(-self.main(torch.cat([xbar, std], 1)).sum(), xbar, create_graph=True)[0]
        else:
            g = self.main(torch.cat([xbar, std], 1))
        return torch.nn.functional.mse_loss(std * g, -eps)


def engine(kind, B, ns, d, h, nl, fused):
    m = (net.MLPGradARDAE if kind == "grad" else net.MLPResARDAE)(input_dim=d, h_dim=h, num_hidden_layers=nl, nonlinearity="softplus").cuda()
    eng = net.ArdaeScoreEngine(m, net.ScoreConfig(delta=1.0, nsigma=ns, lr=1e-3, optimizer="rmsprop"), B)
    assert eng.fused_front, "the notebook shapes must qualify for the fused front end"
    eng.fused_front = fused
    return eng


FIT_SHAPE = dict(B=1024, nsigma=10, d=2, z_dim=10, h=256, layers=3)


def spread(samples):
    return {"median": statistics.median(samples), "min": min(samples), "max": max(samples), "samples": samples}


def timed_all(fn, steps, repeats, warmup=20):
    """Like timed(), but every repeat's figure."""
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


def fit_engine(kind, fused):
    c = FIT_SHAPE
    gen = net.Generator(input_dim=c["d"], hidden_dim=c["h"], z_dim=c["z_dim"], num_hidden_layers=c["layers"], nonlinearity="relu").cuda()
    dae = (net.MLPGradARDAE if kind == "grad" else net.MLPResARDAE)(input_dim=c["d"], h_dim=c["h"], num_hidden_layers=c["layers"], nonlinearity="softplus").cuda()
    eng = net.ArdaeFitEngine(gen, dae, net.FitConfig(nsigma=c["nsigma"]), c["B"])
    assert eng.fused_front and eng.score.fused_front, "the notebook's shape must qualify for both fused front ends"
    eng.fused_front = fused
    return eng


def torch_route(kind):
    """INTEGRATION.md section 2a before the fit engine: a torch generator (autograd, torch.optim.Adam, the notebook's StepLR and annealing on the
    host), ArdaeScoreEngine for the AR-DAE updates, engine.score for the entropy gradient."""
    c = FIT_SHAPE
    B, d = c["B"], c["d"]
    layers, w = [], c["z_dim"]
    for _ in range(c["layers"]):
        layers += [torch.nn.Linear(w, c["h"]), torch.nn.ReLU()]
        w = c["h"]
    gen = torch.nn.Sequential(*layers, torch.nn.Linear(c["h"], d)).cuda()
    opt = torch.optim.Adam(gen.parameters(), lr=1e-3, betas=(0.5, 0.999))
    dae = (net.MLPGradARDAE if kind == "grad" else net.MLPResARDAE)(input_dim=d, h_dim=c["h"], num_hidden_layers=c["layers"], nonlinearity="softplus").cuda()
    eng = net.ArdaeScoreEngine(dae, net.ScoreConfig(delta=0.1, nsigma=c["nsigma"], lr=1e-3, optimizer="rmsprop"), B)
    cfg, it = net.FitConfig(), [0]
    from ardae_amd import fit

    def step():
        alpha = fit.alpha_at(cfg, it[0])
        for _ in range(2):
            with torch.no_grad():
                x = gen(torch.randn(B, c["z_dim"], device="cuda"))
            eng.step(x)
        opt.zero_grad()
        out = gen(torch.randn(B, c["z_dim"], device="cuda"))
        loss = torch.mean(net.energy.energy_func4(out))
        (0 + alpha * loss).backward(retain_graph=True)
        out.backward(eng.score(out.detach()) / float(B))
        opt.step()
        it[0] += 1
        opt.param_groups[0]["lr"] = fit.step_lr(cfg, it[0])
    return step


def time_fit_iteration(a):
    out = {"shape": FIT_SHAPE, "updates_per_iteration": 2}
    for kind in ("grad", "res"):
        ef, eu, tr = fit_engine(kind, True), fit_engine(kind, False), torch_route(kind)
        rounds = {"fit_engine_fused_front": [], "fit_engine_unfused_front": [], "torch_generator_plus_score_engine": []}
        for _ in range(3):              # alternate the three routes
            rounds["fit_engine_fused_front"] += timed_all(ef.step, a.steps, a.repeats)
            rounds["fit_engine_unfused_front"] += timed_all(eu.step, a.steps, a.repeats)
            rounds["torch_generator_plus_score_engine"] += timed_all(tr, a.steps, a.repeats)
        out[kind] = {k: spread(v) for k, v in rounds.items()}
    return out


def time_dae_front(a):
    """The open question of DESIGN.md section 6: ArdaeScoreEngine.step with dae_perturb_fwd_kernel and without, with spreads."""
    out = {}
    B, ns, d, h, nl = SHAPES["ardae_fit"]
    for kind in ("grad", "res"):
        x = torch.randn(B, d, device="cuda")
        ef, eu = engine(kind, B, ns, d, h, nl, True), engine(kind, B, ns, d, h, nl, False)
        f, u = [], []
        for _ in range(3):
            f += timed_all(lambda: ef.step(x), a.steps, a.repeats)
            u += timed_all(lambda: eu.step(x), a.steps, a.repeats)
        out[kind] = {"step_fused": spread(f), "step_unfused": spread(u)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ardae_uncond_timing.json"))
    ap.add_argument("--profile-kernels", action="store_true")
    ap.add_argument("--only-iteration", action="store_true", help="time only the whole fit iteration and the front-end question; keep the file's other entries")
    a = ap.parse_args()
    if a.profile_kernels:
        B, ns, d, h, nl = SHAPES["ardae_fit"]
        eng = engine("grad", B, ns, d, h, nl, True)
        eng.use_graph = False
        x = torch.randn(B, d, device="cuda")
        for _ in range(50):
            eng.step(x)
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "repeats": a.repeats, "unit": "ms", "shapes": {}}
    if a.only_iteration and os.path.exists(a.out):
        with open(a.out) as f:
            res = dict(json.load(f), steps_iteration=a.steps, repeats_iteration=a.repeats)

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    res["fit_iteration"] = time_fit_iteration(a)
    save()
    res["dae_front_end"] = time_dae_front(a)
    save()
    for name, (B, ns, d, h, nl) in ([] if a.only_iteration else SHAPES.items()):
        for kind in ("grad", "res"):
            x = torch.randn(B, d, device="cuda")
            ef, eu = engine(kind, B, ns, d, h, nl, True), engine(kind, B, ns, d, h, nl, False)
            row = {"rows": B * ns, "d": d, "h": h, "layers": nl}
            # alternate the two front ends: two rounds each, the better median of each is kept
            f1, u1 = timed(lambda: ef.step(x), a.steps, a.repeats), timed(lambda: eu.step(x), a.steps, a.repeats)
            f2, u2 = timed(lambda: ef.step(x), a.steps, a.repeats), timed(lambda: eu.step(x), a.steps, a.repeats)
            row["step_fused"], row["step_unfused"] = min(f1, f2), min(u1, u2)
            row["step_fused_rounds"], row["step_unfused_rounds"] = [f1, f2], [u1, u2]
            row["score"] = timed(lambda: ef.score(x), a.steps, a.repeats)
            tm = TorchARDAE(kind, d, h, nl).cuda()
            opt = torch.optim.RMSprop(tm.parameters(), lr=1e-3, momentum=0.5)

            def torch_step():
                opt.zero_grad()
                sigma = torch.randn(B * ns, 1, device="cuda")
                rows = x.unsqueeze(1).expand(B, ns, d).contiguous().view(B * ns, d)
                tm(rows, sigma).backward()
                opt.step()
            row["step_torch_autograd"] = timed(torch_step, a.steps, a.repeats)
            res["shapes"][f"{name}/{kind}"] = row
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
