"""Time the reconstruction DAEs (net.MLPDAE / net.MLPCDAE, models/dae/mlp.py) on the device  --  reported, not gated.

    python tools/time_recon_dae.py [--steps 30] [--engine-steps 200] [--repeats 3] [--rounds 3] [--out profiles/recon_dae_timing.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_recon_dae.py --trace-steps 50      (a run of its own: the kind-13 step alone)
    python tools/time_recon_dae.py --merge-trace DIR                                                (its per-kernel split into the JSON)

1. `MLPDAE` at notebooks/dae_toy.ipynb's shape (B 256 x num_sigma 10 = 2560 rows, d 2, h 128, 3 layers, softplus), both noise types, milliseconds per
   update through four routes alternated in one process: `ArdaeScoreEngine.step` replayed, the same engine eager (graph=False), the drop-in module
   with `torch.optim.Adam`, and a plain PyTorch autograd loop of the same network.
2. `MLPCDAE` at the cDAE shape of BASELINE config #2 (B 512 x S 256, z 32, c 32, h 256, 3 layers), enc_input False (kind 13) and True (kind 11's
   network), against kind 11's own engine step (`MLPResCDAE`) on the same rows: `ArdaeCondScoreEngine.step` replayed.  `kind13_vs_kind11` records
   whether kind 13's median is above kind 11's by more than the spread between repeats of the same route.
3. The draw + perturb kernel against the stand-alone draw plus the unfused perturbation at both shapes, as launches and inside the replayed step.
   `draw_form_decision` records the rule: the draw form is the engines' default only if its median is not above the two launches' at every shape.
Device events around `steps` calls, everything warmed, median [min .. max] over rounds x repeats.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ardae_amd as net  # noqa: E402
from ardae_amd import _lib as L  # noqa: E402

TOY = dict(B=256, ns=10, d=2, h=128, nl=3)
CFG2 = dict(B=512, S=256, z=32, c=32, h=256, nl=3)
SIGMA = (5.0, 0.05, 4000)
STD_SCALE, LR = 100.0, 5e-3
OUT = os.path.join(ROOT, "profiles", "recon_dae_timing.json")


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


def mlpdae(noise):
    return net.MLPDAE(input_dim=TOY["d"], h_dim=TOY["h"], num_hidden_layers=TOY["nl"], nonlinearity="softplus", noise_type=noise).cuda()


def cond_module(which, noise="gaussian"):
    """x: MLPCDAE(enc_input=False) = kind 13; a: MLPCDAE(enc_input=True) = kind 11's network; kind11: MLPResCDAE"""
    kw = dict(input_dim=CFG2["z"], context_dim=CFG2["c"], h_dim=CFG2["h"], num_hidden_layers=CFG2["nl"], nonlinearity="softplus")
    if which == "kind11":
        return net.MLPResCDAE(**kw).cuda()
    return net.MLPCDAE(enc_input=which == "a", noise_type=noise, **kw).cuda()


def cond_engine(which, noise="gaussian", **kw):
    return net.ArdaeCondScoreEngine(cond_module(which, noise), net.DaeConfig(*SIGMA, nsigma=1, lr=LR), CFG2["B"], CFG2["S"], std_scale=STD_SCALE, **kw)


class TorchDAE(torch.nn.Module):
    """The reconstruction DAE as the reference writes it, under autograd"""

    def __init__(self, noise):
        super().__init__()
        layers, w = [], TOY["d"]
        for _ in range(TOY["nl"]):
            layers += [torch.nn.Linear(w, TOY["h"]), torch.nn.Softplus()]
            w = TOY["h"]
        self.main, self.noise = torch.nn.Sequential(*layers, torch.nn.Linear(w, TOY["d"])), noise

    def forward(self, x, std):
        xbar = x + std * torch.randn_like(x) if self.noise == "gaussian" else x + (2. * std * torch.rand_like(x) - std)
        return torch.nn.functional.mse_loss(self.main(xbar), x)


def toy_loop(forward, opt, x):
    """The training cell of notebooks/dae_toy.ipynb around a forward: the noise level on the host, broadcast, backward, optimiser."""
    it = [0]

    def step():
        opt.zero_grad()
        rows = x.unsqueeze(1).expand(TOY["B"], TOY["ns"], TOY["d"]).contiguous().view(-1, TOY["d"])
        forward(rows, net.dae_sigma(*SIGMA, it[0])).backward()
        opt.step()
        it[0] += 1
    return step


def trace_run(steps):
    """The kind-13 step alone, for a profiler run of its own"""
    B, S, z, c = CFG2["B"], CFG2["S"], CFG2["z"], CFG2["c"]
    mean = torch.randn(B, z, device="cuda")
    latent, ctx = (mean[:, None, :] + 0.01 * torch.randn(B, S, z, device="cuda")).contiguous(), torch.randn(B, c, device="cuda")
    eng = cond_engine("x", graph=False)
    for _ in range(steps):
        eng.step(latent, ctx, mean)
    torch.cuda.synchronize()
    print(f"{steps} kind-13 steps, last loss {eng.stats()['loss']:.5f}")


def merge_trace(directory, out):
    """rocprofv3 --kernel-trace --stats: the per-kernel split of the traced kind-13 steps into the JSON"""
    paths = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    dbs = sorted(glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True))
    if paths:
        with open(paths[-1]) as f:
            rows = list(csv.DictReader(f))
    elif dbs:                                   # the profiler's database output: its `kernels` view holds every dispatch with start and end in ns
        import sqlite3
        with sqlite3.connect(dbs[-1]) as db:
            rows = [{"Name": n, "Calls": c, "TotalDurationNs": t} for n, c, t in db.execute('select name, count(*), sum("end" - start) from kernels group by name')]
    else:
        raise SystemExit(f"no *kernel_stats.csv or *_results.db under {directory}")
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    split = [{"kernel": r["Name"], "calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6, "share": float(r["TotalDurationNs"]) / total}
             for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))]
    with open(out) as f:
        res = json.load(f)
    res["kind13_step_kernel_split"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own (eager steps at the config #2 shape)", "kernels": split}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    for k in split[:12]:
        print(f"{k['share']:.3f} {k['total_ms']:.3f} ms {k['calls']} x {k['kernel'][:100]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--engine-steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--merge-trace")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.merge_trace:
        return merge_trace(a.merge_trace, a.out)
    if a.trace_steps:
        return trace_run(a.trace_steps)
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "engine_steps": a.engine_steps, "repeats": a.repeats, "rounds": a.rounds, "unit": "ms",
           "mlpdae_dae_toy": {}, "mlpcdae_config2": {}, "perturbation": {}}

    def measure(routes, steps):
        samples = {k: [] for k in routes}
        for k, fn in routes.items():            # one untimed window per route
            timed_all(fn, steps[k], 1)
        for _ in range(a.rounds):               # alternate the routes
            for k, fn in routes.items():
                samples[k] += timed_all(fn, steps[k], a.repeats)
        return {k: spread(v) for k, v in samples.items()}

    show = lambda row: ", ".join(f"{k} {v['median']:.4f} [{v['min']:.4f} .. {v['max']:.4f}]" for k, v in row.items() if isinstance(v, dict))
    engine_steps = lambda routes: {k: a.engine_steps if k.startswith("engine") or k in ("two_launches", "draw_form") else a.steps for k in routes}

    # 1. MLPDAE at the dae_toy shape
    B, ns, d = TOY["B"], TOY["ns"], TOY["d"]
    x = 0.5 * torch.randn(B, d, device="cuda")
    cfg = net.DaeConfig(*SIGMA, nsigma=ns, lr=LR)
    for noise in ("gaussian", "uniform"):
        replayed, eager = net.ArdaeScoreEngine(mlpdae(noise), cfg, B), net.ArdaeScoreEngine(mlpdae(noise), cfg, B, graph=False)
        m, tm = mlpdae(noise), TorchDAE(noise).cuda()
        routes = {"engine_replayed": lambda: replayed.step(x), "engine_eager": lambda: eager.step(x),
                  "module_torch_adam": toy_loop(lambda rows, s: m(rows, s)[1], torch.optim.Adam(m.parameters(), lr=LR), x),
                  "torch_autograd": toy_loop(tm, torch.optim.Adam(tm.parameters(), lr=LR), x)}
        row = {"rows": B * ns, "d": d, "h": TOY["h"], "layers": TOY["nl"], "noise": noise, "draw_form": bool(replayed.draw_form)}
        row.update(measure(routes, engine_steps(routes)))
        res["mlpdae_dae_toy"][noise] = row
        print(f"mlpdae/{noise}: " + show(row), flush=True)

    # 2. MLPCDAE at config #2's cDAE shape against kind 11's engine step on the same rows
    Bc, S, z, c = CFG2["B"], CFG2["S"], CFG2["z"], CFG2["c"]
    mean = torch.randn(Bc, z, device="cuda")
    latent, ctx = (mean[:, None, :] + 0.01 * torch.randn(Bc, S, z, device="cuda")).contiguous(), torch.randn(Bc, c, device="cuda")
    engines = {"engine_replayed_mlpcdae_x_kind13": cond_engine("x"), "engine_replayed_mlpcdae_a_kind11": cond_engine("a"),
               "engine_replayed_mlprescdae_kind11": cond_engine("kind11"), "engine_replayed_mlpcdae_x_kind13_uniform": cond_engine("x", "uniform")}
    routes = {k: (lambda e=e: e.step(latent, ctx, mean)) for k, e in engines.items()}
    row = {"B": Bc, "S": S, "rows": Bc * S, "z": z, "c": c, "h": CFG2["h"], "layers": CFG2["nl"]}
    row.update(measure(routes, engine_steps(routes)))
    res["mlpcdae_config2"] = row
    print("mlpcdae/config2: " + show(row), flush=True)
    k13, k11 = row["engine_replayed_mlpcdae_x_kind13"], row["engine_replayed_mlprescdae_kind11"]
    noise_band = max(v["max"] - v["min"] for v in (k13, k11))
    res["kind13_vs_kind11"] = {"rule": "kind 13 runs a subset of kind 11's layers: its median must not exceed kind 11's by more than the spread between repeats of one route",
                               "kind13_median": k13["median"], "kind11_median": k11["median"], "spread_between_repeats": noise_band,
                               "kind13_slower_beyond_spread": bool(k13["median"] - k11["median"] > noise_band)}

    # 3. the draw form against its two launches, at both shapes
    state = torch.zeros(4, dtype=torch.int64, device="cuda")
    L.call("ardae_dae_state_advance", state, 16, LR, 0.9, 0.999, *SIGMA)
    for noise_id, noise in enumerate(("gaussian", "uniform")):
        draw_fn = "ardae_philox_uniform_at" if noise_id else "ardae_philox_normal_at"
        N = B * ns
        xbar, sg, tg, eps = (torch.empty(s, device="cuda") for s in ((N, d), (N,), (N, d), (N, d)))

        def two(xbar=xbar, sg=sg, tg=tg, eps=eps, N=N, draw_fn=draw_fn, noise_id=noise_id):
            L.call(draw_fn, eps, N * d, 7, 1, state, 0)
            L.call("ardae_recon_perturb", x, eps, B, ns, d, noise_id, 0.0, state, xbar, sg, tg)
        draw = lambda xbar=xbar, sg=sg, tg=tg, eps=eps, noise_id=noise_id: L.call("ardae_recon_perturb_draw", x, B, ns, d, noise_id, 0.0, state, 7, 1, 0, xbar, sg, tg, eps)
        e_two, e_draw = net.ArdaeScoreEngine(mlpdae(noise), cfg, B, draw_form=False), net.ArdaeScoreEngine(mlpdae(noise), cfg, B, draw_form=True)
        routes = {"two_launches": two, "draw_form": draw, "engine_replayed_two_launches": lambda: e_two.step(x), "engine_replayed_draw_form": lambda: e_draw.step(x)}
        row = {"rows": N, "d": d}
        row.update(measure(routes, engine_steps(routes)))
        res["perturbation"][f"dae_toy/{noise}"] = row
        print(f"perturbation/dae_toy/{noise}: " + show(row), flush=True)

        N2 = Bc * S
        xbar2, sg2, tg2, eps2 = (torch.empty(s, device="cuda") for s in ((N2, z), (N2,), (N2, z), (N2, z)))

        def two2(noise_id=noise_id, draw_fn=draw_fn, xbar2=xbar2, sg2=sg2, tg2=tg2, eps2=eps2):
            L.call(draw_fn, eps2, N2 * z, 7, 1, state, 0)
            L.call("ardae_latent_recon_perturb", latent, mean, eps2, Bc, S, 1, z, STD_SCALE, noise_id, 0.0, state, xbar2, sg2, tg2)
        draw2 = lambda noise_id=noise_id, xbar2=xbar2, sg2=sg2, tg2=tg2, eps2=eps2: L.call(
            "ardae_latent_recon_perturb_draw", latent, mean, Bc, S, 1, z, STD_SCALE, noise_id, 0.0, state, 7, 1, 0, xbar2, sg2, tg2, eps2)
        c_two, c_draw = cond_engine("x", noise, draw_form=False), cond_engine("x", noise, draw_form=True)
        assert c_draw.draw_form and not c_two.draw_form
        routes = {"two_launches": two2, "draw_form": draw2, "engine_replayed_two_launches": lambda: c_two.step(latent, ctx, mean),
                  "engine_replayed_draw_form": lambda: c_draw.step(latent, ctx, mean)}
        row = {"rows": N2, "z": z}
        row.update(measure(routes, engine_steps(routes)))
        res["perturbation"][f"config2/{noise}"] = row
        print(f"perturbation/config2/{noise}: " + show(row), flush=True)
        del c_two, c_draw
    above = [k for k, v in res["perturbation"].items() if v["draw_form"]["median"] > v["two_launches"]["median"]]
    res["draw_form_decision"] = {"rule": "default only if the draw form's median is not above the two launches' at every measured shape",
                                 "draw_form_above_two_launches_at": above, "draw_form_is_default": not above,
                                 "engine_defaults": {"ArdaeScoreEngine": bool(net.ArdaeScoreEngine.RECON_DRAW_FORM_DEFAULT),
                                                     "ArdaeCondScoreEngine": bool(net.ArdaeCondScoreEngine.RECON_DRAW_FORM_DEFAULT)}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["kind13_vs_kind11"]))
    print(json.dumps(res["draw_form_decision"]))


if __name__ == "__main__":
    main()
