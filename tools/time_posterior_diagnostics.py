"""Time the posterior diagnostics (the loop's `''' visualize '''` block, ivae_ardae.py:952-1111) on the device against the loop it replaces.

    python tools/time_posterior_diagnostics.py [--images 20000] [--repeats 2] [--rounds 3] [--out profiles/posterior_diagnostics_timing.json]

Two cases, each over `images` synthetic images:
  25gaussians    the 25-Gaussians recipe's model (run_vae_25gaussians.sh: mlp-concat, 2-D data, noise 10, h 256 x 2, z 2, relu)
  mnist-concat   config #2's widths (784 pixels, noise 100, h 256 x 2, z 32, softplus)
Milliseconds per pass, two routes alternated in one process:
  loop           the reference's block as a user writes it on the module route today: per batch of 512, `model.encode(x, std=s)` for
                 s = 0, 0.1, 0.5, 0.8, `model(x)` and (2-D data) `model.generate(512)`; every tensor concatenated, copied to the host and binned
                 with np.histogram2d (128 x 128; five latent panels, and data | recon | gen for 2-D data); then
                 log(var(forward_hidden(x, nz=64), dim=1) + 1e-10) of the last batch with its mean and median
  diagnostics    `PosteriorDiagnostics(model).run(x_all, x_batch)`: one scaled draw, one stacked sampler call and one ardae_hist2d per chunk,
                 ardae_sample_logvar, one host synchronisation
and, for the parts of the new pass, microseconds per call of the histogram launch and of the numpy binning it replaces.
Device events around each pass (the loop's host work lies between them); every route runs one untimed pass first; `rounds` x `repeats`
figures per route; median [min .. max].  Beside each: what 100 training steps cost at that shape (the interval of the 25-Gaussians recipe),
from BENCH_r04.json (config #2) and profiles/r04_configs_and_recipes.txt (config #1).  No ratio is gated: nothing was measured before.
"""
import argparse
import json
import os
import re
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ardae_amd as net  # noqa: E402
from ardae_amd import _lib as L  # noqa: E402

BATCH, BINS = 512, 128


def timed(fn, repeats, calls=1):
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return out


def spread(samples):
    return {"median": statistics.median(samples), "min": min(samples), "max": max(samples), "samples": samples}


def hist(points, val):
    p = points.numpy()
    return np.histogram2d(p[:, 0], p[:, 1], range=[[-val, val], [-val, val]], bins=BINS)[0]


def reference_loop(model, x_all, x_batch, two_d):
    """ivae_ardae.py:956-962 and 980-1038 / 1055-1085 without the drawing."""
    def run():
        keep = {k: [] for k in ("latent", "std08", "std05", "std01", "std0", "data", "output", "gen")}
        for i in range(0, x_all.size(0), BATCH):
            x = x_all[i:i + BATCH]
            b = x.size(0)
            if two_d:
                keep["data"].append(x)
                keep["gen"].append(model.generate(b)[0].detach())
            keep["std0"].append(model.encode(x, std=0).detach().view(b, -1))
            keep["std01"].append(model.encode(x, std=0.1).detach().view(b, -1))
            keep["std05"].append(model.encode(x, std=0.5).detach().view(b, -1))
            keep["std08"].append(model.encode(x, std=0.8).detach().view(b, -1))
            output, _, latent, _, _, _ = model(x)
            keep["latent"].append(latent.detach().view(b, -1))
            if two_d:
                keep["output"].append(output.detach())
        host = {k: torch.cat(v, dim=0).cpu() for k, v in keep.items() if v}
        val = 4 if two_d else 6
        out = {k: hist(host[k], val) for k in ("latent", "std08", "std05", "std01", "std0")}
        if two_d:
            out.update({k: hist(host[k], 6) for k in ("data", "output", "gen")})
        latent = model.forward_hidden(x_batch, nz=64)
        logvar = torch.log(torch.var(latent.detach(), dim=1) + 1e-10)
        out["logvar_qz"] = logvar.view(-1).cpu().numpy()
        out["mean"], out["median"] = torch.mean(logvar).item(), torch.median(logvar).item()
        return out
    return run


def steps_cost():
    """ms per training step at the two shapes, from the committed records."""
    with open(os.path.join(ROOT, "BENCH_r04.json")) as f:
        cfg2 = json.load(f)["parsed"]["ms_per_step"]
    with open(os.path.join(ROOT, "profiles", "r04_configs_and_recipes.txt")) as f:
        cfg1 = float(re.search(r"config #1:.*?([\d.]+) ms/step", f.read()).group(1))
    return {"25gaussians": (cfg1, "profiles/r04_configs_and_recipes.txt, config #1"), "mnist-concat": (cfg2, "BENCH_r04.json, config #2")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_diagnostics_timing.json"))
    a = ap.parse_args()
    torch.manual_seed(0)
    net.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    centres = torch.tensor([[i, j] for i in (-4., -2., 0., 2., 4.) for j in (-4., -2., 0., 2., 4.)])
    cases = {
        "25gaussians": (net.ToyIPVAE(input_dim=2, noise_dim=10, h_dim=256, num_hidden_layers=2, nonlinearity="relu", enc_type="concat", z_dim=2).cuda(),
                        (centres[torch.randint(0, 25, (a.images,), generator=g)] + 0.05 * torch.randn(a.images, 2, generator=g)).cuda(),
                        "mlp-concat (2-D data, noise 10, h 256 x 2, z 2, relu)"),
        "mnist-concat": (net.MNISTIPVAE(input_dim=784, noise_dim=100, h_dim=256, num_hidden_layers=2, nonlinearity="softplus", enc_type="concat",
                                        z_dim=32).cuda(),
                         (torch.rand(a.images, 784, generator=g) < 0.13).float().cuda(), "mnist-concat (784, noise 100, h 256 x 2, z 32, softplus)")}
    cost = steps_cost()
    res = {"device": torch.cuda.get_device_name(0), "images": a.images, "batch": BATCH, "bins": BINS, "repeats": a.repeats, "rounds": a.rounds,
           "unit": "ms per pass", "cases": {}}
    for name, (model, x_all, what) in cases.items():
        two_d = name == "25gaussians"
        pd = net.PosteriorDiagnostics(model)
        x_batch = x_all[-BATCH:].contiguous()
        routes = {"loop": reference_loop(model, x_all, x_batch, two_d), "diagnostics": lambda: pd.run(x_all, x_batch)}
        first = {k: fn() for k, fn in routes.items()}               # one untimed pass per route
        samples = {k: [] for k in routes}
        for _ in range(a.rounds):                                   # alternate the routes
            for k, fn in routes.items():
                samples[k] += timed(fn, a.repeats)
        ms_step, source = cost[name]
        case = {"model": what, "chunks": {"latent": pd.plan_latent(a.images), "logvar": pd.plan_logvar(BATCH)},
                "passes": {k: spread(v) for k, v in samples.items()},
                "counted": {"loop": float(first["loop"]["latent"].sum()), "diagnostics": int(first["diagnostics"]["latent_counts"][0].sum())},
                "logvar_qz_mean": {"loop": first["loop"]["mean"], "diagnostics": first["diagnostics"]["logvar_qz_mean"]},
                "train_steps_100_ms": 100 * ms_step, "train_steps_source": source}
        case["loop_over_diagnostics"] = case["passes"]["loop"]["median"] / case["passes"]["diagnostics"]["median"]
        case["diagnostics_over_100_steps"] = case["passes"]["diagnostics"]["median"] / case["train_steps_100_ms"]
        case["loop_over_100_steps"] = case["passes"]["loop"]["median"] / case["train_steps_100_ms"]
        res["cases"][name] = case
        for k, v in case["passes"].items():
            print(f"{name} {k}: {v['median']:.3f} ms [{v['min']:.3f} .. {v['max']:.3f}]   (100 training steps: {100 * ms_step:.0f} ms)", flush=True)

    # the histogram alone: five slots of 20000 latents, the launch against numpy on host copies that are already there
    z = (1.5 * torch.randn(a.images, 5, 32, generator=g)).cuda()
    counts = torch.zeros(5, BINS, BINS, dtype=torch.int64, device="cuda")
    zh = z.cpu().numpy()
    micro = {"hist2d_kernel": lambda: L.call("ardae_hist2d", z, a.images, 5 * 32, 5, 32, 0, 1, -6.0, 6.0, BINS, counts),
             "numpy_histogram2d": lambda: [np.histogram2d(zh[:, s, 0], zh[:, s, 1], range=[[-6, 6], [-6, 6]], bins=BINS) for s in range(5)],
             "copy_to_host": lambda: z.cpu()}
    msamples = {k: [] for k in micro}
    for k, fn in micro.items():
        timed(fn, 1, 5)
    for _ in range(a.rounds):
        for k, fn in micro.items():
            msamples[k] += [1e3 * t for t in timed(fn, a.repeats, 20)]
    res["five_slots_of_latents"] = dict({k: spread(v) for k, v in msamples.items()}, unit="us per call", shape=[a.images, 5, 32])
    for k, v in msamples.items():
        print(f"{k}: {statistics.median(v):.1f} us [{min(v):.1f} .. {max(v):.1f}]", flush=True)

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({n: {"loop_ms": c["passes"]["loop"]["median"], "diagnostics_ms": c["passes"]["diagnostics"]["median"],
                          "train_steps_100_ms": c["train_steps_100_ms"]} for n, c in res["cases"].items()}))


if __name__ == "__main__":
    main()
