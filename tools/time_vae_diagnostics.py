"""Time the diagnostics of the Gaussian baselines (vae.py's `''' visualize '''` block, :497-593), both scripts' last block
(`''' test visualize '''`, vae.py:677-720, ivae_ardae.py:1224-1290) and the wide histogram kernel on the device.

    python tools/time_vae_diagnostics.py [--images 20000] [--points 1000000] [--repeats 1] [--rounds 3] [--out profiles/vae_diagnostics_timing.json]

Three parts, every figure a median [min .. max] of `rounds` x `repeats` samples taken after one untimed pass per route; a sample times as many passes
as fill about 200 ms and reports the time per pass:
  block        per Gaussian kind at its class defaults (the reference's constructor defaults: the recipes' widths), milliseconds per pass over `images` synthetic images, two routes
               alternated in one process:
                 loop         the reference's block as a user writes it on the drop-in module route: per batch of 128 `model(x)` and (2-D data)
                              `model.generate(128)`; every tensor concatenated, copied to the host and binned with np.histogram2d at 128 bins
                 diagnostics  `GaussianDiagnostics(model).run(x_all)`: the encoder statistics, the draw and one histogram launch per chunk (2-D
                              data: two decoder passes and three more histogram launches); no host synchronisation inside
  final_pass   `GaussianDiagnostics(ToyVAE).final_pass` and `PosteriorDiagnostics(ToyIPVAE).final_pass` over `points` points at 256 bins
  kernel       ardae_hist2d_wide alone on `points` points at 256 and 512 bins, for normal points and for all points in one cell, next to
               ardae_hist2d at 128 bins on the same points; microseconds per call
Device events around each pass (the loop's host work lies between them).  No ratio is gated: nothing was measured before.  The share of the wide
kernel's time that goes to LDS-atomic contention is not measured here (that takes hardware counters, in a run of their own).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ardae_amd as net  # noqa: E402
from ardae_amd import _lib as L  # noqa: E402

BATCH = 128                                                                     # --train-batch-size of the recipes: 20000 // 128 + 1 = 157 forward calls


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


def calls_for(fn, window_ms=200.0, most=256):
    """Passes per sample, so that a sample times about `window_ms` of work (a pass of a millisecond alone would measure the clock)."""
    return max(1, min(most, int(window_ms / max(timed(fn, 1)[0], 1e-3))))


def spread(samples):
    return {"median": statistics.median(samples), "min": min(samples), "max": max(samples), "samples": samples}


def hist(points, val, bins=128):
    p = points.numpy()
    return np.histogram2d(p[:, 0], p[:, 1], range=[[-val, val], [-val, val]], bins=bins)[0]


def reference_loop(model, x_all, two_d):
    """vae.py:499-570 without the drawing."""
    def run():
        keep = {k: [] for k in ("latent", "data", "output", "gen")}
        for i in range(0, x_all.size(0), BATCH):
            x = x_all[i:i + BATCH]
            b = x.size(0)
            if two_d:
                keep["data"].append(x)
                keep["gen"].append(model.generate(b)[0].detach())
            output, _, latent, _, _, _ = model(x)
            keep["latent"].append(latent.detach().view(b, -1))
            if two_d:
                keep["output"].append(output.detach())
        host = {k: torch.cat(v, dim=0).cpu() for k, v in keep.items() if v}
        out = {"latent": hist(host["latent"], 4 if two_d else 6)}
        if two_d:
            out.update({k: hist(host[k], 6) for k in ("data", "output", "gen")})
        return out
    return run


def gaussians25(n, g):
    centres = torch.tensor([[i, j] for i in (-4., -2., 0., 2., 4.) for j in (-4., -2., 0., 2., 4.)])
    return (centres[torch.randint(0, 25, (n,), generator=g)] + 0.05 * torch.randn(n, 2, generator=g)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=20000)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kinds", default="mnist,toy,conv,resconv,auxmnist,auxtoy,auxconv,auxresconv")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_diagnostics_timing.json"))
    a = ap.parse_args()
    torch.manual_seed(0)
    net.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    kinds = {"mnist": net.MNISTVAE, "toy": net.ToyVAE, "conv": net.MNISTConvVAE, "resconv": net.MNISTResConvVAE, "auxmnist": net.MNISTAuxVAE,
             "auxtoy": net.ToyAuxVAE, "auxconv": net.MNISTConvAuxVAE, "auxresconv": net.MNISTResConvAuxVAE}
    res = {"device": torch.cuda.get_device_name(0), "images": a.images, "points": a.points, "batch": BATCH, "repeats": a.repeats, "rounds": a.rounds,
           "block": {"unit": "ms per pass", "bins": 128, "kinds": {}}}
    pixels = (torch.rand(a.images, 784, generator=g) < 0.13).float().cuda()
    toy_x = gaussians25(a.images, g)

    # ---- 1. the training block, per kind ------------------------------------------------------------------------------------------------
    for name in a.kinds.split(","):
        model = kinds[name]().cuda()
        two_d = name in ("toy", "auxtoy")
        x_all = toy_x if two_d else pixels
        gd = net.GaussianDiagnostics(model)
        routes = {"loop": reference_loop(model, x_all, two_d), "diagnostics": lambda: gd.run(x_all)}
        first = {k: fn() for k, fn in routes.items()}               # one untimed pass per route
        torch.cuda.synchronize()
        calls = {k: calls_for(fn) for k, fn in routes.items()}
        samples = {k: [] for k in routes}
        for _ in range(a.rounds):                                   # alternate the routes
            for k, fn in routes.items():
                samples[k] += timed(fn, a.repeats, calls[k])
        case = {"model": f"{type(model).__name__}() at its defaults: input {model.input_dim}, z {model.z_dim}, h {model.h_dim}, noise {model.noise_dim}",
                "chunks": len(gd.plan(a.images, two_d)), "passes_per_sample": calls, "passes": {k: spread(v) for k, v in samples.items()},
                "counted": {"loop": float(first["loop"]["latent"].sum()), "diagnostics": int(first["diagnostics"]["latent_counts"].sum())}}
        case["loop_over_diagnostics"] = case["passes"]["loop"]["median"] / case["passes"]["diagnostics"]["median"]
        res["block"]["kinds"][name] = case
        for k, v in case["passes"].items():
            print(f"{name} {k}: {v['median']:.3f} ms [{v['min']:.3f} .. {v['max']:.3f}]", flush=True)
        del model, gd, routes, first

    # ---- 2. the last block: `points` points at 256 bins ---------------------------------------------------------------------------------
    x_big = gaussians25(a.points, g)
    finals = {"ToyVAE": net.GaussianDiagnostics(net.ToyVAE().cuda()),
              "ToyIPVAE": net.PosteriorDiagnostics(net.ToyIPVAE(input_dim=2, noise_dim=10, h_dim=256, num_hidden_layers=2, nonlinearity="relu",
                                                                enc_type="concat", z_dim=2).cuda())}
    res["final_pass"] = {"unit": "ms per pass", "bins": 256, "models": {}}
    for name, diag in finals.items():
        first = diag.final_pass(x_big)
        torch.cuda.synchronize()
        calls, samples = calls_for(lambda: diag.final_pass(x_big)), []
        for _ in range(a.rounds):
            samples += timed(lambda: diag.final_pass(x_big), a.repeats, calls)
        chunks = len(diag.plan(a.points, True)) if name == "ToyVAE" else {"latent": len(diag.plan_latent(a.points)), "data": len(diag.plan_data(a.points))}
        res["final_pass"]["models"][name] = {"pass": spread(samples), "chunks": chunks, "passes_per_sample": calls,
                                             "counted": {"latent": int(first["latent_counts"].sum()), "data": int(first["data_counts"].sum())}}
        print(f"final pass {name}: {statistics.median(samples):.3f} ms [{min(samples):.3f} .. {max(samples):.3f}]", flush=True)
    del finals

    # ---- 3. the kernel alone ------------------------------------------------------------------------------------------------------------
    sets = {"normal": (1.5 * torch.randn(a.points, 2, generator=g)).cuda(), "one_cell": torch.tensor([[0.3, -1.1]]).repeat(a.points, 1).cuda()}
    counts = {b: torch.zeros(1, b, b, dtype=torch.int64, device="cuda") for b in (128, 256, 512)}
    micro = {}
    for what, pts in sets.items():
        micro[f"hist2d_128_{what}"] = lambda pts=pts: L.call("ardae_hist2d", pts, a.points, 2, 1, 0, 0, 1, -6.0, 6.0, 128, counts[128])
        for b in (256, 512):
            micro[f"hist2d_wide_{b}_{what}"] = lambda pts=pts, b=b: L.call("ardae_hist2d_wide", pts, a.points, 2, 1, 0, 0, 1, -6.0, 6.0, b, counts[b])
    msamples = {k: [] for k in micro}
    for k, fn in micro.items():
        timed(fn, 1, 5)
    for _ in range(a.rounds):
        for k, fn in micro.items():
            msamples[k] += [1e3 * t for t in timed(fn, max(a.repeats, 2), 20)]
    res["kernel"] = dict({k: spread(v) for k, v in msamples.items()}, unit="us per call", points=a.points, range=[-6.0, 6.0],
                         lds_atomic_contention_share="not measured (no hardware-counter run was made)")
    for k, v in msamples.items():
        print(f"{k}: {statistics.median(v):.1f} us [{min(v):.1f} .. {max(v):.1f}]", flush=True)

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({n: {"loop_ms": c["passes"]["loop"]["median"], "diagnostics_ms": c["passes"]["diagnostics"]["median"]}
                      for n, c in res["block"]["kinds"].items()}))


if __name__ == "__main__":
    main()
