"""Time the conditional AR-DAE without an input encoder (ardae_cdae_desc.kind 16 / 17) against its siblings (kind 0 / 1)  --  reported; the two
conditions below are recorded, not gated.

    python tools/time_noenc_score.py [--window-ms 1000] [--repeats 3] [--rounds 3] [--out profiles/noenc_score_timing.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_noenc_score.py --trace-steps 50    (a run of its own: the kind-16 step alone)
    python tools/time_noenc_score.py --merge-trace DIR                                              (its per-kernel split into the JSON)

1. The cDAE step: `ArdaeCondScoreEngine.step` replayed, kinds 16 / 17 against kinds 0 / 1, alternated in one process, at the cDAE shape of
   BASELINE config #2 (B 512 x S 256, z 32, c 32, h 256, 3 layers, softplus) and at a dae_toy-like small shape (B 256 x S 10, z 2, c 2, h 128).
   `noenc_vs_sibling` records the ratios and whether a new kind's median is above its sibling's by more than the spread between repeats of one
   route (the new kinds run a strict subset of the siblings' N-row layers).
2. The front end of kinds 16 / 17: the first energy layer inside the perturbation kernel (`fused_first`) against the draw + perturb launch followed
   by the stand-alone first layer, inside the replayed step, at both shapes (the small one is not eligible: z = 2).  `fused_first_decision` records
   the rule: the fused form is the engines' default only where it wins by more than the spread of repeated identical runs.
3. The whole VAE-loop step: `ArdaeEngine.step` at config #2 (MNISTIPVAE 784 -> z 32, h 256; B 512, nz_cdae 256) with a kind-16 cDAE against a kind-0
   cDAE, alternated.
Device events around enough replays for a window of `window_ms`, everything warmed, median [min .. max] over rounds x repeats.  The achieved MFMA
rate and the LDS stall share of the front kernel are not measured here (they need a counter run of their own).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ardae_amd as net  # noqa: E402
from time_recon_dae import merge_trace as merge_kernel_split  # noqa: E402

SHAPES = {"config2": dict(B=512, S=256, z=32, c=32, h=256, nl=3), "small": dict(B=256, S=10, z=2, c=2, h=128, nl=3)}
STD_SCALE = 100.0
OUT = os.path.join(ROOT, "profiles", "noenc_score_timing.json")
CLASSES = {"grad": net.MLPGradCARDAE, "res": net.MLPResCARDAE}


def module(kind, enc_input, s):
    torch.manual_seed(0)
    return CLASSES[kind](input_dim=s["z"], context_dim=s["c"], std=1., h_dim=s["h"], num_hidden_layers=s["nl"], nonlinearity="softplus", enc_input=enc_input).cuda()


def engine(kind, enc_input, s, **kw):
    return net.ArdaeCondScoreEngine(module(kind, enc_input, s), net.ScoreConfig(delta=0.1, nsigma=1, lr=1e-4), s["B"], s["S"], std_scale=STD_SCALE, **kw)


def batch(s):
    g = torch.Generator().manual_seed(1)
    mean = torch.randn(s["B"], s["z"], generator=g).cuda()
    return (mean[:, None, :] + 0.01 * torch.randn(s["B"], s["S"], s["z"], generator=g).cuda()).contiguous(), torch.randn(s["B"], s["c"], generator=g).cuda(), mean


def timed(fn, steps, repeats):
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


def measure(routes, a):
    """Warm every route (the engines capture at their third call), size its window, then alternate the routes."""
    steps, samples = {}, {k: [] for k in routes}
    for k, fn in routes.items():
        once = timed(fn, 10, 2)[-1]
        steps[k] = max(10, int(a.window_ms / max(once, 1e-3)) + 1)
    for _ in range(a.rounds):
        for k, fn in routes.items():
            samples[k] += timed(fn, steps[k], a.repeats)
    out = {k: spread(v) for k, v in samples.items()}
    for k in out:
        out[k]["steps_per_window"] = steps[k]
    return out


def show(row):
    return ", ".join(f"{k} {v['median']:.4f} [{v['min']:.4f} .. {v['max']:.4f}]" for k, v in row.items() if isinstance(v, dict) and "median" in v)


def vae_engine(enc_input):
    torch.manual_seed(0)
    model = net.MNISTIPVAE(input_dim=784, noise_dim=100, h_dim=256, num_hidden_layers=2, nonlinearity="softplus", enc_type="concat", z_dim=32).cuda()
    return net.ArdaeEngine(model, module("grad", enc_input, SHAPES["config2"]), net.TrainConfig(nz_cdae=256), batch_size=512)


def trace_run(steps):
    """The kind-16 step alone, for a profiler run of its own"""
    s = SHAPES["config2"]
    latent, ctx, mean = batch(s)
    eng = engine("grad", False, s, graph=False)
    for _ in range(steps):
        eng.step(latent, ctx, mean)
    torch.cuda.synchronize()
    print(f"{steps} kind-16 steps (fused_first {eng.fused_first}), last loss {eng.stats()['loss']:.5f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=1000.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--merge-trace")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.merge_trace:
        merge_kernel_split(a.merge_trace, a.out)
        with open(a.out) as f:
            res = json.load(f)
        res["profile_kernel_split"] = res.pop("kind13_step_kernel_split")
        res["profile_kernel_split"]["source"] = "rocprofv3 --kernel-trace --stats, a run of its own (eager kind-16 steps at the config #2 shape)"
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        return
    if a.trace_steps:
        return trace_run(a.trace_steps)
    res = {"device": torch.cuda.get_device_name(0), "window_ms": a.window_ms, "repeats": a.repeats, "rounds": a.rounds, "unit": "ms", "cdae_step": {},
           "front_end": {}, "not_measured": ["achieved MFMA rate of the front kernel", "LDS stall share of the front kernel"]}

    # 1. the cDAE step, the new kinds against their siblings
    verdict = {}
    for name, s in SHAPES.items():
        latent, ctx, mean = batch(s)
        engines = {f"kind{k}": engine(kind, enc, s) for k, kind, enc in ((0, "grad", True), (16, "grad", False), (1, "res", True), (17, "res", False))}
        row = dict(s, rows=s["B"] * s["S"], forms={k: dict(fused_first=bool(e.fused_first), fused_draw=bool(e.fused_draw)) for k, e in engines.items()})
        row.update(measure({k: (lambda e=e: e.step(latent, ctx, mean)) for k, e in engines.items()}, a))
        res["cdae_step"][name] = row
        print(f"cdae_step/{name}: " + show(row), flush=True)
        for new, sib in ((16, 0), (17, 1)):
            n, o = row[f"kind{new}"], row[f"kind{sib}"]
            band = max(v["max"] - v["min"] for v in (n, o))
            verdict[f"{name}/kind{new}_vs_kind{sib}"] = {"ratio": n["median"] / o["median"], "new_median": n["median"], "sibling_median": o["median"],
                                                       "spread_between_repeats": band, "new_slower_beyond_spread": bool(n["median"] - o["median"] > band)}
        del engines
    res["noenc_vs_sibling"] = {"rule": "kinds 16 / 17 run a strict subset of their siblings' N-row layers: at config #2's shape their median must not exceed "
                                       "the sibling's by more than the spread between repeats of one route", **verdict}

    # 2. the front end of the new kinds
    wins = {}
    for name, s in SHAPES.items():
        latent, ctx, mean = batch(s)
        for k, kind in ((16, "grad"), (17, "res")):
            on, off = engine(kind, False, s, fused_first=True), engine(kind, False, s, fused_first=False)
            if not on.fused_first:
                res["front_end"][f"{name}/kind{k}"] = "not eligible (ardae_cdae_perturb_fused_ok = 0): the step has its separate launches only"
                continue
            # the unfused form twice: the spread of repeated identical runs
            routes = {"fused_first": lambda: on.step(latent, ctx, mean), "draw_then_layer": lambda: off.step(latent, ctx, mean),
                      "draw_then_layer_again": lambda: off.step(latent, ctx, mean)}
            row = measure(routes, a)
            band = max(max(v["max"] - v["min"] for v in row.values()), abs(row["draw_then_layer"]["median"] - row["draw_then_layer_again"]["median"]))
            gain = min(row["draw_then_layer"]["median"], row["draw_then_layer_again"]["median"]) - row["fused_first"]["median"]
            row.update(gain_ms=gain, spread_of_identical_runs=band, fused_wins_beyond_spread=bool(gain > band))
            res["front_end"][f"{name}/kind{k}"] = row
            wins[f"{name}/kind{k}"] = bool(gain > band)
            print(f"front_end/{name}/kind{k}: " + show(row) + f"; gain {gain:.4f} ms, spread {band:.4f} ms", flush=True)
            del on, off
    res["fused_first_decision"] = {"rule": "fused_first is the engines' default for kinds 16 / 17 only where it wins by more than the spread of repeated identical runs",
                                   "fused_wins_beyond_spread": wins, "engine_default": bool(net.ArdaeCondScoreEngine.FUSED_FIRST_NOENC_DEFAULT)}

    # 3. the whole VAE-loop step at config #2
    g = torch.Generator().manual_seed(2)
    xc, xv = (torch.bernoulli(torch.full((512, 784), 0.15), generator=g).cuda() for _ in range(2))
    engines = {"kind0": vae_engine(True), "kind16": vae_engine(False)}
    row = measure({k: (lambda e=e: e.step(xc, xv)) for k, e in engines.items()}, a)
    row["ratio_kind16_over_kind0"] = row["kind16"]["median"] / row["kind0"]["median"]
    res["vae_loop_step_config2"] = row
    print("vae_loop_step/config2: " + show(row), flush=True)

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["noenc_vs_sibling"]))
    print(json.dumps(res["fused_first_decision"]))


if __name__ == "__main__":
    main()
