"""Time the train step while --beta-annealing moves beta, and check that the device schedule replays at the constant-beta step's speed.

    python tools/time_beta_annealing.py [--steps 200] [--repeats 5] [--rounds 3] [--out profiles/beta_annealing_timing.json]

Per shape - BASELINE config #2 (512 images x 256 Monte-Carlo rows) and its 64-image shard (what one of 8 ranks runs) - three engines,
alternated round by round in one process:

  a  constant beta, the captured step replayed                                       (the steady state)
  b  beta passed by the caller every step while it moves (`step(beta=)`): the engine launches eagerly, as it did during the
     first --beta-annealing steps of the annealed recipes before the schedule moved to the device
  c  the device schedule (`TrainConfig(beta_init=1e-4, beta_annealing=50000)`, run_vae_sbmnist.sh) while beta moves: replayed

The workload is bench.py's: its networks, seeds and on-device binarisation are set up inside bench.main(), which cannot be called for
its parts, so `variant` restates them and `check_against_bench` refuses to run when bench.py's source no longer holds those lines.
Device events around `steps` calls; every shape and variant is warmed up (capture included) before anything is timed; median
[min .. max] over rounds x repeats, every sample kept in the file.  c is the same graph as a, so c's median must lie within a's
[min .. max] at each shape: the file records it per shape and the tool exits with status 1 where it does not hold.
`--control` adds a fourth engine, reported only (the check above does not look at it): a constant-beta replay like a, at the beta the
ramp takes in the middle of the timed window - the same launches as a on weights trained in c's regime (DESIGN section 6 quotes
profiles/beta_annealing_timing_control.json for the 512 x 256 shape; a fourth engine in the process changed c's time on the shard in
the runs made so far, so the check is read from a run without it)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import ardae_amd as net  # noqa: E402
from ardae_amd import _lib as L  # noqa: E402

NZ = 256
SHAPES = {"config2_512x256": 512, "shard_64x256": 64}
RECIPE = dict(beta=1.0, beta_init=1e-4, beta_annealing=50000)       # run_vae_sbmnist.sh / run_vae_dbmnist.sh:28


# what `variant` restates, as bench.main() writes it (bench.py is not edited with this tool: a mismatch means it has moved on)
BENCH_LINES = ('GLOBAL_B, NZ = int(knob("BENCH_GLOBAL_B", "512")), 256',
               'torch.manual_seed(0)',
               'model = net.MNISTIPVAE(input_dim=784, noise_dim=100, h_dim=256, num_hidden_layers=2, nonlinearity="softplus",',
               'enc_type="concat", z_dim=32).to(dev)',
               'cdae = net.MLPGradCARDAE(input_dim=32, context_dim=32, std=1., h_dim=256, num_hidden_layers=3, nonlinearity="softplus",',
               'noise_type="gaussian", enc_ctx=True, enc_input=True).to(dev)',
               'g = torch.Generator(device="cpu").manual_seed(1234)',
               'pimg = ((torch.rand(784, generator=g) < 0.2).float() * 0.6 + 0.03).to(dev)',
               'net.TrainConfig(nz_cdae=NZ)',
               'net.manual_seed(42)',
               '(xc,), xv = eng.input_buffers(1)',
               'lib.ardae_bernoulli(L.ptr(pimg), B, 784, L.ptr(xc), ctypes.c_uint64(1000 + rank), ctypes.c_uint64(2 * i), L.stream_ptr())',
               'lib.ardae_bernoulli(L.ptr(pimg), B, 784, L.ptr(xv), ctypes.c_uint64(1000 + rank), ctypes.c_uint64(2 * i + 1), L.stream_ptr())')


def check_against_bench():
    import inspect
    src = inspect.getsource(bench.main)
    missing = [line for line in BENCH_LINES if line not in src]
    if missing:
        raise SystemExit("tools/time_beta_annealing.py restates bench.py's workload, which has changed: bench.main() no longer holds\n  " +
                         "\n  ".join(missing))


def spread(samples):
    return {"median": statistics.median(samples), "min": min(samples), "max": max(samples), "samples": samples}


def timed_all(fn, steps, repeats):
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


def variant(B, cfg, fed):
    """bench.py's workload at batch B: one step function (two fresh binarised batches written into the engine's static buffers, then
    step()); fed: the caller computes beta per step."""
    torch.manual_seed(0)
    model = net.MNISTIPVAE(input_dim=784, noise_dim=100, h_dim=256, num_hidden_layers=2, nonlinearity="softplus", enc_type="concat", z_dim=32).cuda()
    cdae = net.MLPGradCARDAE(input_dim=32, context_dim=32, std=1., h_dim=256, num_hidden_layers=3, nonlinearity="softplus", noise_type="gaussian",
                             enc_ctx=True, enc_input=True).cuda()
    g = torch.Generator(device="cpu").manual_seed(1234)
    pimg = ((torch.rand(784, generator=g) < 0.2).float() * 0.6 + 0.03).cuda()
    eng = net.ArdaeEngine(model, cdae, cfg, batch_size=B)
    net.manual_seed(42)
    (xc,), xv = eng.input_buffers(1)
    i = [0]

    def step():
        k = i[0]
        i[0] += 1
        L.call("ardae_bernoulli", pimg, B, 784, xc, 1000, 2 * k)
        L.call("ardae_bernoulli", pimg, B, 784, xv, 1000, 2 * k + 1)
        if fed:
            eng.step(xc, xv, beta=net.annealing_func(RECIPE["beta_init"], RECIPE["beta"], RECIPE["beta_annealing"], k))
        else:
            eng.step(xc, xv)
    return eng, step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--control", action="store_true", help="also time a constant-beta replay at the ramp's mid-window beta (reported only)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beta_annealing_timing.json"))
    a = ap.parse_args()
    check_against_bench()
    total = a.warmup + a.rounds * a.repeats * a.steps
    assert total < RECIPE["beta_annealing"], "every timed step must lie on the ramp"
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "repeats": a.repeats, "rounds": a.rounds, "unit": "ms per step",
           "schedule": RECIPE, "shapes": {}}
    for name, B in SHAPES.items():
        runs = {"a_constant_beta_replay": variant(B, net.TrainConfig(nz_cdae=NZ), False),
                "b_caller_beta_eager": variant(B, net.TrainConfig(nz_cdae=NZ), True),
                "c_device_schedule_replay": variant(B, net.TrainConfig(nz_cdae=NZ, **RECIPE), False)}
        if a.control:
            mid = net.annealing_func(RECIPE["beta_init"], RECIPE["beta"], RECIPE["beta_annealing"], total // 2)
            runs["control_constant_beta_at_ramp_value_replay"] = variant(B, net.TrainConfig(nz_cdae=NZ, beta=mid), False)
        for _, step in runs.values():           # every variant of the shape warm (kernels loaded, graphs captured) before any is timed
            for _ in range(a.warmup):
                step()
        torch.cuda.synchronize()
        graphs = {k: eng._graph is not None for k, (eng, _) in runs.items()}
        assert graphs == dict({k: True for k in runs}, b_caller_beta_eager=False), graphs
        samples = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, (_, step) in runs.items():
                samples[k] += timed_all(step, a.steps, a.repeats)
        row = {k: spread(v) for k, v in samples.items()}
        ra, rc = row["a_constant_beta_replay"], row["c_device_schedule_replay"]
        row["replayed"] = graphs
        if a.control:
            row["control_beta"] = mid
        row["c_median_within_a_min_max"] = ra["min"] <= rc["median"] <= ra["max"]
        row["b_over_a_median"] = row["b_caller_beta_eager"]["median"] / ra["median"]
        res["shapes"][name] = dict(row, batch=B, nz_cdae=NZ)
        del runs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({n: {k: (round(v["median"], 4), round(v["min"], 4), round(v["max"], 4)) if isinstance(v, dict) and "median" in v else v
                          for k, v in r.items()} for n, r in res["shapes"].items()}))
    missed = [n for n, r in res["shapes"].items() if not r["c_median_within_a_min_max"]]
    if missed:
        sys.stderr.write("the device schedule's median lies outside the constant-beta replay's [min .. max] at: " + ", ".join(missed) + "\n")
        sys.exit(1)


if __name__ == "__main__":
    main()
