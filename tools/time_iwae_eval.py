"""Time IWAE evaluation (evaluate_iws, ivae_ardae.py:644-673) on the device  --  gated: the evaluator must not lose to the loop it replaces.

    python tools/time_iwae_eval.py [--images 2048] [--repeats 3] [--rounds 3] [--out profiles/iwae_eval_timing.json]

Model: the `mnist-concat` recipe's widths (784 pixels, noise 100, h 256, 2 hidden layers, z 32, softplus) at --iws-samples 256; data:
`images` synthetic binarised images.  Milliseconds per pass over the set, of three routes alternated in one process:
  loop_b32      the reference's loop over `model.logprob(batch, sample_size=256)` at --eval-batch-size 32, one `.item()` per batch
  loop_b1       the same loop at batch 1 (the sbMNIST / 25-Gaussians recipes' evaluation batch), on the first 256 images
  evaluator     `IwaeEvaluator(model, 256).evaluate(x_all)`: large chunks, the fused proposal kernel, one host synchronisation
and, on the encoder samples of one batch of 32 images, microseconds per call of
  proposal_kernel   ardae_iwae_proposal (mean, covariance, factor, proposal samples, log-density: one launch)
  proposal_torch    the torch glue of `model.logprob` that it replaces (about twenty launches and the host's isfinite check)
Device events around each pass; every route runs one untimed pass first; `rounds` x `repeats` figures per route; median [min .. max].
Exit code 1 if the evaluator's median is above loop_b32's minimum (both from this run; loop_b32 is untouched by the evaluator).
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ardae_amd as net  # noqa: E402
from ardae_amd import _lib as L  # noqa: E402

K = 256


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


def reference_loop(model, x_all, batch):
    """evaluate_iws: logprob += model.logprob(batch_x, sample_size=k).item() * batch size; / num_total."""
    def run():
        total = 0.0
        for i in range(0, x_all.size(0), batch):
            xb = x_all[i:i + batch]
            total += model.logprob(xb, sample_size=K).item() * xb.size(0)
        return total / x_all.size(0)
    return run


def torch_glue(zs, e):
    """The lines of ImplicitPosteriorVAE.logprob between the sampler and the decoder."""
    B, ke, zd = zs.shape

    def run():
        mu = zs.mean(1)
        zc = zs - mu.unsqueeze(1)
        cov = (zc.transpose(1, 2) @ zc / (ke - 1)).contiguous()
        Lc = torch.empty_like(cov)
        L.call("ardae_cholesky_batched", cov, B, zd, Lc)
        if not bool(torch.isfinite(Lc).all()):
            raise ValueError("not positive definite")
        newz = (mu.unsqueeze(1) + e @ Lc.transpose(1, 2)).contiguous()
        logq = -0.5 * (e ** 2).sum(2) - torch.log(torch.diagonal(Lc, dim1=1, dim2=2)).sum(1, keepdim=True) - 0.5 * zd * math.log(2 * math.pi)
        return newz, logq
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iwae_eval_timing.json"))
    a = ap.parse_args()
    torch.manual_seed(0)
    net.manual_seed(0)
    model = net.MNISTIPVAE(input_dim=784, noise_dim=100, h_dim=256, num_hidden_layers=2, nonlinearity="softplus", enc_type="concat", z_dim=32).cuda()
    x_all = (torch.rand(a.images, 784, device="cuda") < 0.13).float()
    ev = net.IwaeEvaluator(model, K)
    routes = {"loop_b32": reference_loop(model, x_all, 32), "loop_b1": reference_loop(model, x_all[:256], 1), "evaluator": lambda: ev.evaluate(x_all)}
    values = {k: fn() for k, fn in routes.items()}              # one untimed pass per route (and the three estimates of the same bound)
    samples = {k: [] for k in routes}
    for _ in range(a.rounds):                                   # alternate the routes
        for k, fn in routes.items():
            samples[k] += timed(fn, a.repeats)
    res = {"device": torch.cuda.get_device_name(0), "images": a.images, "loop_b1_images": 256, "sample_size": K, "repeats": a.repeats, "rounds": a.rounds,
           "model": "mnist-concat (784, noise 100, h 256 x 2, z 32, softplus)", "chunks": ev.plan(a.images), "unit": "ms per pass",
           "bound": values, "passes": {k: spread(v) for k, v in samples.items()}}
    for k, v in res["passes"].items():
        print(f"{k}: {v['median']:.3f} ms [{v['min']:.3f} .. {v['max']:.3f}]  bound {values[k]:.4f}", flush=True)

    # the proposal alone, on one batch of 32 images' encoder samples
    zs = model.forward_hidden(x_all[:32], nz=K).contiguous()
    e = torch.randn(32, K, 32, device="cuda")
    newz, logq = torch.empty(32, K, 32, device="cuda"), torch.empty(32, K, device="cuda")
    micro = {"proposal_kernel": lambda: L.call("ardae_iwae_proposal", zs, e, 32, K, K, 32, 0.0, 0, 0, 0, newz, logq, None, None, None),
             "proposal_torch": torch_glue(zs, e)}
    msamples = {k: [] for k in micro}
    for k, fn in micro.items():
        timed(fn, 1, 50)
    for _ in range(a.rounds):
        for k, fn in micro.items():
            msamples[k] += [1e3 * t for t in timed(fn, a.repeats, 200)]
    res["proposal_32_images"] = dict({k: spread(v) for k, v in msamples.items()}, unit="us per call")
    for k, v in msamples.items():
        print(f"{k}: {statistics.median(v):.1f} us [{min(v):.1f} .. {max(v):.1f}]", flush=True)

    ok = res["passes"]["evaluator"]["median"] <= res["passes"]["loop_b32"]["min"]
    res["gate"] = {"rule": "evaluator median <= loop_b32 min", "passed": ok}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"evaluator_ms": res["passes"]["evaluator"]["median"], "loop_b32_ms": res["passes"]["loop_b32"]["median"],
                      "loop_b1_ms_256_images": res["passes"]["loop_b1"]["median"], "gate_passed": ok}))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
