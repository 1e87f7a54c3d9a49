"""Time the AR-DAE half of the two notebook loops on the device  --  reported, not gated.

    python tools/time_ardae_fit.py [--steps 200] [--repeats 5] [--out profiles/ardae_uncond_timing.json]

Per notebook shape (ardae_toy.ipynb: 256 x 10 rows, h 128; ardae_fit.ipynb: 1024 x 10 rows, h 256; d 2, 3 hidden layers, softplus) and
kind: milliseconds per `ArdaeScoreEngine.step` with the fused front end (draw + perturbation + first layer in one kernel) and with the
unfused one (two draws, scale, perturbation, first layer as launches of their own), alternated in one process; per `score()` on the
batch; and per step of a plain PyTorch autograd loop of the same network on the same device (the notebooks' own code path: broadcast,
randn, double backward through autograd, torch.optim.RMSprop).  Device events around `steps` calls, median of `repeats`.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ardae_uncond_timing.json"))
    ap.add_argument("--profile-kernels", action="store_true")
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
    for name, (B, ns, d, h, nl) in SHAPES.items():
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
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
