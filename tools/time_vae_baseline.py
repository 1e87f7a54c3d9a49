"""Time the Gaussian-posterior VAE baselines (vae.py --model mnist / toy / conv) on the device  --  reported, not gated.

    python tools/time_vae_baseline.py [--steps 200] [--engine-steps 1000] [--repeats 5] [--rounds 3] [--out profiles/vae_baseline_timing.json]
    python tools/time_vae_baseline.py --shapes conv_128x784_z32        # -> profiles/vae_conv_baseline_timing.json

At the recipe shape (mnist: 128 x 784, h 300, z 32, 2 layers, softplus) and at the toy shape (toy: 1024 x 2, h 256, z 2, 2 layers, relu), or
(`--shapes`) at the conv recipe's (conv: 128 x 784, z 32, softplus; the head's h is 800), milliseconds per call of
  engine_replay      (a) `VaeEngine.step`, the captured unit replayed (vendored Adam, beta ramp of 50000 steps on the device)
  engine_eager       (b) the same engine with graph=False
  torch_autograd     (c) a plain PyTorch autograd loop of the same network with torch.optim.Adam on the same device: the yardstick, not the
                         code under test
  head_fused / head_unfused   (d) the Gaussian head alone (ardae_vae_head variant 1 / 2) on the shape's [B, h] hidden rows, drawing its eps;
                         conv shape: also gauss_head_kernel at h = 800 (a kind-8 descriptor) against its unfused launches, and the conv head at z = 6
  iwae_engine / iwae_logprob_loop   (e) `evaluate_iws` of the first MNIST-sized shape on 2048 images at k = 256 against the loop over `model(x)` + `model.logprob(x)` at batch 32
                         (vae.py:352-370), as tools/time_iwae_eval.py does for the implicit models; seconds per set
Device events around `steps` calls; every route runs one untimed window first; the routes of a group are alternated over `rounds`;
`rounds` x `repeats` figures per route; median [min .. max] are recorded.
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

SHAPES = {"mnist_128x784_h300_z32": ("mnist", 128, 784, 300, 32, 2, "softplus"), "toy_1024x2_h256_z2": ("toy", 1024, 2, 256, 2, 2, "relu"),
          "conv_128x784_z32": ("conv", 128, 784, 800, 32, 1, "softplus")}
DEFAULT_SHAPES = "mnist_128x784_h300_z32,toy_1024x2_h256_z2"
IWAE = dict(images=2048, k=256, loop_batch=32)


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


def alternate(routes, steps, repeats, rounds):
    samples = {k: [] for k in routes}
    for k, fn in routes.items():            # one untimed window per route
        timed_all(fn, steps[k], 1)
    for _ in range(rounds):
        for k, fn in routes.items():
            samples[k] += timed_all(fn, steps[k], repeats)
    return {k: spread(v) for k, v in samples.items()}


def module(family, D, h, z, nl, act):
    if family == "conv":
        return net.MNISTConvVAE(z_dim=z, nonlinearity=act).cuda()
    ctor = net.MNISTVAE if family == "mnist" else net.ToyVAE
    return ctor(input_dim=D, h_dim=h, z_dim=z, nonlinearity=act, num_hidden_layers=nl).cuda()


class TorchVAE(torch.nn.Module):
    """The same network in plain PyTorch (nn.Linear stacks, the reference's loss lines) for the autograd column."""

    def __init__(self, family, D, h, z, nl, act):
        super().__init__()
        A = torch.nn.Softplus if act == "softplus" else torch.nn.ReLU

        def stack(w):
            layers = []
            for _ in range(nl):
                layers += [torch.nn.Linear(w, h), A()]
                w = h
            return torch.nn.Sequential(*layers)
        self.family, self.D = family, D
        self.enc, self.mean, self.logvar, self.dec = stack(D), torch.nn.Linear(h, z), torch.nn.Linear(h, z), stack(z)
        self.out = torch.nn.Linear(h, D)
        self.out_lv = torch.nn.Linear(h, D) if family == "toy" else None

    def forward(self, x, beta):
        hdn = self.enc(2 * x - 1 if self.family == "mnist" else x)
        mu, lv = self.mean(hdn), self.logvar(hdn)
        z = mu + torch.exp(0.5 * lv) * torch.randn_like(mu)
        kld = -0.5 * (1 + lv - mu.pow(2) - lv.exp()).sum(1)
        hd = self.dec(z)
        if self.family == "mnist":
            rec = torch.nn.functional.binary_cross_entropy_with_logits(self.out(hd), x, reduction="none").sum(1)
        else:
            m, l = self.out(hd), self.out_lv(hd)
            rec = 0.5 * (l + (x - m) ** 2 / l.exp() + 1.8378770664093453).sum(1)
        return (rec + beta * kld).mean()


class TorchConvVAE(torch.nn.Module):
    """models/vae/conv.py in plain PyTorch (nn.Conv2d / nn.ConvTranspose2d, the reference's loss lines) for the autograd column."""

    def __init__(self, z, act):
        super().__init__()
        nn = torch.nn
        self.D, self.a = 784, torch.nn.functional.softplus if act == "softplus" else torch.relu
        self.conv1, self.conv2, self.conv3 = nn.Conv2d(1, 16, 5, 2, 2), nn.Conv2d(16, 32, 5, 2, 2), nn.Conv2d(32, 32, 5, 2, 2)
        self.fc, self.mean, self.logvar = nn.Linear(512, 800), nn.Linear(800, z), nn.Linear(800, z)
        self.d1, self.d2 = nn.Linear(z, 300), nn.Linear(300, 512)
        self.deconv1, self.deconv2, self.logit = nn.ConvTranspose2d(32, 32, 5, 2, 2), nn.ConvTranspose2d(32, 16, 5, 2, 2), nn.ConvTranspose2d(16, 1, 5, 2, 2)

    def forward(self, x, beta):
        a, B = self.a, x.size(0)
        hdn = a(self.conv3(a(self.conv2(a(self.conv1((2 * x - 1).view(B, 1, 28, 28)))))))
        hdn = a(self.fc(hdn.view(B, -1)))
        mu, lv = self.mean(hdn), self.logvar(hdn)
        z = mu + torch.exp(0.5 * lv) * torch.randn_like(mu)
        kld = -0.5 * (1 + lv - mu.pow(2) - lv.exp()).sum(1)
        hd = a(self.d2(a(self.d1(z)))).view(B, 32, 4, 4)
        hd = a(self.deconv2(torch.nn.functional.pad(a(self.deconv1(hd)), (0, 1, 0, 1))))
        logit = self.logit(hd)[:, :, :28, :28].reshape(B, 784)
        rec = torch.nn.functional.binary_cross_entropy_with_logits(logit, x, reduction="none").sum(1)
        return (rec + beta * kld).mean()


def torch_loop(tm, x, lr):
    opt = torch.optim.Adam(tm.parameters(), lr=lr, betas=(0.5, 0.999))

    def step():
        opt.zero_grad()
        (tm(x, 1.0) * (1.0 / tm.D)).backward()
        opt.step()
    return step


def head_route(m, hid, variant):
    B, z = hid.size(0), m.z_dim
    bufs = [torch.empty(B, z, device="cuda") for _ in range(4)] + [torch.empty(B, device="cuda")]
    packed = m._packed_weights()
    return lambda: L.call("ardae_vae_head", m._desc, m._flat, packed, hid, None, B, 7, 3, None, variant, bufs[0], bufs[1], bufs[2], bufs[3], bufs[4])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--engine-steps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iwae-rounds", type=int, default=3)
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="comma-separated names out of " + ", ".join(SHAPES))
    ap.add_argument("--out", default=None, help="default: profiles/vae_baseline_timing.json (profiles/vae_conv_baseline_timing.json for the conv shape alone)")
    a = ap.parse_args()
    names = a.shapes.split(",")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "vae_conv_baseline_timing.json" if names == ["conv_128x784_z32"] else "vae_baseline_timing.json")
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "engine_steps": a.engine_steps, "repeats": a.repeats, "rounds": a.rounds, "unit": "ms",
           "shapes": {}, "iwae": dict(IWAE, unit="s")}
    for name in names:
        family, B, D, h, z, nl, act = SHAPES[name]
        x = (torch.randn(B, D) if family == "toy" else torch.bernoulli(torch.full((B, D), 0.3))).cuda()
        cfg = net.VaeConfig(lr=1e-4, beta_init=1e-4, beta_fin=1.0, beta_annealing=50000)      # the recipe's ramp: beta read from the device block
        replay, eager = net.VaeEngine(module(family, D, h, z, nl, act), cfg, B), net.VaeEngine(module(family, D, h, z, nl, act), cfg, B, graph=False)
        xr = replay.input_buffer().copy_(x)
        tm = (TorchConvVAE(z, act) if family == "conv" else TorchVAE(family, D, h, z, nl, act)).cuda()
        routes = {"engine_replay": lambda: replay.step(xr), "engine_eager": lambda: eager.step(x), "torch_autograd": torch_loop(tm, x, 1e-4)}
        row = {"B": B, "input_dim": D, "h": h, "z": z, "layers": nl, "act": act}
        row.update(alternate(routes, {"engine_replay": a.engine_steps, "engine_eager": a.steps, "torch_autograd": a.steps}, a.repeats, a.rounds))
        assert replay._graph is not None and eager._graph is None
        m = module(family, D, h, z, nl, act)
        hid = torch.rand(B, h, device="cuda")
        heads = {"head_fused": head_route(m, hid, 1), "head_unfused": head_route(m, hid, 2)}
        row.update(alternate(heads, {k: a.engine_steps for k in heads}, a.repeats, a.rounds))
        row["head_fused_is_default"] = int(L.query("ardae_vae_head_fused_ok", m._desc))
        if family == "conv":
            # (d') what this family's fused head was chosen against: gauss_head_kernel on the same 800-wide rows, reached through a kind-8 descriptor
            # with h_dim 800 (variant 1; its variant 2 = the same five unfused launches), and the family's own head at an unaligned z = 6
            mk = net.MNISTVAE(input_dim=D, h_dim=h, z_dim=z, nonlinearity=act, num_hidden_layers=1).cuda()
            m6 = module(family, D, h, 6, nl, act)
            more = {"gauss_head_kernel_h800": head_route(mk, hid, 1), "gauss_head_kernel_h800_unfused": head_route(mk, hid, 2),
                    "head_fused_z6": head_route(m6, hid, 1), "head_unfused_z6": head_route(m6, hid, 2)}
            row.update(alternate(more, {k: a.engine_steps for k in more}, a.repeats, a.rounds))
            row["head_fused_is_default_z6"] = int(L.query("ardae_vae_head_fused_ok", m6._desc))
        row["replay_over_torch_autograd"] = row["engine_replay"]["median"] / row["torch_autograd"]["median"]
        res["shapes"][name] = row
        print(f"{name}: " + ", ".join(f"{k} {v['median']:.4f} [{v['min']:.4f} .. {v['max']:.4f}]" for k, v in row.items() if isinstance(v, dict)), flush=True)
    # (e) evaluate_iws on the recipe model: the first MNIST-sized shape of the run
    iwae_name = next(n for n in names if SHAPES[n][0] != "toy")
    family, B, D, h, z, nl, act = SHAPES[iwae_name]
    res["iwae"]["shape"] = iwae_name
    m = module(family, D, h, z, nl, act)
    eng = net.VaeEngine(m, net.VaeConfig(), B)
    xs = torch.bernoulli(torch.full((IWAE["images"], D), 0.3)).cuda()
    m.return_samples = False

    def loop():                              # vae.py:352-370
        tot_e = tot_l = 0.0
        for i in range(0, xs.size(0), IWAE["loop_batch"]):
            xb = xs[i:i + IWAE["loop_batch"]]
            with torch.no_grad():
                loss = m(xb)[3]
                lp = m.logprob(xb, sample_size=IWAE["k"])
            tot_e += -loss.item() * xb.size(0)
            tot_l += lp.item() * xb.size(0)
        return tot_e / xs.size(0), tot_l / xs.size(0)
    routes = {"iwae_engine": lambda: eng.evaluate_iws(xs, IWAE["k"]), "iwae_logprob_loop": loop}
    samples = {k: [] for k in routes}
    for fn in routes.values():
        fn()
    for _ in range(a.iwae_rounds):
        for k, fn in routes.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            samples[k].append(s.elapsed_time(e) / 1e3)
    res["iwae"].update({k: spread(v) for k, v in samples.items()})
    res["iwae"]["chunks"] = len(eng._iwae[1].plan(xs.size(0)))
    print("iwae: " + ", ".join(f"{k} {res['iwae'][k]['median']:.4f} s [{res['iwae'][k]['min']:.4f} .. {res['iwae'][k]['max']:.4f}]" for k in routes), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
