"""Time the auxiliary-variable Gaussian baselines (vae.py --model auxmnist / auxtoy) on the device  --  reported, not gated.

    python tools/time_vae_aux_baseline.py [--steps 200] [--engine-steps 1000] [--repeats 5] [--rounds 3] [--out profiles/vae_aux_baseline_timing.json]

At the recipe shape (auxmnist: 128 x 784, h 300, noise 100, z 32, 2 layers, softplus) and at the toy shape (auxtoy: 1024 x 2, h 64, noise 2, z 2, 1 layer,
tanh), milliseconds per call of
  engine_replay      (a) `VaeEngine.step`, the captured unit replayed (vendored Adam, beta ramp of 50000 steps on the device)
  engine_eager       (b) the same engine with graph=False
  torch_autograd     (c) a plain PyTorch autograd loop of the same network with torch.optim.Adam on the same device: the yardstick, not the
                         code under test
  iwae_engine / iwae_logprob_loop   (d) `evaluate_iws` of the recipe shape on 2048 images at k = 256 against the loop over `model(x)` + `model.logprob(x)` at
                         batch 32 (vae.py:352-370); seconds per set
  iwae_split         (e) where one evaluation pass spends its time, device events around the calls of each chunk, seconds per set: `stats_elbo`
                         (ardae_vae_encode_stats + ardae_vae_aux_elbo_rows), `draw` (ardae_vae_aux_iwae_draw: the three stochastic stages with their
                         two conditional stacks and six head products), `decode_rows` (ardae_model_decode + ardae_model_loss_rows + ardae_iwae_reduce);
                         `draw_stage1 / 2 / 3`: the draw call stopped after its first and second stage (ARDAE_AUX_DRAW_STAGES under
                         ARDAE_DEBUG_KNOBS=1) and whole, differenced; and `stage3_materialised_bytes`, what the third stage moves because it writes mup / lvp [R, noise] and reads them back
Device events around `steps` calls; every route runs one untimed window first; the routes of a group are alternated over `rounds`;
`rounds` x `repeats` figures per route; median [min .. max] are recorded.
"""
import argparse
import json
import os
import sys

import torch

os.environ["ARDAE_DEBUG_KNOBS"] = "1"      # arms ARDAE_AUX_DRAW_STAGES (set only inside iwae_split; no other knob is set here)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ardae_amd as net  # noqa: E402
from ardae_amd import _lib as L  # noqa: E402
from ardae_amd import rng  # noqa: E402
from time_vae_baseline import alternate, spread, torch_loop  # noqa: E402

SHAPES = {"auxmnist_128x784_h300_n100_z32": ("mnist", 128, 784, 300, 100, 32, 2, "softplus"), "auxtoy_1024x2_h64_n2_z2": ("toy", 1024, 2, 64, 2, 2, 1, "tanh")}
IWAE = dict(images=2048, k=256, loop_batch=32)


def module(family, D, h, nd, z, nl, act):
    ctor = net.MNISTAuxVAE if family == "mnist" else net.ToyAuxVAE
    return ctor(input_dim=D, noise_dim=nd, h_dim=h, z_dim=z, nonlinearity=act, num_hidden_layers=nl).cuda()


class TorchAuxVAE(torch.nn.Module):
    """The same network in plain PyTorch (nn.Linear stacks, the reference's loss lines) for the autograd column."""

    def __init__(self, family, D, h, nd, z, nl, act):
        super().__init__()
        nn = torch.nn
        A = {"softplus": nn.Softplus, "tanh": nn.Tanh, "relu": nn.ReLU}[act]

        def stack(w):
            layers = []
            for _ in range(nl):
                layers += [nn.Linear(w, h), A()]
                w = h
            return nn.Sequential(*layers)
        self.family, self.D = family, D
        self.aux, self.mean0, self.logvar0 = stack(D), nn.Linear(h, nd), nn.Linear(h, nd)
        self.enc, self.mean, self.logvar = stack(D + nd), nn.Linear(h, z), nn.Linear(h, z)
        self.auxdec, self.meanp, self.logvarp = stack(D + z), nn.Linear(h, nd), nn.Linear(h, nd)
        self.dec, self.out = stack(z), nn.Linear(h, D)
        self.out_lv = nn.Linear(h, D) if family == "toy" else None

    def forward(self, x, beta):
        xs = 2 * x - 1 if self.family == "mnist" else x
        h0 = self.aux(xs)
        mu0, lv0 = self.mean0(h0), self.logvar0(h0)
        z0 = mu0 + torch.exp(0.5 * lv0) * torch.randn_like(mu0)
        hdn = self.enc(torch.cat([xs, z0], 1))
        mu, lv = self.mean(hdn), self.logvar(hdn)
        z = mu + torch.exp(0.5 * lv) * torch.randn_like(mu)
        hr = self.auxdec(torch.cat([xs, z], 1))
        mup, lvp = self.meanp(hr), self.logvarp(hr)
        kld = -0.5 * (1 + lv - mu.pow(2) - lv.exp()).sum(1)
        aux = -0.5 * (1 - lvp + lv0 - (lv0.exp() + (mu0 - mup).pow(2)) / lvp.exp()).sum(1)
        hd = self.dec(z)
        if self.family == "mnist":
            rec = torch.nn.functional.binary_cross_entropy_with_logits(self.out(hd), x, reduction="none").sum(1)
        else:
            m, l = self.out(hd), self.out_lv(hd)
            rec = 0.5 * (l + (x - m) ** 2 / l.exp() + 1.8378770664093453).sum(1)
        return (rec + beta * kld + beta * aux).mean()


def iwae_split(ev, xs, rounds):
    """One evaluation pass, chunk by chunk as GaussianIwaeEvaluator._evaluate_rows_aux makes it, with device events around each phase"""
    m, k = ev.model, ev.k
    N = xs.size(0)
    chunks = ev.plan(N)
    b = ev._buffers(chunks[0][1] - chunks[0][0], xs.device)
    d, flat, packed, ws = m._desc, m._flat, m._packed_weights(), b["ws"]
    recon, kld, out = (torch.empty(N, device=xs.device) for _ in range(3))
    seed = rng.get_state()["seed"]
    samples = {"stats_elbo": [], "draw": [], "decode_rows": []}
    for r in range(rounds + 1):
        marks = []
        for i0, i1 in chunks:
            c, xc = i1 - i0, xs[i0:i1]
            ev4 = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev4[0].record()
            ev._encode_stats(b, xc, c)
            L.call("ardae_vae_aux_elbo_rows", d, flat, packed, xc, None, c, seed, 1, 2, i0, ws, ws.numel(), recon[i0:i1], kld[i0:i1])
            ev4[1].record()
            L.call("ardae_vae_aux_iwae_draw", d, flat, packed, xc, b["mu"], b["lv"], None, c, k, seed, 3, 4, i0, ws, ws.numel(), b["z"], b["logq"], None)
            ev4[2].record()
            ev._decode_rows(b, xc, b["z"], c, k, b["rec"], ev.group)
            L.call("ardae_iwae_reduce", b["rec"], b["pri"], b["logq"], c, k, out[i0:i1])
            ev4[3].record()
            marks.append(ev4)
        torch.cuda.synchronize()
        if r == 0:
            continue                                     # one untimed pass
        for j, key in enumerate(samples):
            samples[key].append(sum(e[j].elapsed_time(e[j + 1]) for e in marks) / 1e3)
    out = {key: spread(v) for key, v in samples.items()}
    # the three stages of the draw: the call stopped after stage 1, after stage 2, and whole (ARDAE_AUX_DRAW_STAGES), differenced
    upto = {n: [] for n in (1, 2, 3)}
    for r in range(rounds + 1):
        for n in (1, 2, 3):
            os.environ["ARDAE_AUX_DRAW_STAGES"] = str(n)
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i0, i1 in chunks:
                L.call("ardae_vae_aux_iwae_draw", d, flat, packed, xs[i0:i1], b["mu"], b["lv"], None, i1 - i0, k, seed, 3, 4, i0, ws, ws.numel(), b["z"],
                       b["logq"], None)
            e.record()
            torch.cuda.synchronize()
            if r:
                upto[n].append(a.elapsed_time(e) / 1e3)
    del os.environ["ARDAE_AUX_DRAW_STAGES"]
    med = {n: spread(v)["median"] for n, v in upto.items()}
    out["draw_stage1"], out["draw_stage2"], out["draw_stage3"] = med[1], med[2] - med[1], med[3] - med[2]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--engine-steps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iwae-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_aux_baseline_timing.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "engine_steps": a.engine_steps, "repeats": a.repeats, "rounds": a.rounds, "unit": "ms",
           "shapes": {}, "iwae": dict(IWAE, unit="s")}
    for name, (family, B, D, h, nd, z, nl, act) in SHAPES.items():
        x = (torch.randn(B, D) if family == "toy" else torch.bernoulli(torch.full((B, D), 0.3))).cuda()
        cfg = net.VaeConfig(lr=1e-4, beta_init=1e-4, beta_fin=1.0, beta_annealing=50000)      # the recipe's ramp: beta read from the device block
        replay = net.VaeEngine(module(family, D, h, nd, z, nl, act), cfg, B)
        eager = net.VaeEngine(module(family, D, h, nd, z, nl, act), cfg, B, graph=False)
        xr = replay.input_buffer().copy_(x)
        tm = TorchAuxVAE(family, D, h, nd, z, nl, act).cuda()
        routes = {"engine_replay": lambda: replay.step(xr), "engine_eager": lambda: eager.step(x), "torch_autograd": torch_loop(tm, x, 1e-4)}
        row = {"B": B, "input_dim": D, "h": h, "noise": nd, "z": z, "layers": nl, "act": act}
        row.update(alternate(routes, {"engine_replay": a.engine_steps, "engine_eager": a.steps, "torch_autograd": a.steps}, a.repeats, a.rounds))
        assert replay._graph is not None and eager._graph is None
        row["replay_over_torch_autograd"] = row["engine_replay"]["median"] / row["torch_autograd"]["median"]
        res["shapes"][name] = row
        print(f"{name}: " + ", ".join(f"{k} {v['median']:.4f} [{v['min']:.4f} .. {v['max']:.4f}]" for k, v in row.items() if isinstance(v, dict)), flush=True)
    # (d) evaluate_iws on the recipe model
    iwae_name = next(iter(SHAPES))
    family, B, D, h, nd, z, nl, act = SHAPES[iwae_name]
    res["iwae"]["shape"] = iwae_name
    m = module(family, D, h, nd, z, nl, act)
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
    ev = eng._iwae[1]
    res["iwae"]["chunks"] = len(ev.plan(xs.size(0)))
    res["iwae"]["engine_over_loop"] = res["iwae"]["iwae_engine"]["median"] / res["iwae"]["iwae_logprob_loop"]["median"]
    print("iwae: " + ", ".join(f"{k} {res['iwae'][k]['median']:.4f} s [{res['iwae'][k]['min']:.4f} .. {res['iwae'][k]['max']:.4f}]" for k in routes), flush=True)
    split = iwae_split(ev, xs, a.iwae_rounds)
    # stage 3 writes mup and lvp [R, noise] and reads them back once: 4 passes over R x noise floats
    split["stage3_materialised_bytes"] = 4 * IWAE["images"] * IWAE["k"] * nd * 4
    res["iwae"]["iwae_split"] = split
    print("iwae split: " + ", ".join(f"{k} {v['median'] if isinstance(v, dict) else v:.5f} s" for k, v in split.items() if not isinstance(v, int)), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
