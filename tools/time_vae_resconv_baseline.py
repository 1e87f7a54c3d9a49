"""Time the residual-conv Gaussian-posterior baseline (vae.py --model resconv, ardae_model_desc.kind 12) on the device  --  reported, not gated.

    python tools/time_vae_resconv_baseline.py [--steps 100] [--engine-steps 300] [--repeats 3] [--rounds 2] [--out profiles/vae_resconv_baseline_timing.json]

At the recipe shape (128 x 784, z 32, c_dim 450, ELU, no centring; Adam lr 1e-3, beta1 0.9, beta ramp of 50000 steps), milliseconds per call of
  engine_replay / engine_eager   `VaeEngine.step`, the captured unit replayed / the same engine with graph=False
  torch_autograd                 a plain PyTorch autograd loop of the same network (weight-normalised blocks restated with F.conv2d / F.linear,
                                 F.interpolate) with torch.optim.Adam on the same device: the yardstick, not the code under test
  head_fused / head_unfused      the Gaussian head alone (ardae_vae_head variant 1 = gauss_head_kernel / 2) on [128, 450] hidden rows, drawing its eps
  tail_fused / tail_unfused      the decoder's last stage alone (ardae_resconv_tail variant 1 = resconv_tail_kernel / 2 = upsample + the block's launches) at the
                                 evaluator's call shape (8 images x k 256 = 2048 rows) and at R = 128
  decode_2048                    ardae_model_decode of 2048 rows (the decode-only path, fused tail)
and seconds per set of
  iwae_engine / iwae_logprob_loop   `evaluate_iws` on 2048 images at k = 256 against the loop over `model(x)` + `model.logprob(x)` at batch 32 (vae.py:352-370)
Device events around `steps` calls; every route runs one untimed window first; the routes of a group are alternated over `rounds`; `rounds` x `repeats`
figures per route; median [min .. max] are recorded, with the floats per decoded row of the decode-only workspace.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ardae_amd as net  # noqa: E402
from ardae_amd import _lib as L  # noqa: E402
from time_vae_baseline import IWAE, alternate, head_route, spread  # noqa: E402

B, D, Z, C = 128, 784, 32, 450
EVAL_ROWS = 8 * 256


class WN(torch.nn.Module):
    """a weight-normalised operator: scale * direction / ||direction||, bias"""

    def __init__(self, out, inn, conv):
        super().__init__()
        shape = (out, inn, 3, 3) if conv else (out, inn)
        self.direction = torch.nn.Parameter(torch.empty(shape).uniform_(-1, 1) / inn ** 0.5)
        self.scale, self.bias = torch.nn.Parameter(torch.ones(out)), torch.nn.Parameter(torch.zeros(out))

    def weight(self):
        d = self.direction
        view = (-1,) + (1,) * (d.dim() - 1)
        return self.scale.view(view) * d / d.pow(2).flatten(1).sum(1).sqrt().view(view)


class Res(torch.nn.Module):
    def __init__(self, out, inn, conv, stride=1):
        super().__init__()
        self.conv, self.stride = conv, stride
        self.a, self.h, self.s = WN(out, inn, conv), WN(out, out, conv), WN(out, inn, conv)

    def forward(self, x):
        if self.conv:
            hdn = F.elu(F.conv2d(x, self.a.weight(), self.a.bias, self.stride, 1))
            return F.conv2d(hdn, self.h.weight(), self.h.bias, 1, 1) + F.conv2d(x, self.s.weight(), self.s.bias, self.stride, 1)
        hdn = F.relu(F.linear(x, self.a.weight(), self.a.bias))
        return F.linear(hdn, self.h.weight(), self.h.bias) + F.linear(x, self.s.weight(), self.s.bias)


class TorchResConvVAE(torch.nn.Module):
    """models/vae/resconv.py in plain PyTorch for the autograd column."""

    def __init__(self, z, c):
        super().__init__()
        self.D = D
        self.enc = torch.nn.ModuleList([Res(16, 1, True, 2), Res(16, 16, True), Res(32, 16, True, 2), Res(32, 32, True), Res(32, 32, True, 2)])
        self.efc, self.mean, self.logvar = Res(c, 512, False), torch.nn.Linear(c, z), torch.nn.Linear(c, z)
        self.d0, self.d1 = Res(c, z, False), Res(512, c, False)
        self.dec = torch.nn.ModuleList([Res(32, 32, True), Res(32, 32, True), Res(16, 32, True), Res(16, 16, True), Res(1, 16, True)])

    def forward(self, x, beta):
        n = x.size(0)
        up = lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=True)      # noqa: E731
        hdn = x.view(n, 1, 28, 28)
        for blk in self.enc:
            hdn = F.elu(blk(hdn))
        hdn = F.elu(self.efc(hdn.reshape(n, 512)))
        mu, lv = self.mean(hdn), self.logvar(hdn)
        z = mu + torch.exp(0.5 * lv) * torch.randn_like(mu)
        kld = -0.5 * (1 + lv - mu.pow(2) - lv.exp()).sum(1)
        hd = up(F.elu(self.d1(F.elu(self.d0(z)))).view(n, 32, 4, 4))
        hd = F.elu(self.dec[1](F.elu(self.dec[0](hd))))[:, :, :-1, :-1]
        hd = F.elu(self.dec[3](F.elu(self.dec[2](up(hd)))))
        logit = self.dec[4](up(hd)).reshape(n, D)
        rec = F.binary_cross_entropy_with_logits(logit, x, reduction="none").sum(1)
        return (rec + beta * kld).mean()


def torch_loop(tm, x, lr):
    opt = torch.optim.Adam(tm.parameters(), lr=lr, betas=(0.9, 0.999))

    def step():
        opt.zero_grad()
        (tm(x, 1.0) * (1.0 / tm.D)).backward()
        opt.step()
    return step


def tail_route(m, R, variant):
    y = F.elu(torch.randn(R, 14, 14, 16, device="cuda")).contiguous()
    wsf = L.query("ardae_resconv_tail_workspace_floats", m._desc, R, variant)
    ws, out, packed = torch.empty(max(wsf, 64), device="cuda"), torch.empty(R, D, device="cuda"), m._packed_weights()
    return lambda: L.call("ardae_resconv_tail", m._desc, m._flat, packed, y, R, variant, ws, wsf, out)


def module():
    return net.MNISTResConvVAE(z_dim=Z, c_dim=C).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--engine-steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--iwae-rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_resconv_baseline_timing.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "engine_steps": a.engine_steps, "repeats": a.repeats, "rounds": a.rounds, "unit": "ms",
           "shape": {"B": B, "input_dim": D, "z": Z, "c_dim": C, "act": "elu"}, "iwae": dict(IWAE, unit="s")}
    x = torch.bernoulli(torch.full((B, D), 0.3)).cuda()
    cfg = net.VaeConfig(lr=1e-3, beta1=0.9, beta_init=1e-4, beta_fin=1.0, beta_annealing=50000)
    replay, eager = net.VaeEngine(module(), cfg, B), net.VaeEngine(module(), cfg, B, graph=False)
    xr = replay.input_buffer().copy_(x)
    routes = {"engine_replay": lambda: replay.step(xr), "engine_eager": lambda: eager.step(x), "torch_autograd": torch_loop(TorchResConvVAE(Z, C).cuda(), x, 1e-3)}
    res.update(alternate(routes, {"engine_replay": a.engine_steps, "engine_eager": a.steps, "torch_autograd": a.steps}, a.repeats, a.rounds))
    assert replay._graph is not None and eager._graph is None
    res["replay_over_torch_autograd"] = res["engine_replay"]["median"] / res["torch_autograd"]["median"]
    m = module()
    hid = torch.rand(B, C, device="cuda")
    small = {"head_fused": head_route(m, hid, 1), "head_unfused": head_route(m, hid, 2), "tail_fused_128": tail_route(m, 128, 1),
             "tail_unfused_128": tail_route(m, 128, 2)}
    res.update(alternate(small, {k: a.engine_steps for k in small}, a.repeats, a.rounds))
    res["head_fused_is_default"] = int(L.query("ardae_vae_head_fused_ok", m._desc))
    zrows = torch.randn(EVAL_ROWS, Z, device="cuda")
    wsf = L.query("ardae_model_workspace_floats", m._desc, EVAL_ROWS, 1, 2)
    ws, logits = torch.empty(wsf, device="cuda"), torch.empty(EVAL_ROWS, D, device="cuda")
    big = {f"tail_fused_{EVAL_ROWS}": tail_route(m, EVAL_ROWS, 1), f"tail_unfused_{EVAL_ROWS}": tail_route(m, EVAL_ROWS, 2),
           f"decode_{EVAL_ROWS}": lambda: L.call("ardae_model_decode", m._desc, m._flat, m._packed_weights(), zrows, EVAL_ROWS, ws, wsf, logits, None)}
    res.update(alternate(big, {k: a.steps for k in big}, a.repeats, a.rounds))
    res["tail_fused_is_default"] = int(L.query("ardae_resconv_tail_workspace_floats", m._desc, EVAL_ROWS, 0) == 0)
    res["decode_workspace_floats_per_row"] = wsf / EVAL_ROWS
    res["training_carving_floats_per_row"] = L.query("ardae_model_workspace_floats", L.ModelDesc(6, D, 100, C, Z, 1, L.ACT["elu"], 0), EVAL_ROWS, 1, 2) / EVAL_ROWS
    print(", ".join(f"{k} {v['median']:.4f} [{v['min']:.4f} .. {v['max']:.4f}]" for k, v in res.items() if isinstance(v, dict) and "median" in v), flush=True)
    # evaluate_iws on the recipe model
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
    iw = {"iwae_engine": lambda: eng.evaluate_iws(xs, IWAE["k"]), "iwae_logprob_loop": loop}
    samples = {k: [] for k in iw}
    for fn in iw.values():
        fn()
    for _ in range(a.iwae_rounds):
        for k, fn in iw.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            samples[k].append(s.elapsed_time(e) / 1e3)
    res["iwae"].update({k: spread(v) for k, v in samples.items()})
    res["iwae"]["chunks"] = len(eng._iwae[1].plan(xs.size(0)))
    res["iwae"]["groups"] = list(m._eval_groups)
    print("iwae: " + ", ".join(f"{k} {res['iwae'][k]['median']:.4f} s [{res['iwae'][k]['min']:.4f} .. {res['iwae'][k]['max']:.4f}]" for k in iw), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
