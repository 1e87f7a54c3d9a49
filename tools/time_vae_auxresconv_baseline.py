"""Time the hierarchical resconv Gaussian baseline (vae.py --model auxresconvct) on the device  --  reported, not gated.

    python tools/time_vae_auxresconv_baseline.py [--steps 100] [--engine-steps 300] [--repeats 3] [--rounds 2] [--out profiles/vae_auxresconv_baseline_timing.json]
    python tools/time_vae_auxresconv_baseline.py --decode-only 12|19      (one ardae_model_decode at 2048 rows after a warm-up: the kernel-trace runs)

At the counterpart recipe's shape (128 x 784, z0 100, z 32, c_dim 450, centred, ELU), milliseconds per call of
  engine_replay      (a) `VaeEngine.step`, the captured unit replayed (vendored Adam 1e-3 / beta1 0.9, beta ramp of 50000 steps on the device)
  engine_eager       (b) the same engine with graph=False
  torch_autograd     (c) a plain PyTorch autograd loop of the same network (weight-normalised residual blocks on F.conv2d / F.linear) with torch.optim.Adam
                         on the same device: the yardstick, not the code under test
  mid_fused_R / mid_unfused_R     the decoder's 14 x 14 stage alone (ardae_resconv_mid variant 1 = resconv_mid_kernel / 2 = the ten launches) at R = 128
                         rows and at the evaluator's call shape (g x 256 rows, g = the model's importance-sample group)
  decode19_R / decode12_R / decode19_unfused_R     ardae_model_decode of kind 19, of kind 12 on the same rows and the same decoder weights (the path
                         before this kernel), and of kind 19 with ARDAE_RESCONV_MID_UNFUSED=1, alternated in the same call
  iwae_engine / iwae_logprob_loop   `evaluate_iws` on 2048 images at k = 256 against the loop over `model(x)` + `model.logprob(x)` at batch 32
                         (vae.py:352-370); seconds per set
  draw_stage1 / 2 / 3    the three stages of ardae_vae_aux_iwae_draw over the set (time_vae_auxconv_baseline.draw_stages); seconds per set
Device events around `steps` calls; every route runs one untimed window first; the routes of a group are alternated over `rounds`;
`rounds` x `repeats` figures per route; median [min .. max] are recorded.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

os.environ["ARDAE_DEBUG_KNOBS"] = "1"      # arms ARDAE_AUX_DRAW_STAGES and ARDAE_RESCONV_MID_UNFUSED (each set only inside its own measurement)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ardae_amd as net  # noqa: E402
from ardae_amd import _lib as L  # noqa: E402
from time_vae_baseline import alternate, spread  # noqa: E402
from time_vae_resconv_baseline import Res, torch_loop  # noqa: E402
from time_vae_auxconv_baseline import draw_stages  # noqa: E402

B, D, ND, Z, C = 128, 784, 100, 32, 450
IWAE = dict(images=2048, k=256, loop_batch=32)


class TorchResConvAuxVAE(torch.nn.Module):
    """models/vae/auxresconv.py in plain PyTorch for the autograd column."""

    def __init__(self, nd, z, c):
        super().__init__()
        nn = torch.nn
        self.D = D
        self.enc = nn.ModuleList([Res(16, 1, True, 2), Res(16, 16, True), Res(32, 16, True, 2), Res(32, 32, True), Res(32, 32, True, 2)])
        self.efc = Res(c, 512, False)
        self.mean0, self.logvar0 = nn.Linear(c, nd), nn.Linear(c, nd)
        self.fc, self.mean, self.logvar = nn.Linear(c + nd, c), nn.Linear(c, z), nn.Linear(c, z)
        self.rfc, self.meanp, self.logvarp = nn.Linear(c + z, c), nn.Linear(c, nd), nn.Linear(c, nd)
        self.d0, self.d1 = Res(c, z, False), Res(512, c, False)
        self.dec = nn.ModuleList([Res(32, 32, True), Res(32, 32, True), Res(16, 32, True), Res(16, 16, True), Res(1, 16, True)])

    def forward(self, x, beta):
        n = x.size(0)
        up = lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=True)      # noqa: E731
        hdn = (2 * x - 1).view(n, 1, 28, 28)
        for blk in self.enc:
            hdn = F.elu(blk(hdn))
        ctx = F.elu(self.efc(hdn.reshape(n, 512)))
        mu0, lv0 = self.mean0(ctx), self.logvar0(ctx)
        z0 = mu0 + torch.exp(0.5 * lv0) * torch.randn_like(mu0)
        h = F.elu(self.fc(torch.cat([ctx, z0], 1)))
        mu, lv = self.mean(h), self.logvar(h)
        z = mu + torch.exp(0.5 * lv) * torch.randn_like(mu)
        hr = F.elu(self.rfc(torch.cat([ctx, z], 1)))
        mup, lvp = self.meanp(hr), self.logvarp(hr)
        kld = -0.5 * (1 + lv - mu.pow(2) - lv.exp()).sum(1)
        aux = -0.5 * (1 - lvp + lv0 - (lv0.exp() + (mu0 - mup).pow(2)) / lvp.exp()).sum(1)
        hd = up(F.elu(self.d1(F.elu(self.d0(z)))).view(n, 32, 4, 4))
        hd = F.elu(self.dec[1](F.elu(self.dec[0](hd))))[:, :, :-1, :-1]
        hd = F.elu(self.dec[3](F.elu(self.dec[2](up(hd)))))
        logit = self.dec[4](up(hd)).reshape(n, D)
        rec = F.binary_cross_entropy_with_logits(logit, x, reduction="none").sum(1)
        return (rec + beta * kld + beta * aux).mean()


def module():
    return net.MNISTResConvAuxVAE(z0_dim=ND, z_dim=Z, c_dim=C, do_center=True).cuda()


def module12(m19):
    """kind 12 with kind 19's decoder weights"""
    m = net.MNISTResConvVAE(z_dim=Z, c_dim=C).cuda()
    sd = m.state_dict()
    sd.update({k: v for k, v in m19.state_dict().items() if k.startswith("decode.")})
    m.load_state_dict(sd)
    return m


def mid_route(m, R, variant):
    y8 = F.elu(torch.randn(R, 8, 8, 32, device="cuda")).contiguous()
    wsf = L.query("ardae_resconv_mid_workspace_floats", m._desc, R, variant)
    ws, out, packed = torch.empty(max(wsf, 64), device="cuda"), torch.empty(R, 196 * 16, device="cuda"), m._packed_weights()
    return lambda: L.call("ardae_resconv_mid", m._desc, m._flat, packed, y8, R, variant, ws, wsf, out)


def knob(on):      # the library reads the knob at every call (ARDAE_DEBUG_KNOBS armed it at load)
    if on:
        os.environ["ARDAE_RESCONV_MID_UNFUSED"] = "1"
    else:
        os.environ.pop("ARDAE_RESCONV_MID_UNFUSED", None)


def decode_route(m, rows, unfused=False):
    zrows, logits = torch.randn(rows, Z, device="cuda", generator=torch.Generator("cuda").manual_seed(1)), torch.empty(rows, D, device="cuda")
    knob(unfused)
    wsf = L.query("ardae_model_workspace_floats", m._desc, rows, 1, 2)
    knob(False)
    ws = torch.empty(wsf, device="cuda")

    def run():
        knob(unfused)
        L.call("ardae_model_decode", m._desc, m._flat, m._packed_weights(), zrows, rows, ws, wsf, logits, None)
        knob(False)
    return run, wsf


def decode_only(kind):
    """one decode call at 2048 rows behind two warm-up calls: what the kernel-trace runs execute"""
    torch.manual_seed(0)
    m19 = module()
    run, _ = decode_route(m19 if kind == 19 else module12(m19), 2048)
    for _ in range(3):
        run()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--engine-steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--iwae-rounds", type=int, default=2)
    ap.add_argument("--decode-only", type=int, choices=[12, 19])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_auxresconv_baseline_timing.json"))
    a = ap.parse_args()
    if a.decode_only:
        return decode_only(a.decode_only)
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "engine_steps": a.engine_steps, "repeats": a.repeats, "rounds": a.rounds, "unit": "ms",
           "shape": {"B": B, "input_dim": D, "z0": ND, "z": Z, "c_dim": C, "act": "elu", "do_center": 1}, "iwae": dict(IWAE, unit="s")}
    x = torch.bernoulli(torch.full((B, D), 0.3)).cuda()
    cfg = net.VaeConfig(lr=1e-3, beta1=0.9, beta_init=1e-4, beta_fin=1.0, beta_annealing=50000)
    replay, eager = net.VaeEngine(module(), cfg, B), net.VaeEngine(module(), cfg, B, graph=False)
    xr = replay.input_buffer().copy_(x)
    routes = {"engine_replay": lambda: replay.step(xr), "engine_eager": lambda: eager.step(x),
              "torch_autograd": torch_loop(TorchResConvAuxVAE(ND, Z, C).cuda(), x, 1e-3)}
    res.update(alternate(routes, {"engine_replay": a.engine_steps, "engine_eager": a.steps, "torch_autograd": a.steps}, a.repeats, a.rounds))
    assert replay._graph is not None and eager._graph is None
    res["replay_over_torch_autograd"] = res["engine_replay"]["median"] / res["torch_autograd"]["median"]
    m = module()
    m12 = module12(m)
    rows = m._eval_groups[1] * IWAE["k"]
    for R, steps in ((128, a.engine_steps), (rows, max(a.steps // 4, 10))):
        (d19, w19), (d12, w12), (d19u, w19u) = decode_route(m, R), decode_route(m12, R), decode_route(m, R, True)
        group = {f"mid_fused_{R}": mid_route(m, R, 1), f"mid_unfused_{R}": mid_route(m, R, 2), f"decode19_{R}": d19, f"decode12_{R}": d12,
                 f"decode19_unfused_{R}": d19u}
        res.update(alternate(group, {k: steps for k in group}, a.repeats, a.rounds))
        res[f"mid_fused_over_unfused_{R}"] = res[f"mid_fused_{R}"]["median"] / res[f"mid_unfused_{R}"]["median"]
        res[f"decode19_over_decode12_{R}"] = res[f"decode19_{R}"]["median"] / res[f"decode12_{R}"]["median"]
        if R == rows:
            res["decode19_workspace_floats_per_row"], res["decode12_workspace_floats_per_row"] = w19 / R, w12 / R
            res["decode19_unfused_workspace_floats_per_row"] = w19u / R
        del d19, d12, d19u, group
        torch.cuda.empty_cache()
    res["mid_fused_is_default"] = int(L.query("ardae_resconv_mid_workspace_floats", m._desc, rows, 0) == 0)
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
    ev = eng._iwae[1]
    res["iwae"]["chunks"] = len(ev.plan(xs.size(0)))
    res["iwae"]["groups"] = list(m._eval_groups)
    res["iwae"]["engine_over_loop"] = res["iwae"]["iwae_engine"]["median"] / res["iwae"]["iwae_logprob_loop"]["median"]
    res["iwae"]["floats_per_decoded_row"] = res["decode19_workspace_floats_per_row"]
    res["iwae"].update(draw_stages(ev, xs, a.iwae_rounds))
    print("iwae: " + ", ".join(f"{k} {res['iwae'][k]['median']:.4f} s [{res['iwae'][k]['min']:.4f} .. {res['iwae'][k]['max']:.4f}]" for k in iw)
          + ", " + ", ".join(f"{k} {res['iwae'][k]:.5f} s" for k in ("draw_stage1", "draw_stage2", "draw_stage3")), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
