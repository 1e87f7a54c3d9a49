"""Time the hierarchical conv Gaussian baseline (vae.py --model auxconv) on the device  --  reported, not gated.

    python tools/time_vae_auxconv_baseline.py [--steps 100] [--engine-steps 300] [--repeats 3] [--rounds 2] [--out profiles/vae_auxconv_baseline_timing.json]

At the recipe shape (128 x 784, z0 100, z 32, softplus), milliseconds per call of
  engine_replay      (a) `VaeEngine.step`, the captured unit replayed (vendored Adam, beta ramp of 50000 steps on the device)
  engine_eager       (b) the same engine with graph=False
  torch_autograd     (c) a plain PyTorch autograd loop of the same network (nn.Conv2d / nn.ConvTranspose2d) with torch.optim.Adam on the same device: the
                         yardstick, not the code under test
  tail_fused_R / tail_unfused_R   the decoder's last two stages alone (ardae_conv_tail variant 1 = conv_tail_kernel / 2 = linear, col2im, linear, col2im) at
                         R = 128 rows and at the evaluator's call shape (g x 256 rows, g = the model's importance-sample group)
  decode_R / decode_unfused_R     ardae_model_decode at the evaluator's call shape with the fused tail, and with ARDAE_CONV_TAIL_UNFUSED=1: the decode call
                         before and after
  iwae_engine / iwae_logprob_loop   `evaluate_iws` on 2048 images at k = 256 against the loop over `model(x)` + `model.logprob(x)` at batch 32
                         (vae.py:352-370); seconds per set
  draw_stage1 / 2 / 3    the three stages of ardae_vae_aux_iwae_draw over the set: the call stopped after its first and second stage
                         (ARDAE_AUX_DRAW_STAGES under ARDAE_DEBUG_KNOBS=1) and whole, differenced; seconds per set
Device events around `steps` calls; every route runs one untimed window first; the routes of a group are alternated over `rounds`;
`rounds` x `repeats` figures per route; median [min .. max] are recorded.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

os.environ["ARDAE_DEBUG_KNOBS"] = "1"      # arms ARDAE_AUX_DRAW_STAGES and ARDAE_CONV_TAIL_UNFUSED (each set only inside its own measurement)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ardae_amd as net  # noqa: E402
from ardae_amd import _lib as L  # noqa: E402
from ardae_amd import rng  # noqa: E402
from time_vae_baseline import alternate, spread  # noqa: E402
from time_vae_resconv_baseline import torch_loop  # noqa: E402

B, D, ND, Z = 128, 784, 100, 32
IWAE = dict(images=2048, k=256, loop_batch=32)


class TorchConvAuxVAE(torch.nn.Module):
    """The same network in plain PyTorch for the autograd column."""

    def __init__(self, nd, z):
        super().__init__()
        nn = torch.nn

        def trunk(extra, out):
            return nn.ModuleList([nn.Conv2d(1, 16, 5, 2, 2), nn.Conv2d(16, 32, 5, 2, 2), nn.Conv2d(32, 32, 5, 2, 2), nn.Linear(512 + extra, 800),
                                  nn.Linear(800, out), nn.Linear(800, out)])
        self.D, self.nd = D, nd
        self.aux, self.enc, self.auxdec = trunk(0, nd), trunk(nd, z), trunk(z, nd)
        self.dec = nn.ModuleList([nn.Linear(z, 300), nn.Linear(300, 512), nn.ConvTranspose2d(32, 32, 5, 2, 2), nn.ConvTranspose2d(32, 16, 5, 2, 2),
                                  nn.ConvTranspose2d(16, 1, 5, 2, 2)])

    @staticmethod
    def stats(net_, x2, s=None):
        hdn = x2
        for conv in net_[:3]:
            hdn = F.softplus(conv(hdn))
        hdn = hdn.reshape(hdn.size(0), -1)
        hdn = F.softplus(net_[3](hdn if s is None else torch.cat([hdn, s], 1)))
        return net_[4](hdn), net_[5](hdn)

    def forward(self, x, beta):
        x2 = (2 * x - 1).view(-1, 1, 28, 28)
        mu0, lv0 = self.stats(self.aux, x2)
        z0 = mu0 + torch.exp(0.5 * lv0) * torch.randn_like(mu0)
        mu, lv = self.stats(self.enc, x2, z0)
        z = mu + torch.exp(0.5 * lv) * torch.randn_like(mu)
        mup, lvp = self.stats(self.auxdec, x2, z)
        kld = -0.5 * (1 + lv - mu.pow(2) - lv.exp()).sum(1)
        aux = -0.5 * (1 - lvp + lv0 - (lv0.exp() + (mu0 - mup).pow(2)) / lvp.exp()).sum(1)
        hd = F.softplus(self.dec[1](F.softplus(self.dec[0](z)))).view(-1, 32, 4, 4)
        hd = F.pad(F.softplus(self.dec[2](hd)), (0, 1, 0, 1))
        logit = self.dec[4](F.softplus(self.dec[3](hd)))[:, :, :28, :28].reshape(-1, D)
        rec = F.binary_cross_entropy_with_logits(logit, x, reduction="none").sum(1)
        return (rec + beta * kld + beta * aux).mean()


def module():
    return net.MNISTConvAuxVAE(z0_dim=ND, z_dim=Z).cuda()


def tail_route(m, R, variant):
    u1 = F.softplus(torch.randn(R, 8, 8, 32, device="cuda"))
    u1[:, 7], u1[:, :, 7] = 0.0, 0.0
    wsf = L.query("ardae_conv_tail_workspace_floats", m._desc, R, variant)
    ws, out, packed = torch.empty(max(wsf, 64), device="cuda"), torch.empty(R, D, device="cuda"), m._packed_weights()
    return lambda: L.call("ardae_conv_tail", m._desc, m._flat, packed, u1, R, variant, ws, wsf, out)


def draw_stages(ev, xs, rounds):
    """The three stages of the draw over the set, on the evaluator's groups: the call stopped after stage 1, after stage 2, and whole, differenced"""
    m, k, g = ev.model, ev.k, ev.group
    b = ev._buffers(ev.plan(xs.size(0))[0][1], xs.device)
    d, flat, packed, ws, seed = m._desc, m._flat, m._packed_weights(), b["ws"], rng.get_state()["seed"]
    ev._encode_stats(b, xs[:g], g)
    upto = {n: [] for n in (1, 2, 3)}
    for r in range(rounds + 1):
        for n in (1, 2, 3):
            os.environ["ARDAE_AUX_DRAW_STAGES"] = str(n)
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i0 in range(0, xs.size(0), g):      # (every group on the first group's statistics: the time does not depend on them)
                L.call("ardae_vae_aux_iwae_draw", d, flat, packed, xs[i0:i0 + g], b["mu"], b["lv"], None, g, k, seed, 3, 4, i0, ws, ws.numel(), b["z"],
                       b["logq"], None)
            e.record()
            torch.cuda.synchronize()
            if r:
                upto[n].append(a.elapsed_time(e) / 1e3)
    del os.environ["ARDAE_AUX_DRAW_STAGES"]
    med = {n: spread(v)["median"] for n, v in upto.items()}
    return {"draw_stage1": med[1], "draw_stage2": med[2] - med[1], "draw_stage3": med[3] - med[2]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--engine-steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--iwae-rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_auxconv_baseline_timing.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "engine_steps": a.engine_steps, "repeats": a.repeats, "rounds": a.rounds, "unit": "ms",
           "shape": {"B": B, "input_dim": D, "z0": ND, "z": Z, "act": "softplus"}, "iwae": dict(IWAE, unit="s")}
    x = torch.bernoulli(torch.full((B, D), 0.3)).cuda()
    cfg = net.VaeConfig(lr=1e-4, beta_init=1e-4, beta_fin=1.0, beta_annealing=50000)
    replay, eager = net.VaeEngine(module(), cfg, B), net.VaeEngine(module(), cfg, B, graph=False)
    xr = replay.input_buffer().copy_(x)
    routes = {"engine_replay": lambda: replay.step(xr), "engine_eager": lambda: eager.step(x), "torch_autograd": torch_loop(TorchConvAuxVAE(ND, Z).cuda(), x, 1e-4)}
    res.update(alternate(routes, {"engine_replay": a.engine_steps, "engine_eager": a.steps, "torch_autograd": a.steps}, a.repeats, a.rounds))
    assert replay._graph is not None and eager._graph is None
    res["replay_over_torch_autograd"] = res["engine_replay"]["median"] / res["torch_autograd"]["median"]
    m = module()
    rows = m._eval_groups[1] * IWAE["k"]
    small = {"tail_fused_128": tail_route(m, 128, 1), "tail_unfused_128": tail_route(m, 128, 2)}
    res.update(alternate(small, {k: a.engine_steps for k in small}, a.repeats, a.rounds))
    zrows, logits = torch.randn(rows, Z, device="cuda"), torch.empty(rows, D, device="cuda")

    def knob(on):      # the library reads the knob at every call (ARDAE_DEBUG_KNOBS armed it at load)
        if on:
            os.environ["ARDAE_CONV_TAIL_UNFUSED"] = "1"
        else:
            os.environ.pop("ARDAE_CONV_TAIL_UNFUSED", None)

    def decode_route(unfused):
        knob(unfused)
        wsf = L.query("ardae_model_workspace_floats", m._desc, rows, 1, 2)
        knob(False)
        ws = torch.empty(wsf, device="cuda")

        def run():
            knob(unfused)
            L.call("ardae_model_decode", m._desc, m._flat, m._packed_weights(), zrows, rows, ws, wsf, logits, None)
            knob(False)
        return run, wsf
    (dec_fused, wsf_fused), (dec_unfused, wsf_unfused) = decode_route(False), decode_route(True)
    big = {f"tail_fused_{rows}": tail_route(m, rows, 1), f"tail_unfused_{rows}": tail_route(m, rows, 2), f"decode_{rows}": dec_fused,
           f"decode_unfused_{rows}": dec_unfused}
    res.update(alternate(big, {k: max(a.steps // 4, 10) for k in big}, a.repeats, a.rounds))
    res["tail_fused_is_default"] = int(L.query("ardae_conv_tail_workspace_floats", m._desc, rows, 0) == 0)
    res["decode_workspace_floats_per_row"], res["decode_unfused_workspace_floats_per_row"] = wsf_fused / rows, wsf_unfused / rows
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
    res["iwae"].update(draw_stages(ev, xs, a.iwae_rounds))
    print("iwae: " + ", ".join(f"{k} {res['iwae'][k]['median']:.4f} s [{res['iwae'][k]['min']:.4f} .. {res['iwae'][k]['max']:.4f}]" for k in iw)
          + ", " + ", ".join(f"{k} {res['iwae'][k]:.5f} s" for k in ("draw_stage1", "draw_stage2", "draw_stage3")), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
