"""Golden vectors of the score networks outside the VAE loop (ardae_cdae_desc.kind 2 / 3, 6 / 7, 10 / 11, 13, 16 / 17)  --  TEST INFRASTRUCTURE.

Runs only where the reference checkout is available (it never travels to the GPU box):

    python tools/gen_score_golden.py [--reference DIR] [--family NAME ...] [--only cases|traj|quality]

It imports the reference's own classes through oracle.gen_golden.import_reference() (behind inert stubs for the plotting imports) and stores THEIR
outputs.  FAMILIES below holds what differs between the five families; the layout is common.  <kind> is grad | res: models/graddae/mlp.py and
models/resdae/mlp.py.

  tests/golden/<family prefix>_<kind>_<case>.npz     per kind and shape, (N, d, h, L, act) or (B, S, d, c, h, L, act):
      kind, act, shape
      sd/<name>            the reference's state_dict (default nn.Linear init under a fixed seed; the constructors call no reset_parameters)
      x, [ctx,] std, eps   inputs: x [N, d] or [B, S, d] with ctx [B, 1, c]; std is a scalar (stored in float64) or a tensor, by the case; eps
                           [rows, d] is what the reference drew (seed, call forward, re-seed, redraw randn_like; forward on the injected draw is
                           checked to return the same loss)
      loss, g/<name>       forward(x, [ctx,] std)[1] and every parameter's .grad after loss.backward()  ("g/<name>/none": .grad is None)
      glog, glog0          glogprob, as the family calls it (below)
      loss_f64, g_f64/.., glog_f64      the same calls on the same inputs after .double()
  tests/golden/<family prefix>_traj_<kind>.npz       6 steps of a training loop on injected draws under torch.optim.Adam(lr):  cfg/<name>, kind,
      sd/<name>, and per step s the inputs, <s>/eps, <s>/loss, <s>/p/<name> after the step; the same loop in float64 on the same inputs under
      <s>/loss_f64, <s>/p_f64/<name>.  The unconditional loop is the training cell of notebooks/dae_toy.ipynb: <s>/x [B, d], each row repeated
      nsigma times.  The conditional loop is the cDAE update of ivae_ardae.py:752-779: <s>/latent [B, S, d], <s>/mean [B, d], <s>/ctx [B, c] (one
      context per image), the samples centred, scaled by std_scale and each repeated nsigma times.  A configuration with sigma_annealing has one
      noise level per step, <s>/sigma (the Python float), from sigma_max to sigma_min (the ramp ends inside the run); one with delta has
      std = delta * mean_d std_S(u) * xi per row, <s>/xi [B*S*nsigma].

  ardae          MLPGradARDAE / MLPResARDAE -> ardae_uncond_<kind>_<case>.npz.  std [N, 1]; glog0 = glogprob(x) (std = None: zeros), glog =
                 glogprob(x, std); the float64 keys are loss64, g64/.., glog0_64, glog_64.  The trajectories are in the case files: traj_<opt>/...,
                 6 steps of the training cell of notebooks/ardae_toy.ipynb with torch.optim.RMSprop(lr 1e-3, momentum 0.5) and torch.optim.SGD: per
                 step x, std, eps, the loss, and every parameter after the step.  --only quality:  ardae_uncond_quality.npz, 8 seeds per kind of
                 that cell on x ~ N(0, I_2) (B 256, nsigma 10, delta 1, h 64, 3 layers, softplus, torch.optim.Adam(lr 0.005), 600 steps): mean
                 loss of the last 100 steps and the relative L2 error of glogprob(x_t, s) against the exact score -x_t / (1 + s^2) of the
                 sigma-smoothed Gaussian on 4096 fixed points, s in {.25, .5, 1}
  dae            MLPGradDAE / MLPResDAE -> dae_plain_*: ardae's shapes; std is a scalar in three of the cases; glog = glogprob(x).  Trajectory:
                 B 16 x nsigma 4, d 2, h 64, 3 layers, softplus, lr 0.005, sigma 1.0 to 0.1 with sigma_annealing 4
  cdae_plain     MLPGradCDAE / MLPResCDAE -> cdae_plain_*: std is a scalar in three cases and [B*S, 1] in two; glog = glogprob(x, ctx).
                 Trajectory: B 4 x S 8 x nsigma 2, d 2, c 3, h 48, 2 layers (the parameters are stored 12 times: the file stays under 1 MiB),
                 std_scale 1.5, lr 0.005, annealed sigma
  cardae_noenc   MLPGradCARDAE / MLPResCARDAE with enc_input=False -> cardae_noenc_*: cdae_plain's shapes; std [B, S, 1], always a tensor
                 (ConditionalARDAE asserts one); glog0 = glogprob(x, ctx) (std = 0), glog = glogprob(x, ctx, std).  Trajectory: cdae_plain's
                 widths, delta 0.1, lr 0.001
  recon          the reconstruction DAEs models.MLPDAE = models/dae/mlp.py::DAE -> recon_dae_<case>.npz (ardae's shapes; the noise type
                 alternates) and models.MLPCDAE = models/dae/mlp.py::ConditionalDAE -> recon_cdae_<enc>_<case>.npz, enc = x (enc_input=False) |
                 a (enc_input=True): cdae_plain's shapes and one L = 1 case each, ctx [B, S, c]: one context row PER SAMPLE ROW in half of the
                 cases ("rows" = 1), a [B, 1, c] context repeated over S in the other half ("rows" = 0).  No kind: act, [enc_input, rows,] shape,
                 noise; std is a float >= 0.3 or a tensor with |std| >= 0.05 (the score divides by std^2); `draw` stands for eps: normals, or
                 uniforms in [0, 1) (rand_like); x_recon = forward(x, std)[0]; glog = glogprob(x, [ctx,] std); xbar = add_noise(x, std) on that
                 draw.  Trajectories recon_dae_traj_<noise>.npz (dae's configuration) and recon_cdae_traj_<noise>.npz (MLPCDAE(enc_input=False),
                 cdae_plain's configuration at S 16, nsigma 4), with noise in place of kind and <s>/eps the raw draw

Fixtures hold tensors, names and settings only.
"""
import contextlib
import os

import numpy as np
import torch

from golden_common import GOLDEN, open_reference, widened

KINDS = ("grad", "res")
# name -> (N, d, h, L, act)
SHAPES = {"n64_d2_softplus": (64, 2, 64, 3, "softplus"), "n96_d8_tanh": (96, 8, 64, 3, "tanh"), "n60_d3_elu": (60, 3, 100, 2, "elu"),
          "n64_d2_relu1": (64, 2, 64, 1, "relu"), "n64_d2_swish": (64, 2, 64, 3, "swish")}
SCALAR_STD = {"n64_d2_softplus": 0.5, "n60_d3_elu": 0.3, "n64_d2_swish": None, "n64_d2_relu1": None, "n96_d8_tanh": 1.25}     # None: a [N, 1] tensor
# name -> (B, S, d, c, h, L, act), std (None: a [B*S, 1] tensor)
CSHAPES = {"b4_s16_d2_softplus": ((4, 16, 2, 2, 64, 3, "softplus"), 0.5),
           "b5_s12_d3_elu": ((5, 12, 3, 5, 100, 2, "elu"), None),            # N = 60: a ragged tile
           "b6_s16_d8_tanh": ((6, 16, 8, 24, 64, 2, "tanh"), 1.25),
           "b8_s8_d2_relu1": ((8, 8, 2, 2, 64, 1, "relu"), 0.3),             # L = 1: the encoders are one `fc` each
           "b4_s16_d2_swish": ((4, 16, 2, 3, 64, 3, "swish"), None)}
# recon: name -> noise (in this order; the shapes are SHAPES', the stds SCALAR_STD's)
RECON_NOISE = {"n64_d2_softplus": "gaussian", "n60_d3_elu": "uniform", "n64_d2_swish": "gaussian", "n64_d2_relu1": "uniform", "n96_d8_tanh": "gaussian"}
# recon: name -> (B, S, d, c, h, L, act), std (None: a [B*S, 1] tensor), per-row contexts; enc_input False and True for each; noise alternates over the list
RECON_CSHAPES = {"b4_s16_d2": ((4, 16, 2, 2, 64, 3, "softplus"), 0.5, True),
                 "b5_s12_d3": ((5, 12, 3, 5, 100, 2, "elu"), None, False),           # N = 60: a ragged tile
                 "b4_s16_d2_swish": ((4, 16, 2, 3, 64, 3, "swish"), None, True),
                 "b8_s8_d2_relu1": ((8, 8, 2, 2, 64, 1, "relu"), 0.3, False),        # L = 1: ctx_encode is one Linear
                 "b6_s16_d8_tanh": ((6, 16, 8, 24, 64, 2, "tanh"), 1.25, True),
                 "b3_s20_d3_tanh1": ((3, 20, 3, 4, 32, 1, "tanh"), 0.4, False)}
TRAJ = dict(B=16, nsigma=4, d=2, h=64, L=3, act="softplus", lr=0.005, sigma_max=1.0, sigma_min=0.1, sigma_annealing=4, steps=6)
CTRAJ = dict(B=4, S=8, nsigma=2, d=2, c=3, h=48, L=2, act="softplus", std_scale=1.5, lr=0.005, sigma_max=1.0, sigma_min=0.1, sigma_annealing=4, steps=6)
NOENC_TRAJ = dict(B=4, S=8, nsigma=2, d=2, c=3, h=48, L=2, act="softplus", std_scale=1.5, delta=0.1, lr=0.001, steps=6)
ARDAE_TRAJ_STEPS = 6
ARDAE_OPTIMS = {"rmsprop": lambda ps: torch.optim.RMSprop(ps, lr=1e-3, momentum=0.5), "sgd": lambda ps: torch.optim.SGD(ps, lr=1e-2)}
QUALITY = dict(B=256, nsigma=10, delta=1.0, h=64, L=3, act="softplus", lr=0.005, steps=600, tail=100, seeds=list(range(8)), points=4096,
               levels=(0.25, 0.5, 1.0))


@contextlib.contextmanager
def injected_draw(eps):
    """The next torch.randn_like returns `eps` (the fp64 evaluation must see the fp32 call's draw, not one of its own)."""
    orig = torch.randn_like
    torch.randn_like = lambda t, *a, **k: eps.to(t.dtype)
    try:
        yield
    finally:
        torch.randn_like = orig


@contextlib.contextmanager
def injected_uniform(u):
    """injected_draw's twin for add_uniform_noise: the next torch.rand_like returns `u`."""
    orig = torch.rand_like
    torch.rand_like = lambda t, *a, **k: u.to(t.dtype)
    try:
        yield
    finally:
        torch.rand_like = orig


def injected(noise, draw):
    return injected_draw(draw) if noise == "gaussian" else injected_uniform(draw)


def build(net, cls, shape, **more):
    """The reference class `cls` at a shape (N, d, h, L, act) or (B, S, d, c, h, L, act)"""
    if len(shape) == 7:
        more = dict(more, context_dim=shape[3])
    return getattr(net, cls)(input_dim=shape[-4 if len(shape) == 5 else 2], h_dim=shape[-3], num_hidden_layers=shape[-2], nonlinearity=shape[-1], **more)


def score_class(kind, suffix):
    return f"MLP{'Grad' if kind == 'grad' else 'Res'}{suffix}"


# ---- what differs between the families ------------------------------------------------------------------------------------------------
def half_normal_std(n, g):
    return 0.5 * torch.randn(*n, generator=g)


def floored_std(n, g):
    """[n, 1] with 0.05 <= |std| (the reconstruction DAEs' score divides by std^2)"""
    s = half_normal_std(n, g)
    return torch.where(s.abs() < 0.05, torch.full_like(s, 0.05), s)


def kind_cases(prefix, suffix, base, shapes, **more):
    """-> (file name, seed, case) per kind and shape; the seeds step by 100 per kind and 10 per shape from `base` + 7"""
    for ki, kind in enumerate(KINDS):
        for ci, (name, (shape, std)) in enumerate(shapes.items()):
            yield f"{prefix}_{kind}_{name}", base + 100 * ki + 10 * ci + 7, dict(cls=score_class(kind, suffix), more=more, shape=shape, std=std,
                                                                                 fields={"kind": kind})


def kind_trajs(prefix, suffix, base, t, **more):
    for ki, kind in enumerate(KINDS):
        yield f"{prefix}_traj_{kind}", base + ki, dict(cls=score_class(kind, suffix), more=more, t=t, fields={"kind": kind})


def recon_cases():
    for ci, (name, noise) in enumerate(RECON_NOISE.items()):
        yield f"recon_dae_{name}", 5000 + 10 * ci + 7, dict(cls="MLPDAE", more=dict(noise_type=noise), shape=SHAPES[name], std=SCALAR_STD[name],
                                                            fields={}, noise=noise)
    for ci, (name, (shape, std, per_row)) in enumerate(RECON_CSHAPES.items()):
        for ei, enc_input in enumerate((False, True)):
            noise = ("gaussian", "uniform")[(ci + ei) % 2]
            yield (f"recon_cdae_{'a' if enc_input else 'x'}_{name}", 6000 + 100 * ei + 10 * ci + 7,
                   dict(cls="MLPCDAE", more=dict(noise_type=noise, enc_input=enc_input), shape=shape, std=std, per_row=per_row,
                        fields={"enc_input": int(enc_input), "rows": int(per_row)}, noise=noise))


def recon_trajs():
    for ni, noise in enumerate(("gaussian", "uniform")):
        yield f"recon_dae_traj_{noise}", 7000 + ni, dict(cls="MLPDAE", more=dict(noise_type=noise), t=TRAJ, fields={"noise": noise}, noise=noise)
        yield f"recon_cdae_traj_{noise}", 7100 + ni, dict(cls="MLPCDAE", more=dict(noise_type=noise, enc_input=False), t=dict(CTRAJ, S=16, nsigma=4),
                                                          fields={"noise": noise}, noise=noise)


def recon_inputs(c, g):
    """x, then the std tensor, then ctx: [B, S, c], one row per sample row or one per image repeated over S"""
    shape = c["shape"]
    if len(shape) == 5:
        return (torch.randn(shape[0], shape[1], generator=g),), floored_std((shape[0], 1), g)
    B, S, d, cd = shape[:4]
    x, std = torch.randn(B, S, d, generator=g), floored_std((B * S, 1), g)
    return (x, torch.randn(B, S, cd, generator=g) if c["per_row"] else torch.randn(B, 1, cd, generator=g).expand(B, S, cd).contiguous()), std


def uncond_inputs(c, g):
    N, d = c["shape"][:2]
    return (torch.randn(N, d, generator=g),), half_normal_std((N, 1), g)


def cond_inputs(std_shape):
    def inputs(c, g):
        B, S, d, cd = c["shape"][:4]
        return (torch.randn(B, S, d, generator=g), torch.randn(B, 1, cd, generator=g)), half_normal_std(std_shape(B, S), g)
    return inputs


def ardae_trajectories(dae, sd0, args, g, seed, fx):
    """the training cell of notebooks/ardae_toy.ipynb, 6 steps per optimiser, from the same initial parameters; the inputs go on from the case's"""
    N, d = args[0].shape
    for oname, make in ARDAE_OPTIMS.items():
        dae.load_state_dict(sd0)
        opt = make(dae.parameters())
        fx[f"traj_{oname}/lr"] = np.array(opt.param_groups[0]["lr"])
        for s in range(ARDAE_TRAJ_STEPS):
            xs, ss = torch.randn(N, d, generator=g), 0.5 * torch.randn(N, 1, generator=g)
            opt.zero_grad()
            loss, eps_s = forward_with_draw(dae, "gaussian", (xs,), ss, seed + 10 + s)
            loss.backward()
            opt.step()
            pre = f"traj_{oname}/{s}/"
            fx[pre + "x"], fx[pre + "std"], fx[pre + "eps"], fx[pre + "loss"] = xs.numpy(), ss.numpy(), eps_s.numpy(), loss.detach().numpy()
            for k, v in dae.state_dict().items():
                fx[pre + "p/" + k] = v.numpy().copy()


# cases, trajs: -> (file name, seed, case); inputs(case, generator) -> (x, [ctx]), the std tensor (a case with a scalar std draws and drops it);
# glog(model, x, [ctx,] std) -> {key: glogprob as the family calls it}; f64: the suffixes of the float64 keys of loss / g and of glog;
# recon: the reconstruction DAEs' layout (noise and std after sd/, `draw`, x_recon, xbar); more(model, ...): what else goes into a case file
FAMILIES = {
    "ardae": dict(cases=lambda: kind_cases("ardae_uncond", "ARDAE", 0, {n: (s, None) for n, s in SHAPES.items()}), trajs=lambda: (),
                  inputs=uncond_inputs,
                  glog=lambda m, x, std: {"glog0": m.glogprob(x.clone()), "glog": m.glogprob(x.clone(), std)}, f64=("64", "_64"),
                  more=ardae_trajectories),
    "dae": dict(cases=lambda: kind_cases("dae_plain", "DAE", 1000, {n: (s, SCALAR_STD[n]) for n, s in SHAPES.items()}),
                trajs=lambda: kind_trajs("dae_plain", "DAE", 2000, TRAJ),
                inputs=uncond_inputs,
                glog=lambda m, x, std: {"glog": m.glogprob(x.clone())}),
    "cdae_plain": dict(cases=lambda: kind_cases("cdae_plain", "CDAE", 3000, CSHAPES), trajs=lambda: kind_trajs("cdae_plain", "CDAE", 4000, CTRAJ),
                       inputs=cond_inputs(lambda B, S: (B * S, 1)), glog=lambda m, x, ctx, std: {"glog": m.glogprob(x.clone(), ctx)}),
    "cardae_noenc": dict(cases=lambda: kind_cases("cardae_noenc", "CARDAE", 5000, {n: (s, None) for n, (s, _) in CSHAPES.items()}, enc_input=False),
                         trajs=lambda: kind_trajs("cardae_noenc", "CARDAE", 6000, NOENC_TRAJ, enc_input=False),
                         inputs=cond_inputs(lambda B, S: (B, S, 1)),
                         glog=lambda m, x, ctx, std: {"glog0": m.glogprob(x.clone(), ctx), "glog": m.glogprob(x.clone(), ctx, std.reshape(-1, 1))}),
    "recon": dict(cases=recon_cases, trajs=recon_trajs, inputs=recon_inputs, recon=True,
                  glog=lambda m, *a: {"glog": m.glogprob(*a)}),
}


# ---- the shared machinery ---------------------------------------------------------------------------------------------------------------
def save(name, fx, note):
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **fx)
    print(f"{path}: {os.path.getsize(path)} bytes, {note}")


def forward_with_draw(dae, noise, args, std, seed):
    """(loss, draw [rows, d]): the reference's own draw, recovered by replaying the seed."""
    x = args[0]
    torch.manual_seed(seed)
    _, loss = dae(x.clone(), *args[1:], std)
    torch.manual_seed(seed)
    rows = x.reshape(-1, x.size(-1))
    draw = torch.randn_like(rows) if noise == "gaussian" else torch.rand_like(rows)
    with injected(noise, draw):
        _, again = dae(x.clone(), *args[1:], std)
    assert torch.equal(loss.detach(), again.detach()), "the replayed draw is not the one the reference used"
    return loss, draw


def evaluate(fam, dae, noise, args, std, draw, tag, gtag, fx):
    with injected(noise, draw):
        x_recon, loss = dae(args[0].clone(), *args[1:], std)
    for p in dae.parameters():
        p.grad = None
    loss.backward()
    fx["loss" + tag] = loss.detach().numpy()
    if fam.get("recon"):
        fx["x_recon" + tag] = x_recon.detach().numpy()
    for n, p in dae.named_parameters():
        if p.grad is None:
            fx[f"g{tag}/{n}/none"] = np.zeros(0)
        else:
            fx[f"g{tag}/{n}"] = p.grad.detach().numpy().copy()
    for k, v in fam["glog"](dae, *args, std).items():
        fx[k + gtag] = v.detach().numpy()
    if fam.get("recon"):
        with injected(noise, draw):
            fx["xbar" + tag] = dae.add_noise(args[0].reshape(-1, args[0].size(-1)), std).detach().numpy()


def gen_case(net, fam, name, seed, c):
    shape, noise = c["shape"], c.get("noise", "gaussian")
    tag, gtag = fam.get("f64", ("_f64", "_f64"))
    make = lambda: build(net, c["cls"], shape, **c["more"])      # noqa: E731
    torch.manual_seed(seed)
    dae = make()
    sd0 = {k: v.clone() for k, v in dae.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)
    args, std = fam["inputs"](c, g)
    if c["std"] is not None:
        std = c["std"]
    std_np = std.numpy() if torch.is_tensor(std) else np.array(std, dtype=np.float64)
    fx = {"shape": np.array(shape[:-1]), "act": np.array(shape[-1])}
    fx.update({k: np.array(v) for k, v in c["fields"].items()})
    fx.update(zip(("x", "ctx"), (a.numpy() for a in args)))
    if not fam.get("recon"):
        fx["std"] = std_np
    for k, v in sd0.items():
        fx["sd/" + k] = v.numpy().copy()
    if fam.get("recon"):
        fx["noise"], fx["std"] = np.array(noise), std_np
    loss, draw = forward_with_draw(dae, noise, args, std, seed + 2)
    fx["draw" if fam.get("recon") else "eps"] = draw.numpy()
    evaluate(fam, dae, noise, args, std, draw, "", "", fx)
    assert float(fx["loss"]) == float(loss.detach())
    evaluate(fam, widened(make, sd0), noise, tuple(a.double() for a in args), std.double() if torch.is_tensor(std) else std, draw.double(), tag, gtag, fx)
    if "more" in fam:
        fam["more"](dae, sd0, args, g, seed, fx)
    save(name, fx, f"{noise}, loss {float(fx['loss']):.6f} (fp64 {float(fx['loss' + tag]):.6f})")


def gen_traj(net, name, seed, c):
    """The training cell of notebooks/dae_toy.ipynb, or (a configuration with S) the cDAE update of ivae_ardae.py:752-779: centre and scale the
    samples, repeat each nsigma times, forward at the step's one annealed noise level or at std = delta * mean_d std_S(u) * xi per row, backward,
    torch.optim.Adam; samples, means, contexts, xi and the draws injected."""
    t, noise = c["t"], c.get("noise", "gaussian")
    B, ns, d, S, cd = t["B"], t["nsigma"], t["d"], t.get("S"), t.get("c")
    make = lambda: build(net, c["cls"], (B, S, d, cd, t["h"], t["L"], t["act"]) if S else (B, d, t["h"], t["L"], t["act"]), **c["more"])      # noqa: E731
    torch.manual_seed(seed)
    dae = make()
    sd0 = {k: v.clone() for k, v in dae.state_dict().items()}
    dae64 = widened(make, sd0)
    fx = {"cfg/" + k: np.array(v) for k, v in t.items()}
    fx.update({k: np.array(v) for k, v in c["fields"].items()})
    for k, v in sd0.items():
        fx["sd/" + k] = v.numpy().copy()
    g = torch.Generator().manual_seed(seed + 1)
    opts = [(dae, torch.optim.Adam(dae.parameters(), lr=t["lr"]), torch.float32, ""), (dae64, torch.optim.Adam(dae64.parameters(), lr=t["lr"]), torch.float64, "_f64")]
    for i_ep in range(t["steps"]):
        pre = f"{i_ep}/"
        if S:
            mean = torch.randn(B, d, generator=g)
            latent = mean[:, None, :] + 0.5 * torch.randn(B, S, d, generator=g)
            ctx = torch.randn(B, cd, generator=g)
            fx[pre + "latent"], fx[pre + "mean"], fx[pre + "ctx"] = latent.numpy(), mean.numpy(), ctx.numpy()
        else:
            xb = 0.5 * torch.randn(B, d, generator=g)
            fx[pre + "x"] = xb.numpy()
        rows = B * (S or 1) * ns
        if "delta" in t:
            xi = torch.randn(rows, generator=g)
            fx[pre + "xi"] = xi.numpy()
        draw = torch.randn(rows, d, generator=g) if noise == "gaussian" else torch.rand(rows, d, generator=g)
        fx[pre + "eps"] = draw.numpy()
        if "sigma_annealing" in t:
            perc = min((i_ep + 1) / float(t["sigma_annealing"]), 1.0)
            std = t["sigma_max"] * (1 - perc) + t["sigma_min"] * perc
            fx[pre + "sigma"] = np.array(std, dtype=np.float64)
        for m, opt, dtype, tag in opts:
            if S:
                u = t["std_scale"] * (latent.to(dtype) - mean.to(dtype)[:, None, :])
                if "delta" in t:
                    std = t["delta"] * u.std(dim=1, keepdim=True).mean(dim=2, keepdim=True).expand(B, S * ns, 1) * xi.to(dtype).view(B, S * ns, 1)
                u = u.unsqueeze(2).expand(B, S, ns, d).contiguous().view(B, S * ns, d)
                ctx_rows = ctx.to(dtype).view(B, 1, cd)
                args = (u, ctx_rows.expand(B, S * ns, cd).contiguous() if c["cls"] == "MLPCDAE" else ctx_rows)      # (MLPCDAE takes one context per row)
            else:
                args = (xb.to(dtype).unsqueeze(1).expand(B, ns, d).contiguous().view(B * ns, d),)
            opt.zero_grad()
            with injected(noise, draw):
                _, loss = m(*args, std)
            loss.backward()
            opt.step()
            fx[pre + "loss" + tag] = loss.detach().numpy()
            for k, v in m.state_dict().items():
                fx[f"{pre}p{tag}/{k}"] = v.numpy().copy()
    save(name, fx, f"losses {[round(float(fx[f'{s}/loss']), 5) for s in range(t['steps'])]}")


def gen_quality(net):
    q = QUALITY
    B, ns, d = q["B"], q["nsigma"], 2
    xt = torch.randn(q["points"], d, generator=torch.Generator().manual_seed(12345))
    fx = {k: np.array(v) for k, v in q.items()}
    fx["x_t"] = xt.numpy()
    for kind in KINDS:
        losses, errs = [], []
        for seed in q["seeds"]:
            torch.manual_seed(1000 + seed)
            dae = build(net, score_class(kind, "ARDAE"), (B, d, q["h"], q["L"], q["act"]))
            opt = torch.optim.Adam(dae.parameters(), lr=q["lr"])
            hist = []
            for _ in range(q["steps"]):
                opt.zero_grad()
                x = torch.randn(B, d)
                sigma = q["delta"] * torch.randn(B * ns, 1)
                x = x.unsqueeze(1).expand(B, ns, d).contiguous().view(B * ns, d)
                _, loss = dae(x, sigma)
                loss.backward()
                opt.step()
                hist.append(float(loss))
            losses.append(float(np.mean(hist[-q["tail"]:])))
            row = []
            for s in q["levels"]:
                sc = dae.glogprob(xt.clone(), torch.full((q["points"], 1), s)).detach()
                exact = -xt / (1.0 + s * s)
                row.append(float((sc - exact).norm() / exact.norm()))
            errs.append(row)
            print(kind, seed, losses[-1], row, flush=True)
        fx[f"{kind}/loss"], fx[f"{kind}/score_err"] = np.array(losses), np.array(errs)
    save("ardae_uncond_quality", fx, "8 seeds per kind")


def main():
    chosen, only, net, _ = open_reference(FAMILIES, ["cases", "traj", "quality"])
    for f in chosen:
        fam = FAMILIES[f]
        if only in (None, "cases"):
            for name, seed, c in fam["cases"]():
                gen_case(net, fam, name, seed, c)
        if only in (None, "traj"):
            for name, seed, c in fam["trajs"]():
                gen_traj(net, name, seed, c)
        if only in (None, "quality") and f == "ardae":
            gen_quality(net)


if __name__ == "__main__":
    main()
