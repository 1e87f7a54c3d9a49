"""What the GPU tests of the six Gaussian VAE families (tests/test_vae_{,conv_,resconv_,aux_,auxconv_,auxresconv_}baseline_gpu.py) share, written once:
the tolerances, NaN-filled buffers with guard rows, the C ABI's forward / backward on them, the gradient comparisons, and the bodies of the tests
every family has - forward / backward against the reference, other shapes against the float64 restatement, the engine's trajectory, replay == eager
and resume, IWAE evaluation - as functions of a `Family` record that says what differs.  Not a test module: nothing here is collected, so every
assertion carries its message.

Tolerances are the project's for these quantities (tests/test_engine_gpu.py, tests/test_iwae_eval_gpu.py): scalar losses 1e-4 relative, recon / kld
means 2e-5, gradients 2e-3 relative L2 per tensor, updated parameters 5e-3 relative L2, IWAE log-probability 1e-4 against the float64 fixture,
latents (and logits) 1e-5 relative L2."""
import dataclasses
from typing import Callable, Optional

import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import rng
from vae_restate import BETAS, load, rel, summary_err, t64, traj_config  # noqa: F401  (traj_config: re-exported)

DEV = "cuda"
NAN = float("nan")
TOL_LOSS, TOL_MEAN, TOL_GRAD, TOL_PARAM, TOL_IWAE, TOL_LATENT = 1e-4, 2e-5, 2e-3, 5e-3, 1e-4, 1e-5
HEAD_KEYS = ("mu", "lv", "z", "eps", "kld")


def relerr(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def cuda(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV).contiguous()


def np64(t):
    return t.detach().double().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)


@dataclasses.dataclass
class Family:
    """What differs between the families in the shared bodies below"""
    from_fixture: Callable                 # fx -> the module on the device, with the fixture's parameters
    restate: Callable                      # fx -> (float64 parameters, cfg): what the restatement below takes first
    loss_and_grads: Callable               # (p, cfg, x, eps, beta, scale=) -> forward's dict, {name: gradient} in float64
    logprob_rows: Callable                 # (p, cfg, x, eps [B, k, w]) -> [B]
    to64: Callable = t64                   # a tensor or array -> what the restatement computes on (t64, or np64 for the numpy restatement)
    aux: bool = False                      # the auxiliary-variable models: eps is [eps0 | eps], encode_stats gives aux_encode's mu0 / lv0 [B, noise_dim]
    image: bool = False                    # feeds the module [B, 1, 28, 28] where the family's tests did ([B, D] otherwise)
    fixture_grads: str = "full"            # "full": g/ in full, gs/ as summaries (check_grads); "norm": g/ in full, the L2 norm of gs/ (check_grads_fixture)
    grads64: bool = False                  # gradients against the float64 restatement: check_grads64, and also in the fixture test (else check_grads)
    traj: str = "ps"                       # the trajectory fixture's parameters: "p" in full, "ps" as summaries, "restate": trajectory(fx) in float64
    trajectory: Optional[Callable] = None  # traj == "restate": fx -> the float64 loop
    head_fused: Optional[int] = None       # ardae_vae_head_fused_ok of the fixtures' descriptors, where the family states it
    logprob_is_evaluator: bool = False     # model.logprob_rows equals the evaluator's rows to the bit (kinds 11, 12 at the fixtures' B)

    def p64_of(self, m):
        return {k: self.to64(v) for k, v in m.named_parameters()}

    def inp(self, x):
        return x.view(x.size(0), 1, 28, 28) if self.image else x


# ---- NaN-filled buffers with guard rows ---------------------------------------------------------------------------------------------------
def guarded(rows, cols, extra=3):
    """[rows + extra, cols] of NaN: the call may write the first `rows` rows only"""
    return torch.full((rows + extra, cols), NAN, device=DEV)


def check_guard(buf, rows, what):
    assert bool(torch.isfinite(buf[:rows]).all()), f"{what}: a row below B was not written"
    assert bool(torch.isnan(buf[rows:]).all()), f"{what}: a row past B was written"


def nan_workspace(floats, slack=4096):
    """A NaN-filled workspace with `slack` floats behind its declared end"""
    return torch.full((floats + slack,), NAN, device=DEV)


def check_workspace(ws, floats, what):
    assert bool(torch.isnan(ws[floats:]).all()), f"{what}: written past the workspace's declared end"


def abi_forward_backward(m, x, eps, beta, loss_scale, grads_beta=0.0, grads=None, seed=0, offset=0):
    """-> z, losses [3], flat grads, eps_out through ardae_vae_forward / ardae_vae_backward on NaN-filled buffers: the workspace, every output, and
    guard rows behind each of them (and behind the workspace's declared end).  eps None: the call draws at (seed, offset).  grads with
    grads_beta: what the backward accumulates onto."""
    B, n = x.size(0), m._flat.numel()
    wsf = L.query("ardae_model_workspace_floats", m._desc, B, 1, 1)
    ws = nan_workspace(wsf)
    zo, eo, losses = guarded(B, m.z_dim), guarded(B, m._eps_width), guarded(3, 1)
    L.call("ardae_vae_forward", m._desc, m._flat, m._packed_weights(), x, eps, B, beta, loss_scale, seed, offset, None, ws, wsf, zo, eo, losses)
    g = torch.full((n + 64,), NAN, device=DEV)          # (grads_beta 0: whatever was there is overwritten)
    if grads is not None:
        g[:n] = grads
    L.call("ardae_vae_backward", m._desc, m._flat, m._packed_weights(), x, B, beta, loss_scale, ws, wsf, g, grads_beta)
    for buf, rows, what in ((zo, B, "z_out"), (eo, B, "eps_out"), (losses, 3, "losses")):
        check_guard(buf, rows, what)
    check_workspace(ws, wsf, "forward / backward")
    assert bool(torch.isnan(g[n:]).all()) and bool(torch.isfinite(g[:n]).all()), "grads: written past the parameters, or not written"
    assert eps is None or torch.equal(eo[:B], eps), "eps_out is not the injected eps"
    return zo[:B].clone(), losses[:3, 0].clone(), g[:n].clone(), eo[:B].clone()


def abi_encode_stats(m, x, width, what=("mu_out", "lv_out")):
    """-> the two statistics [B, width] of ardae_vae_encode_stats on NaN-filled buffers with guard rows"""
    B = x.size(0)
    wsf = L.query("ardae_model_workspace_floats", m._desc, B, 1, 0)
    ws, mu, lv = nan_workspace(wsf), guarded(B, width), guarded(B, width)
    L.call("ardae_vae_encode_stats", m._desc, m._flat, m._packed_weights(), x, B, ws, wsf, mu, lv)
    check_guard(mu, B, what[0]), check_guard(lv, B, what[1])
    check_workspace(ws, wsf, "encode_stats")
    return mu[:B].clone(), lv[:B].clone()


def abi_decode(m, z, what="decode out0", slack=4096):
    """-> logits [R, 784] of ardae_model_decode on NaN-filled buffers with guard rows, and the workspace it left"""
    R = z.size(0)
    wsf = L.query("ardae_model_workspace_floats", m._desc, R, 1, 2)
    ws, out = nan_workspace(wsf, slack), guarded(R, 784)
    L.call("ardae_model_decode", m._desc, m._flat, m._packed_weights(), z, R, ws, wsf, out, None)
    check_guard(out, R, what)
    check_workspace(ws, wsf, what)
    return out[:R].clone(), ws


def abi_stage(entry, m, inp, variant, cols, what, expect_ws=None):
    """-> the first R rows [R, cols] of one decoder stage on its own (ardae_resconv_tail, ardae_resconv_mid, ardae_conv_tail: `entry`, with
    <entry>_workspace_floats) on NaN-filled buffers, guard rows checked behind the output and the workspace"""
    R = inp.size(0)
    wsf = L.query(entry + "_workspace_floats", m._desc, R, variant)
    assert expect_ws is None or (wsf > 0) == expect_ws, (what, variant, wsf)
    ws, out = nan_workspace(wsf), guarded(R, cols)
    L.call(entry, m._desc, m._flat, m._packed_weights(), inp, R, variant, ws, wsf, out)
    check_guard(out, R, f"{what} variant {variant}")
    check_workspace(ws, wsf, f"{what} variant {variant}")
    return out[:R].clone()


def head(m, hid, variant, eps=None, seed=123, offset=5):
    """-> {mu, lv, z, eps [B, z], kld [B]} of ardae_vae_head on guarded buffers"""
    B, z = hid.size(0), m.z_dim
    out = {k: guarded(B, z) for k in ("mu", "lv", "z", "eps")}
    out["kld"] = guarded(B, 1)
    L.call("ardae_vae_head", m._desc, m._flat, m._packed_weights(), hid, eps, B, seed, offset, None, variant, out["mu"], out["lv"], out["z"], out["eps"],
           out["kld"])
    for k, v in out.items():
        check_guard(v, B, f"head variant {variant} {k}")
    return {k: (v[:B, 0] if k == "kld" else v[:B]).clone() for k, v in out.items()}


def head64(m, hid):
    """-> mu, lv of the Gaussian head on the hidden rows `hid`, in float64 on the host"""
    p, hd = {k: t64(v) for k, v in m.named_parameters()}, t64(hid)
    return (hd @ p["encode.reparam.mean_fn.weight"].t() + p["encode.reparam.mean_fn.bias"],
            hd @ p["encode.reparam.logvar_fn.weight"].t() + p["encode.reparam.logvar_fn.bias"])


def check_head64(out, mu, lv, used, what):
    """one head call's mu / lv / z / kld against float64 on the host, on the draw `used`"""
    assert rel(out["mu"].cpu(), mu) <= TOL_LATENT and rel(out["lv"].cpu(), lv) <= TOL_LATENT, (what, "mu / lv")
    assert rel(out["z"].cpu(), mu + torch.exp(0.5 * lv) * t64(used)) <= TOL_LATENT, (what, "z")
    assert rel(out["kld"].cpu(), -0.5 * (1 + lv - mu ** 2 - lv.exp()).sum(1)) <= TOL_MEAN, (what, "kld")


def philox_normal(shape, seed, offset, first=0):
    """-> the library's normal draw of that shape at (seed, offset), from element `first`"""
    out = torch.empty(*shape, device=DEV)
    L.call("ardae_philox_normal_at", out, out.numel(), seed, offset, None, first)
    return out


def aux_draws(B, nd, zd, seed, offset):
    """-> [eps0 | eps] as the auxiliary models' forward draws them: B nd normals, then B zd from the next whole Philox counter"""
    return torch.cat([philox_normal((B, nd), seed, offset), philox_normal((B, zd), seed, offset, (B * nd + 3) // 4 * 4)], 1)


def aux_iwae_draw(m, x, eps):
    """-> z [B k, z_dim], logq [B k] of ardae_vae_aux_iwae_draw on the injected draws eps [B, k, noise + z] (x, eps on the host), on NaN-filled
    buffers with guard rows; eps_out must be eps"""
    B, k, w = eps.shape
    rows = B * k
    mu0, lv0 = m.encode_stats(x.to(DEV))
    z, logq, eps_out = guarded(rows, m.z_dim), guarded(rows, 1), guarded(rows, w)
    wsf = L.query("ardae_model_workspace_floats", m._desc, B, k, 4)
    ws = nan_workspace(wsf)
    L.call("ardae_vae_aux_iwae_draw", m._desc, m._flat, m._packed_weights(), x.to(DEV), mu0, lv0, eps.to(DEV), B, k, 0, 0, 0, 0, ws, wsf, z, logq, eps_out)
    for buf, what in ((z, "z_out"), (logq, "logq"), (eps_out, "eps_out")):
        check_guard(buf, rows, what)
    check_workspace(ws, wsf, "aux_iwae_draw")
    assert torch.equal(eps_out[:rows].cpu(), eps.view(rows, w)), "eps_out is not the injected eps"
    return z[:rows].clone(), logq[:rows, 0].clone()


def eps_null_draws_the_documented_philox_elements(m, x):
    """An auxiliary model's forward with eps NULL draws [eps0 | eps] at (seed, offset) - both draws, element for element - and gives the bits of
    the same call with that eps injected; the module draws from the library's host stream"""
    B, nd, zd, D = x.size(0), m.noise_dim, m.z_dim, m.input_dim
    z, losses, grads, eps_out = abi_forward_backward(m, x, None, 0.7, 1.0 / D, seed=11, offset=5)
    assert torch.equal(eps_out, aux_draws(B, nd, zd, 11, 5)), "eps_out is not the documented draw"
    z2, losses2, grads2, _ = abi_forward_backward(m, x, eps_out.clone(), 0.7, 1.0 / D)
    assert torch.equal(z, z2) and torch.equal(losses, losses2) and torch.equal(grads, grads2), "own draw against the same draw injected"
    net.manual_seed(5)
    _, _, z1, loss1, _, _ = m(x)
    _, _, z2, loss2, _, _ = m(x, eps=aux_draws(B, nd, zd, 5, rng.HOST_STREAM | 0))
    assert torch.equal(z1, z2) and torch.equal(loss1.detach(), loss2.detach()), "the module's own draw"
    xs, mean, zg = m.generate(6)
    assert xs.shape == mean.shape == (6, D) and zg.shape == (6, zd) and bool(torch.isfinite(xs).all()), "generate"


# ---- losses and gradients -----------------------------------------------------------------------------------------------------------------
def check_losses(got, want, what):
    loss, recon, kld = (float(v) for v in got)
    print(f"{what}: loss {loss:.7g} / {float(want['loss']):.7g}, recon {recon:.7g} / {float(want['recon']):.7g}, kld {kld:.7g} / {float(want['kld']):.7g}")
    assert relerr(loss, want["loss"]) <= TOL_LOSS, (what, "loss", loss)
    assert relerr(recon, want["recon"]) <= TOL_MEAN and relerr(kld, want["kld"]) <= TOL_MEAN, (what, "recon / kld", recon, kld)


def check_grads(m, views, full, what, summ=None, label="worst gradient tensor"):
    """full: {name: gradient}; summ: {name: [L2, sum, first 8]} for the tensors a fixture keeps as summaries"""
    worst = 0.0
    for (name, _), g in zip(m.named_parameters(), views):
        assert bool(torch.isfinite(g).all()), (what, name)
        e = rel(t64(g), full[name]) if name in full else summary_err(t64(g), summ[name])
        worst = max(worst, e)
        assert e <= TOL_GRAD, (what, name, e)
    print(f"{what}: {label} {worst:.3g}")


def check_grads64(m, views, want, what):
    """every gradient tensor in full against the float64 restatement"""
    check_grads(m, views, want, what, label="worst gradient tensor against float64")


def check_grads_fixture(m, views, fx, b, what):
    """against the fp32 reference: the tensors the fixture stores in full, the L2 norms of the summarised ones"""
    worst = 0.0
    for (name, _), g in zip(m.named_parameters(), views):
        if f"{b}/g/{name}" in fx:
            e = rel(g.cpu(), fx[f"{b}/g/{name}"])
        else:
            e = relerr(g.double().norm().item(), fx[f"{b}/gs/{name}"][0])
        worst = max(worst, e)
        assert e <= TOL_GRAD, (what, name, e)
    print(f"{what}: worst gradient tensor / norm against the fp32 reference {worst:.3g}")


def check_restated_grads(fam, m, views, want, what):
    (check_grads64 if fam.grads64 else check_grads)(m, views, want, what)


# ---- the shared bodies --------------------------------------------------------------------------------------------------------------------
def forward_backward_against_the_reference(fam, golden_dir, name, what):
    """Both betas of one fixture: the statistics, then z, the losses and every gradient through the C ABI (on guarded buffers; a second backward on
    top of the first doubles the gradients) and through the module's autograd, the decoder's mean and its sample on the injected draw"""
    fx = load(golden_dir, name)
    m = fam.from_fixture(fx)
    D = m.input_dim
    x, eps, dec = cuda(fx["x"]), cuda(fx["eps"]), cuda(fx["dec_noise"])
    B = x.size(0)
    s0, s1 = ("mu0", "lv0") if fam.aux else ("mu", "lv")
    mu, lv = m.encode_stats(fam.inp(x))
    assert mu.shape == lv.shape == (B, m.noise_dim if fam.aux else m.z_dim), (what, mu.shape)
    assert rel(mu.cpu(), fx[s0]) <= TOL_LATENT and rel(lv.cpu(), fx[s1]) <= TOL_LATENT, (what, s0, s1)
    # the entry point on guarded buffers gives the module's bits
    assert all(torch.equal(a, b) for a, b in zip(abi_encode_stats(m, x, mu.size(1), (s0, s1)), (mu, lv))), (what, "encode_stats")
    if not fam.aux:
        zz, mu2, lv2 = m.encode(fam.inp(x), eps=eps)
        assert torch.equal(mu2, mu) and torch.equal(lv2, lv) and rel(zz.cpu(), fx["b1/z"]) <= TOL_LATENT, (what, "encode")
    if fam.head_fused is not None:
        assert L.query("ardae_vae_head_fused_ok", m._desc) == fam.head_fused, (what, "the default head")
    if fam.grads64:
        p64, cfg = fam.restate(fx)
    for b, beta in BETAS.items():
        want = {k: fx[f"{b}/{k}"] for k in ("loss", "recon", "kld")}
        full = {k[len(b) + 3:]: v for k, v in fx.items() if k.startswith(f"{b}/g/")}
        summ = {k[len(b) + 4:]: v for k, v in fx.items() if k.startswith(f"{b}/gs/")}

        def check_all(views, route):
            if fam.fixture_grads == "norm":
                check_grads_fixture(m, views, fx, b, f"{what} {b} {route}")
            else:
                check_grads(m, views, full, f"{what} {b} {route}", summ)
            if fam.grads64:
                check_grads64(m, views, g64, f"{what} {b} {route}")

        if fam.grads64:
            _, g64 = fam.loss_and_grads(p64, cfg, fam.to64(x), fam.to64(eps), beta, scale=1.0 / D)
        # the C ABI
        zc, losses, grads, _ = abi_forward_backward(m, x, eps, beta, 1.0 / D)
        assert rel(zc.cpu(), fx[f"{b}/z"]) <= TOL_LATENT, (what, b, "z")
        check_losses(losses.tolist(), want, f"{what} {b} abi")
        check_all(m.param_views(grads), "abi")
        # grads = grads_beta * grads + ...: a second call on top of the first doubles them
        _, _, acc, _ = abi_forward_backward(m, x, eps, beta, 1.0 / D, grads_beta=1.0, grads=grads)
        assert rel(acc.cpu(), 2 * grads.cpu()) <= 1e-6, (what, b, "accumulated gradients")
        # the module's autograd
        for p in m.parameters():
            p.grad = None
        xs, mean, zm, loss, recon, kld = m(x, beta=beta, eps=eps, dec_noise=dec)
        (loss / float(D)).backward()
        assert torch.equal(zm, zc) and not recon.requires_grad and not kld.requires_grad, (what, b, "module z")
        check_losses((loss.detach(), recon, kld), want, f"{what} {b} module")
        check_all([p.grad for p in m.parameters()], "module")
        assert xs.shape == mean.shape == (B, D), (what, b, xs.shape)
        assert rel(mean.cpu(), fx[f"{b}/mean"]) <= TOL_LATENT, (what, b, "mean")      # (resconv: the sample pass of forward() is the decode-only path)
        assert rel(xs.cpu(), fx[f"{b}/x_sample"]) <= 1e-4, (what, b, "x_sample")      # the decoder's relaxed-Bernoulli / Gaussian sample on the injected draw


def against_the_float64_restatement(fam, m, cfg, x, eps, cases):
    """z, losses and every gradient of the C ABI on guarded buffers against the live float64 restatement of the module's own parameters; x, eps on
    the host; cases: [(beta, label)] -> the last beta's restated forward, its z on the device"""
    p64, D = fam.p64_of(m), m.input_dim
    xd, ed = x.to(DEV), eps.to(DEV)
    for beta, what in cases:
        out, g64 = fam.loss_and_grads(p64, cfg, fam.to64(x), fam.to64(eps), beta, scale=1.0 / D)
        zc, losses, g, _ = abi_forward_backward(m, xd, ed, beta, 1.0 / D)
        assert rel(zc.cpu(), out["z"]) <= TOL_LATENT, (what, "z")
        check_losses(losses.tolist(), out, what)
        check_restated_grads(fam, m, m.param_views(g), g64, what)
    return out, zc


def engine_trajectory_against_the_reference(fam, golden_dir, name, what, steps):
    fx = load(golden_dir, name)
    m = fam.from_fixture(fx)
    B, D = int(fx["0/x"].shape[0]), m.input_dim
    cfg = traj_config(fx)
    eng = net.VaeEngine(m, cfg, batch_size=B)
    assert eng.loss_scale == 1.0 / D and eng.eps.shape == (B, m._eps_width), (what, eng.loss_scale, eng.eps.shape)
    restated = fam.trajectory(fx) if fam.traj == "restate" else None
    suffix = "_f64" if fam.traj == "restate" else ""
    for s in range(int(fx["cfg/steps"])):
        eng.step(fam.inp(cuda(fx[f"{s}/x"])), eps=cuda(fx[f"{s}/eps"]))
        st = eng.stats()
        assert st["beta"] == float(np.float32(cfg.beta_at(s))) == eng.beta_of_step(s + 1), (s, st["beta"])      # bit for bit, past the ramp's end too
        assert float(np.float32(float(fx[f"{s}/beta"]))) == st["beta"], (s, st["beta"])
        check_losses((st["loss"], st["recon"], st["kld"]), {k: fx[f"{s}/{k}{suffix}"] for k in ("loss", "recon", "kld")}, f"{what} step {s}")
        assert st["elbo"] == -(st["recon"] + st["kld"]), (s, st)
        if fam.traj == "p":
            worst = max(rel(p.detach().cpu(), fx[f"{s}/p/{k}"]) for k, p in m.named_parameters())
            print(f"{what} step {s}: worst parameter tensor {worst:.3g}")
        elif fam.traj == "ps":
            worst = max(summary_err(t64(p), fx[f"{s}/ps/{k}"]) for k, p in m.named_parameters())
            print(f"{what} step {s}: worst parameter summary {worst:.3g}")
        else:
            s64, _, p64 = next(restated)
            assert s64 == s, (s, s64)
            worst = max(rel(q.detach().cpu(), p64[k]) for k, q in m.named_parameters())
            print(f"{what} step {s}: worst parameter tensor against float64 {worst:.3g}")
        assert worst <= TOL_PARAM, (what, s, worst)
    assert eng.step_count == steps and eng.stats()["beta"] == 1.0, (what, eng.step_count)


def replay_equals_eager_and_resume(make, xs, cfg, resume_at):
    """Six steps on the inputs xs: the captured engine against the eager one and against a fresh engine that loads the checkpoint taken after
    `resume_at` steps and continues - parameters, optimiser buffers, per-step losses, the state block, the draw and the weight average, to the
    bit.  make() -> a new module with the same parameters.  -> the captured engine, its losses and its draws per step"""
    B, avg = xs[0].size(0), cfg.weight_avg

    def run(graph, steps, resume=None):
        net.manual_seed(99)
        eng = net.VaeEngine(make(), cfg, batch_size=B, graph=graph)
        if resume is not None:
            eng.load_state_dict(resume)
        losses, draws, saved = [], [], None
        for s in steps:
            eng.step(xs[s])
            losses.append(eng.losses.clone())
            draws.append(eng.eps.clone())
            if s == resume_at - 1:
                saved = eng.state_dict()
        return eng, losses, draws, saved

    a, la, da, sd = run(True, range(6))
    assert a._graph is not None, "no graph was captured"                 # captured at the third call, while beta was still moving
    b, lb, _, _ = run(False, range(6))
    assert b._graph is None, "graph=False captured a graph"
    c, lc, _, _ = run(True, range(resume_at, 6), resume=sd)                # a fresh engine continues
    for who, other, lo in (("eager", b, lb), ("resumed", c, lc)):
        assert torch.equal(a.model._flat, other.model._flat), (who, "parameters")
        for i, (t, u) in enumerate(zip(a.opt.buffers(), other.opt.buffers())):
            assert torch.equal(t, u), (who, "optimiser buffer", i)
        assert len(lo) == 6 - (resume_at if other is c else 0) and all(torch.equal(x, y) for x, y in zip(la[-len(lo):], lo)), (who, "per-step losses")
        assert torch.equal(a.state, other.state) and torch.equal(a.eps, other.eps) and torch.equal(a.losses, other.losses), (who, "state / eps / losses")
        if avg != "none":
            assert torch.equal(a.avg, other.avg) and a._n_avg() == other._n_avg() == 5, (who, "weight average")
    assert a.step_count == 6 and a.stats()["beta"] == float(np.float32(cfg.beta_at(5))) < 1.0, (a.step_count, a.stats()["beta"])
    assert not torch.equal(la[0], la[1]), "two steps gave the same losses"
    return a, la, da


def iwae_on_injected_draws(fam, golden_dir, name, what):
    """evaluate_iws, model.logprob and model.logprob_rows on a fixture's injected draws against its float64 values and the restatement
    -> fx, the module, x (for what only one family asserts)"""
    fx = load(golden_dir, name)
    m = fam.from_fixture(fx)
    x, eps, fwd_eps = cuda(fx["x"]), cuda(fx["lp/eps"]), cuda(fx["eps"])
    B, k = x.size(0), int(eps.size(1))
    eng = net.VaeEngine(m, net.VaeConfig(), batch_size=B)
    elbo, logprob = eng.evaluate_iws(x, k, eps=eps, fwd_eps=fwd_eps)
    print(f"{what}: logprob {logprob:.7f} / {float(fx['lp/value_f64']):.7f}, elbo {elbo:.6f}")
    assert relerr(logprob, fx["lp/value_f64"]) <= TOL_IWAE, (what, "logprob", logprob)
    assert relerr(float(m.logprob(x, sample_size=k, eps=eps)), fx["lp/value_f64"]) <= TOL_IWAE, (what, "model.logprob")
    # elbo = -(recon + kld (+ aux_kld)) of a forward on the same draw: the fixture's, and the model's own
    assert relerr(elbo, -(float(fx["b1/recon_f64"]) + float(fx["b1/kld_f64"]))) <= TOL_MEAN, (what, "elbo", elbo)
    _, _, _, _, recon, kld = m(x, beta=1.0, eps=fwd_eps)
    assert relerr(elbo, -(float(recon) + float(kld))) <= 1e-6, (what, "elbo against forward", elbo, float(recon), float(kld))
    rows = m.logprob_rows(x, k, eps=eps)
    if fam.logprob_is_evaluator:
        # model.logprob is the evaluator's bound on the same draws: at these B both run the encoder on B images and the decoder on B k rows in one
        # call, so the rows are equal to the bit (the means differ by fp32 against double accumulation)
        assert torch.equal(rows, net.GaussianIwaeEvaluator(m, k).evaluate_rows(x, eps, fwd_eps)[2]), (what, "rows against the evaluator's")
        assert relerr(float(m.logprob(x, sample_size=k, eps=eps)), logprob) <= 1e-6, (what, "model.logprob against the evaluator")
    # row by row against the restatement
    p64, cfg = fam.restate(fx)
    want = fam.logprob_rows(p64, cfg, fam.to64(fx["x"]), fam.to64(fx["lp/eps"]))
    assert rel(rows.cpu(), want) <= TOL_IWAE, (what, "rows")
    return fx, m, x


def iwae_does_not_depend_on_the_chunking(fam, m, x, k, plans, eps=None, fwd_eps=None):
    """The evaluator under several workspace budgets: plans = [(images whose chunk sets the budget or None for the default, the chunk lengths it
    must plan or their number)].  Own draws (seed 21) and injected draws (eps [N, k, w], fwd_eps [N, w]; drawn here if not given) give the same
    rows and the same (elbo, logprob) under every plan, to the bit; the ELBO rows are a forward's on the documented draw; the auxiliary models'
    importance samples are the documented Philox elements."""
    N, w = x.size(0), m._eps_width
    nd, zd = w - m.z_dim, m.z_dim
    probe = net.GaussianIwaeEvaluator(m, k)
    if eps is None:
        g = torch.Generator().manual_seed(77)
        eps, fwd_eps = torch.randn(N, k, w, generator=g).to(DEV), torch.randn(N, w, generator=g).to(DEV)
    results = []
    for c, lengths in plans:
        ev = probe if c is None else net.GaussianIwaeEvaluator(m, k, max_workspace_floats=probe.floats_per_chunk(c))
        if isinstance(lengths, int):
            assert len(ev.plan(N)) == lengths, (c, ev.plan(N))
        else:
            assert ev.plan(N) == [(b - n, b) for n, b in zip(lengths, np.cumsum(lengths).tolist())], (c, ev.plan(N))
        net.manual_seed(21)
        own = tuple(t.clone() for t in ev.evaluate_rows(x))                 # recon, kld, logprob rows
        net.manual_seed(21)
        res = ev.evaluate(x)
        results.append((own, res, tuple(t.clone() for t in ev.evaluate_rows(x, eps, fwd_eps)), ev.evaluate(x, eps, fwd_eps)))
    own0, res0, inj0, rinj0 = results[0]
    for (c, _), (own, res, inj, rinj) in zip(plans[1:], results[1:]):
        assert all(torch.equal(a, b) for a, b in zip(own, own0)) and res == res0, (c, "own draws")            # rows and (elbo, logprob), to the bit
        assert all(torch.equal(a, b) for a, b in zip(inj, inj0)) and rinj == rinj0, (c, "injected draws")
    assert all(bool(torch.isfinite(t).all()) for t in own0 + inj0), "not finite"
    assert not torch.equal(own0[2], inj0[2]), "own and injected draws gave the same rows"
    # the ELBO rows are a forward's: the same draw through the model gives their means
    e = [philox_normal((N, n), 21, rng.HOST_STREAM | i) for i, n in enumerate((nd, zd) if fam.aux else (zd,))]
    _, _, _, _, rec_mean, kld_mean = m(x, beta=1.0, eps=torch.cat(e, 1))
    assert relerr(own0[0].double().mean(), rec_mean) <= TOL_MEAN and relerr(own0[1].double().mean(), kld_mean) <= TOL_MEAN, "ELBO rows against forward"
    if fam.aux:      # the importance samples' draws are the documented elements of the next two offsets
        i0, i1 = philox_normal((N, k, nd), 21, rng.HOST_STREAM | 2), philox_normal((N, k, zd), 21, rng.HOST_STREAM | 3)
        net.manual_seed(33)
        assert torch.equal(probe.evaluate_rows(x, eps=torch.cat([i0, i1], 2), fwd_eps=torch.cat(e, 1))[2], own0[2]), "importance draws"
    net.manual_seed(22)
    assert not torch.equal(probe.evaluate_rows(x)[2], own0[2]), "another seed gave the same rows"
    with pytest.raises(ValueError, match="must be"):
        probe.evaluate_rows(x, eps=torch.zeros(N, k + 1, w, device=DEV))
    with pytest.raises(TypeError):
        probe.evaluate_rows(x.double())
    return results


def iwae_under_the_averaged_weights(m, make_other, B, lr):
    """evaluate_iws runs under the engine's averaged weights and puts the trained ones back; make_other() -> a second module of the same shape"""
    D, w = m.input_dim, m._eps_width
    eng = net.VaeEngine(m, net.VaeConfig(lr=lr, weight_avg="polyak", weight_avg_start=1, weight_avg_decay=0.5), batch_size=B)
    net.manual_seed(1)
    for _ in range(4):
        eng.step(torch.bernoulli(torch.full((B, D), 0.3)).to(DEV))
    trained = m._flat.clone()
    avg = eng.averaged_params().clone()
    assert not torch.equal(avg, trained) and bool(torch.isfinite(trained).all()) and bool(torch.isfinite(avg).all()), "the average"
    x = torch.bernoulli(torch.full((12, D), 0.3)).to(DEV)
    eps, fwd_eps = torch.randn(12, 16, w, device=DEV), torch.randn(12, w, device=DEV)
    got = eng.evaluate_iws(x, 16, eps=eps, fwd_eps=fwd_eps)
    assert torch.equal(m._flat, trained), "the trained weights were not put back"
    other = make_other()
    with torch.no_grad():
        other._flat.copy_(avg)
    other.mark_dirty()
    assert net.GaussianIwaeEvaluator(other, 16).evaluate(x, eps, fwd_eps) == got, "not the averaged weights' value"
    with torch.no_grad():
        other._flat.copy_(trained)
    other.mark_dirty()
    assert net.GaussianIwaeEvaluator(other, 16).evaluate(x, eps, fwd_eps) != got, "the trained weights give the same value"
    with eng.averaged_weights():
        assert torch.equal(m._flat, avg), "averaged_weights() did not install the average"
        with pytest.raises(RuntimeError, match="use_trained"):
            eng.step(x[:B])
    assert torch.equal(m._flat, trained), "averaged_weights() did not put the trained weights back"
    eng.step(x[:B].contiguous())           # ... and training goes on


def drop_in_route_equals_the_engine(fam, golden_dir, name):
    """vae.py's own loop (vae.py:396-417) on the module and net.Adam against the engine, three steps of a trajectory fixture"""
    fx = load(golden_dir, name)
    cfg = traj_config(fx)
    me, md = fam.from_fixture(fx), fam.from_fixture(fx)
    B, D = int(fx["0/x"].shape[0]), me.input_dim
    eng = net.VaeEngine(me, cfg, batch_size=B)
    md.return_samples = False
    optimizer = net.Adam(md.parameters(), lr=cfg.lr, betas=(cfg.beta1, 0.999))
    for i_ep in range(3):
        x, eps = cuda(fx[f"{i_ep}/x"]), cuda(fx[f"{i_ep}/eps"])
        eng.step(x, eps=eps)
        beta = net.annealing_func(cfg.beta_init, cfg.beta_fin, cfg.beta_annealing, i_ep)
        optimizer.zero_grad()
        output, _, latent, loss, recon_loss, kld_loss = md(x, beta=beta, eps=eps)
        scale = 1. / float(D)
        loss = scale * loss
        loss.backward()
        optimizer.step()
        st = eng.stats()
        assert relerr(loss.item() / scale, st["loss"]) <= TOL_LOSS and relerr(recon_loss.item(), st["recon"]) <= TOL_MEAN, (i_ep, "loss / recon")
        assert relerr(kld_loss.item(), st["kld"]) <= TOL_MEAN, (i_ep, "kld")
        for (pname, p), q in zip(md.named_parameters(), me.parameters()):
            assert rel(p.detach().cpu(), q.detach().cpu()) <= TOL_PARAM, (i_ep, pname)
            if fam.traj == "p":
                assert rel(p.detach().cpu(), fx[f"{i_ep}/p/{pname}"]) <= TOL_PARAM, (i_ep, pname, "fixture")
