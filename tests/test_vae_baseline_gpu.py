"""Gaussian-posterior VAE baselines on the device (ardae_model_desc.kind 8 / 9; vae.py --model mnist / toy): forward / backward against the
reference's fixtures through the C ABI and through autograd, the fused Gaussian head against the unfused launches, recipe widths against
the float64 restatement of tests/test_vae_baseline.py, the engine's trajectory, replay == eager, resume, IWAE evaluation, the drop-in route.

Tolerances are the project's for the same quantities (tests/test_engine_gpu.py, tests/test_iwae_eval_gpu.py): scalar losses 1e-4 relative,
recon / kld means 2e-5, gradients 2e-3 relative L2 per tensor, updated parameters 5e-3 relative L2, IWAE log-probability 1e-4 against the
float64 fixture, latents 1e-5 relative L2."""
import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import rng
from test_ardae_uncond import rel
from test_vae_baseline import BETAS, KIND_ID, case_names, load, logprob_rows, loss_and_grads, state_dict_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_LOSS, TOL_MEAN, TOL_GRAD, TOL_PARAM, TOL_IWAE, TOL_LATENT = 1e-4, 2e-5, 2e-3, 5e-3, 1e-4, 1e-5


def relerr(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def build(family, D, h, z, nl, act, sd=None):
    ctor = net.MNISTVAE if family == "mnist" else net.ToyVAE
    m = ctor(input_dim=D, h_dim=h, z_dim=z, nonlinearity=act, num_hidden_layers=nl)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV)


def from_fixture(fx):
    B, D, h, z, nl = (int(v) for v in fx["shape"])
    return build(str(fx["family"]), D, h, z, nl, str(fx["act"]), state_dict_of(fx)), (B, D, h, z, nl)


def cuda(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV).contiguous()


def abi_forward_backward(m, x, eps, beta, loss_scale):
    """-> z, losses [3], flat grads through ardae_vae_forward / ardae_vae_backward"""
    B = x.size(0)
    ws = torch.empty(L.query("ardae_model_workspace_floats", m._desc, B, 1, 1), device=DEV)
    z, eps_out, losses = torch.empty(B, m.z_dim, device=DEV), torch.empty(B, m.z_dim, device=DEV), torch.empty(3, device=DEV)
    L.call("ardae_vae_forward", m._desc, m._flat, m._packed_weights(), x, eps, B, beta, loss_scale, 0, 0, None, ws, ws.numel(), z, eps_out, losses)
    grads = torch.full_like(m._flat, float("nan"))          # (grads_beta 0: whatever was there is overwritten)
    L.call("ardae_vae_backward", m._desc, m._flat, m._packed_weights(), x, B, beta, loss_scale, ws, ws.numel(), grads, 0.0)
    assert torch.equal(eps_out, eps)
    return z, losses, grads


def check_losses(got, want, what):
    loss, recon, kld = (float(v) for v in got)
    print(f"{what}: loss {loss:.7g} / {float(want['loss']):.7g}, recon {recon:.7g} / {float(want['recon']):.7g}, kld {kld:.7g} / {float(want['kld']):.7g}")
    assert relerr(loss, want["loss"]) <= TOL_LOSS
    assert relerr(recon, want["recon"]) <= TOL_MEAN and relerr(kld, want["kld"]) <= TOL_MEAN


def check_grads(m, views, want, what):
    worst = 0.0
    for (name, _), g in zip(m.named_parameters(), views):
        e = rel(g.cpu(), want[name])
        worst = max(worst, e)
        assert e <= TOL_GRAD, (what, name, e)
    print(f"{what}: worst gradient tensor {worst:.3g}")


# ---- 5. forward / backward against the reference's fixtures ------------------------------------------------------------------------
@pytest.mark.parametrize("family,case", case_names())
def test_forward_backward_against_the_reference(golden_dir, family, case):
    fx = load(golden_dir, f"vae_{family}_{case}")
    m, (B, D, h, z, nl) = from_fixture(fx)
    x, eps, dec = cuda(fx["x"]), cuda(fx["eps"]), cuda(fx["dec_noise"])
    mu, lv = m.encode_stats(x)
    assert rel(mu.cpu(), fx["mu"]) <= TOL_LATENT and rel(lv.cpu(), fx["lv"]) <= TOL_LATENT
    zz, mu2, lv2 = m.encode(x, eps=eps)
    assert torch.equal(mu2, mu) and torch.equal(lv2, lv) and rel(zz.cpu(), fx["b1/z"]) <= TOL_LATENT
    for b, beta in BETAS.items():
        want = {k: fx[f"{b}/{k}"] for k in ("loss", "recon", "kld")}
        want_g = {k[len(b) + 3:]: v for k, v in fx.items() if k.startswith(f"{b}/g/")}
        # the C ABI
        zc, losses, grads = abi_forward_backward(m, x, eps, beta, 1.0 / D)
        assert rel(zc.cpu(), fx[f"{b}/z"]) <= TOL_LATENT
        check_losses(losses.tolist(), want, f"{family} {case} {b} abi")
        check_grads(m, m.param_views(grads), want_g, f"{family} {case} {b} abi")
        # grads = grads_beta * grads + ...: a second call on top of the first doubles them
        ws = torch.empty(L.query("ardae_model_workspace_floats", m._desc, B, 1, 1), device=DEV)
        z2, l2 = torch.empty_like(zc), torch.empty(3, device=DEV)
        L.call("ardae_vae_forward", m._desc, m._flat, m._packed_weights(), x, eps, B, beta, 1.0 / D, 0, 0, None, ws, ws.numel(), z2, None, l2)
        acc = grads.clone()
        L.call("ardae_vae_backward", m._desc, m._flat, m._packed_weights(), x, B, beta, 1.0 / D, ws, ws.numel(), acc, 1.0)
        assert rel(acc.cpu(), 2 * grads.cpu()) <= 1e-6
        # the module's autograd
        for p in m.parameters():
            p.grad = None
        xs, mean, zm, loss, recon, kld = m(x, beta=beta, eps=eps, dec_noise=dec)
        (loss / float(D)).backward()
        assert torch.equal(zm, zc) and not recon.requires_grad and not kld.requires_grad
        check_losses((loss.detach(), recon, kld), want, f"{family} {case} {b} module")
        check_grads(m, [p.grad for p in m.parameters()], want_g, f"{family} {case} {b} module")
        assert rel(mean.cpu(), fx[f"{b}/mean"]) <= TOL_LATENT
        assert rel(xs.cpu(), fx[f"{b}/x_sample"]) <= 1e-4        # the decoder's relaxed-Bernoulli / Gaussian sample on the injected draw


def test_generate_and_the_in_kernel_draw_of_the_module():
    m = build("mnist", 20, 24, 4, 2, "softplus")
    net.manual_seed(5)
    xs, mean, z = m.generate(7)
    assert xs.shape == mean.shape == (7, 20) and z.shape == (7, 4) and bool(torch.isfinite(xs).all())
    x = torch.bernoulli(torch.full((9, 20), 0.3)).to(DEV)
    net.manual_seed(5)
    offset = rng.HOST_STREAM | 0
    _, _, z1, loss1, _, _ = m(x)
    want = torch.empty(9, 4, device=DEV)
    L.call("ardae_philox_normal_at", want, want.numel(), 5, offset, None, 0)
    _, _, z2, loss2, _, _ = m(x, eps=want)
    assert torch.equal(z1, z2) and torch.equal(loss1.detach(), loss2.detach())      # the head drew exactly that draw


# ---- 6. the fused head against the unfused launches --------------------------------------------------------------------------------
def head(m, hid, variant, seed=123, offset=5, eps=None):
    B, z = hid.size(0), m.z_dim
    out = {k: torch.full((B, z), float("nan"), device=DEV) for k in ("mu", "lv", "z", "eps")}
    out["kld"] = torch.full((B,), float("nan"), device=DEV)
    L.call("ardae_vae_head", m._desc, m._flat, m._packed_weights(), hid, eps, B, seed, offset, None, variant, out["mu"], out["lv"], out["z"], out["eps"],
           out["kld"])
    return out


@pytest.mark.parametrize("B,h,z", [(6, 40, 6), (70, 300, 32), (129, 256, 2)])
def test_fused_head_equals_the_unfused_launches(B, h, z):
    torch.manual_seed(B)
    family = "toy" if z == 2 else "mnist"
    m = build(family, 2 if z == 2 else 36, h, z, 2, "softplus")
    # the default is the fused kernel where both matrices' rows start on 16 bytes (the recipe's 300 -> 2 x 32), the unfused launches elsewhere
    assert L.query("ardae_vae_head_fused_ok", m._desc) == (1 if (h, z) == (300, 32) else 0)
    hid = torch.nn.functional.softplus(torch.randn(B, h)).to(DEV).contiguous()
    fused, unfused = head(m, hid, 1), head(m, hid, 2)
    draw = torch.empty(B, z, device=DEV)
    L.call("ardae_philox_normal_at", draw, draw.numel(), 123, 5, None, 0)
    assert torch.equal(fused["eps"], draw) and torch.equal(unfused["eps"], draw)
    for k in ("mu", "lv", "z", "kld"):
        e = rel(fused[k].cpu(), unfused[k].cpu())
        same = float((fused[k] == unfused[k]).float().mean())
        print(f"head B={B} h={h} z={z} {k}: rel L2 {e:.3g}, bit-identical {100 * same:.1f} %")
        assert bool(torch.isfinite(fused[k]).all()) and e <= 1e-6
    # against float64 on the host
    p = {k: v.detach().double().cpu() for k, v in m.named_parameters()}
    hd = hid.double().cpu()
    mu = hd @ p["encode.reparam.mean_fn.weight"].t() + p["encode.reparam.mean_fn.bias"]
    lv = hd @ p["encode.reparam.logvar_fn.weight"].t() + p["encode.reparam.logvar_fn.bias"]
    assert rel(fused["mu"].cpu(), mu) <= TOL_LATENT and rel(fused["lv"].cpu(), lv) <= TOL_LATENT
    assert rel(fused["z"].cpu(), mu + torch.exp(0.5 * lv) * draw.double().cpu()) <= TOL_LATENT
    assert rel(fused["kld"].cpu(), -0.5 * (1 + lv - mu ** 2 - lv.exp()).sum(1)) <= TOL_MEAN
    # the variant the library picks, and an injected eps goes through unchanged
    auto, picked = head(m, hid, 0, eps=draw), (fused if L.query("ardae_vae_head_fused_ok", m._desc) else unfused)
    assert all(torch.equal(auto[k], picked[k]) for k in ("mu", "lv", "z", "eps", "kld"))
    if B == 70:      # a row's bits do not depend on B
        small = head(m, hid[:6].contiguous(), 1)
        for k in ("mu", "lv", "z", "eps", "kld"):
            assert torch.equal(small[k], fused[k][:6]), k


# ---- 7. recipe width against the live float64 restatement --------------------------------------------------------------------------
@pytest.mark.parametrize("family,D,h,z,act,B", [("mnist", 784, 300, 32, "softplus", 70), ("toy", 2, 256, 2, "relu", 129)])
def test_recipe_width_against_the_float64_restatement(family, D, h, z, act, B):
    torch.manual_seed(17)
    m = build(family, D, h, z, 2, act)
    x = (torch.bernoulli(torch.full((B, D), 0.3)) if family == "mnist" else torch.randn(B, D))
    eps = torch.randn(B, z)
    p64 = {k: v.detach().double().cpu() for k, v in m.named_parameters()}
    for beta in (1.0, 0.3):
        out, grads = loss_and_grads(family, p64, act, x.double(), eps.double(), beta, 1.0 / D)
        zc, losses, g = abi_forward_backward(m, x.to(DEV), eps.to(DEV), beta, 1.0 / D)
        assert rel(zc.cpu(), out["z"]) <= TOL_LATENT
        check_losses(losses.tolist(), out, f"{family} recipe width beta {beta}")
        check_grads(m, m.param_views(g), grads, f"{family} recipe width beta {beta}")


# ---- 8. the engine's trajectory ----------------------------------------------------------------------------------------------------
def traj_config(fx, **kw):
    return net.VaeConfig(lr=float(fx["cfg/lr"]), beta1=float(fx["cfg/beta1"]), beta_init=float(fx["cfg/beta_init"]), beta_fin=float(fx["cfg/beta_fin"]),
                         beta_annealing=int(fx["cfg/beta_annealing"]), **kw)


@pytest.mark.parametrize("family", ["mnist", "toy"])
def test_engine_trajectory_against_the_reference(golden_dir, family):
    fx = load(golden_dir, f"vae_traj_{family}")
    m, (B, D, h, z, nl) = from_fixture(fx)
    cfg = traj_config(fx)
    eng = net.VaeEngine(m, cfg, batch_size=B)
    assert eng.loss_scale == 1.0 / D
    for s in range(int(fx["cfg/steps"])):
        eng.step(cuda(fx[f"{s}/x"]), eps=cuda(fx[f"{s}/eps"]))
        st = eng.stats()
        assert st["beta"] == float(np.float32(cfg.beta_at(s))) == eng.beta_of_step(s + 1), (s, st["beta"])      # bit for bit, past the ramp's end too
        assert float(np.float32(float(fx[f"{s}/beta"]))) == st["beta"]
        check_losses((st["loss"], st["recon"], st["kld"]), {k: fx[f"{s}/{k}"] for k in ("loss", "recon", "kld")}, f"{family} step {s}")
        assert st["elbo"] == -(st["recon"] + st["kld"])
        worst = max(rel(p.detach().cpu(), fx[f"{s}/p/{name}"]) for name, p in m.named_parameters())
        print(f"{family} step {s}: worst parameter tensor {worst:.3g}")
        assert worst <= TOL_PARAM
    assert eng.step_count == 5 and eng.stats()["beta"] == 1.0


# ---- 9. replay == eager, resume -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,optimizer,avg", [("mnist", "adam", "swa"), ("toy", "rmsprop", "none"), ("mnist", "amsgrad", "polyak")])
def test_replay_equals_eager_and_resume_continues_to_the_same_bits(family, optimizer, avg):
    D, h, z, B = (36, 48, 8, 10) if family == "mnist" else (2, 40, 2, 12)
    torch.manual_seed(3)
    sd0 = {k: v.clone() for k, v in build(family, D, h, z, 2, "softplus").state_dict().items()}
    g = torch.Generator().manual_seed(4)
    xs = [(torch.bernoulli(torch.full((B, D), 0.3), generator=g) if family == "mnist" else torch.randn(B, D, generator=g)).to(DEV) for _ in range(6)]
    cfg = net.VaeConfig(optimizer=optimizer, lr=1e-3, beta_init=1e-4, beta_fin=1.0, beta_annealing=10, weight_avg=avg, weight_avg_start=1)

    def run(graph, steps, resume=None):
        net.manual_seed(99)
        m = build(family, D, h, z, 2, "softplus", sd0)
        eng = net.VaeEngine(m, cfg, batch_size=B, graph=graph)
        if resume is not None:
            eng.load_state_dict(resume)
        losses, saved = [], None
        for s in steps:
            eng.step(xs[s])
            losses.append(eng.losses.clone())
            if s == 2:
                saved = eng.state_dict()
        return eng, losses, saved

    a, la, sd3 = run(True, range(6))
    assert a._graph is not None                                     # captured at the third call, while beta was still moving
    b, lb, _ = run(False, range(6))
    assert b._graph is None
    c, lc, _ = run(True, range(3, 6), resume=sd3)
    for other, lo in ((b, lb), (c, lc)):
        assert torch.equal(a.model._flat, other.model._flat)
        for t, u in zip(a.opt.buffers(), other.opt.buffers()):
            assert torch.equal(t, u)
        assert all(torch.equal(x, y) for x, y in zip(la[-len(lo):], lo))
        assert torch.equal(a.state, other.state) and torch.equal(a.eps, other.eps)
        if avg != "none":
            assert torch.equal(a.avg, other.avg) and a._n_avg() == other._n_avg() == 5
    assert a.stats()["beta"] == float(np.float32(cfg.beta_at(5))) < 1.0
    # the step's own draw is the separate draw at Philox offset RNG_STRIDE * step (+ 0), read through the state block
    want = torch.empty(B, z, device=DEV)
    L.call("ardae_philox_normal_at", want, want.numel(), 99, a.RNG_STRIDE * a.step_count, None, 0)
    assert a.RNG_STRIDE == 16 and a.step_count == 6 and torch.equal(a.eps, want)
    assert not torch.equal(la[0], la[1])


# ---- 10. IWAE evaluation under the analytic posterior -------------------------------------------------------------------------------
@pytest.mark.parametrize("family,case", case_names())
def test_iwae_on_injected_draws_against_the_float64_fixture(golden_dir, family, case):
    fx = load(golden_dir, f"vae_{family}_{case}")
    m, (B, D, h, z, nl) = from_fixture(fx)
    x, eps = cuda(fx["x"]), cuda(fx["lp/eps"])
    eng = net.VaeEngine(m, net.VaeConfig(), batch_size=B)
    fwd_eps = cuda(fx["eps"])
    elbo, logprob = eng.evaluate_iws(x, int(eps.size(1)), eps=eps, fwd_eps=fwd_eps)
    print(f"{family} {case}: logprob {logprob:.7f} / {float(fx['lp/value_f64']):.7f}, elbo {elbo:.6f}")
    assert relerr(logprob, fx["lp/value_f64"]) <= TOL_IWAE
    assert relerr(float(m.logprob(x, sample_size=int(eps.size(1)), eps=eps)), fx["lp/value_f64"]) <= TOL_IWAE
    # elbo = -(recon + kld) of a forward on the same draw
    assert relerr(elbo, -(float(fx["b1/recon_f64"]) + float(fx["b1/kld_f64"]))) <= TOL_MEAN
    _, _, _, _, recon, kld = m(x, beta=1.0, eps=fwd_eps)
    assert relerr(elbo, -(float(recon) + float(kld))) <= 1e-6
    # the KL rows the evaluator reduces are the head's
    mu, lv = m.encode_stats(x)
    rows_kld = torch.empty(B, device=DEV)
    L.call("ardae_vae_kld_rows", mu, lv, B, z, rows_kld)
    assert rel(rows_kld.cpu(), -0.5 * (1 + fx["lv_f64"] - fx["mu_f64"] ** 2 - np.exp(fx["lv_f64"])).sum(1)) <= TOL_MEAN
    # row by row against the restatement
    rows = m.logprob_rows(x, int(eps.size(1)), eps=eps)
    want = logprob_rows(family, state_dict_of(fx, torch.float64), str(fx["act"]), x.double().cpu(), eps.double().cpu())
    assert rel(rows.cpu(), want) <= TOL_IWAE


def test_iwae_own_draws_do_not_depend_on_the_chunking():
    torch.manual_seed(8)
    m = build("mnist", 36, 48, 8, 2, "softplus")
    x = torch.bernoulli(torch.full((12, 36), 0.3)).to(DEV)
    k = 16
    probe = net.GaussianIwaeEvaluator(m, k)
    results = []
    for c, nchunks in ((12, 1), (8, 2), (4, 3)):
        ev = net.GaussianIwaeEvaluator(m, k, max_workspace_floats=probe.floats_per_chunk(c))
        assert len(ev.plan(12)) == nchunks
        net.manual_seed(21)
        recon, kld, rows = ev.evaluate_rows(x)
        net.manual_seed(21)
        results.append(((recon.clone(), kld.clone(), rows.clone()), ev.evaluate(x)))
    for parts, result in results[1:]:
        assert all(torch.equal(a, b) for a, b in zip(parts, results[0][0]))
        assert result == results[0][1]                          # (elbo, logprob), to the bit
    # the ELBO rows are a forward's: the same draw through the model gives their means
    net.manual_seed(21)
    fwd_eps = torch.empty(12, 8, device=DEV)
    L.call("ardae_philox_normal_at", fwd_eps, fwd_eps.numel(), 21, rng.HOST_STREAM | 0, None, 0)
    _, _, _, _, rec_mean, kld_mean = m(x, beta=1.0, eps=fwd_eps)
    assert relerr(results[0][0][0].double().mean(), rec_mean) <= TOL_MEAN and relerr(results[0][0][1].double().mean(), kld_mean) <= TOL_MEAN
    net.manual_seed(22)
    assert not torch.equal(probe.evaluate_rows(x)[2], results[0][0][2])
    with pytest.raises(ValueError, match="must be"):
        probe.evaluate_rows(x, eps=torch.zeros(12, k + 1, 8, device=DEV))
    with pytest.raises(TypeError):
        probe.evaluate_rows(x.double())


def test_iwae_runs_under_the_averaged_weights_and_puts_the_trained_ones_back():
    torch.manual_seed(9)
    B, D = 8, 36
    m = build("mnist", D, 48, 8, 2, "softplus")
    eng = net.VaeEngine(m, net.VaeConfig(lr=1e-2, weight_avg="polyak", weight_avg_start=1, weight_avg_decay=0.5), batch_size=B)
    net.manual_seed(1)
    for _ in range(4):
        eng.step(torch.bernoulli(torch.full((B, D), 0.3)).to(DEV))
    trained = m._flat.clone()
    avg = eng.averaged_params().clone()
    assert not torch.equal(avg, trained)
    x = torch.bernoulli(torch.full((12, D), 0.3)).to(DEV)
    eps, fwd_eps = torch.randn(12, 16, 8, device=DEV), torch.randn(12, 8, device=DEV)
    got = eng.evaluate_iws(x, 16, eps=eps, fwd_eps=fwd_eps)
    assert torch.equal(m._flat, trained)
    other = build("mnist", D, 48, 8, 2, "softplus")
    with torch.no_grad():
        other._flat.copy_(avg)
    assert net.GaussianIwaeEvaluator(other, 16).evaluate(x, eps, fwd_eps) == got
    with torch.no_grad():
        other._flat.copy_(trained)
    other.mark_dirty()
    assert net.GaussianIwaeEvaluator(other, 16).evaluate(x, eps, fwd_eps) != got
    with eng.averaged_weights():
        assert torch.equal(m._flat, avg)
        with pytest.raises(RuntimeError, match="use_trained"):
            eng.step(x[:B])
    assert torch.equal(m._flat, trained)
    eng.step(x[:B].contiguous())           # ... and training goes on


# ---- 11. the drop-in route ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["mnist", "toy"])
def test_drop_in_route_equals_the_engine(golden_dir, family):
    fx = load(golden_dir, f"vae_traj_{family}")
    cfg = traj_config(fx)
    me, (B, D, h, z, nl) = from_fixture(fx)
    eng = net.VaeEngine(me, cfg, batch_size=B)
    md, _ = from_fixture(fx)
    md.return_samples = False
    optimizer = net.Adam(md.parameters(), lr=cfg.lr, betas=(cfg.beta1, 0.999))
    for i_ep in range(3):
        x, eps = cuda(fx[f"{i_ep}/x"]), cuda(fx[f"{i_ep}/eps"])
        eng.step(x, eps=eps)
        # vae.py:396-417
        beta = net.annealing_func(cfg.beta_init, cfg.beta_fin, cfg.beta_annealing, i_ep)
        optimizer.zero_grad()
        output, _, latent, loss, recon_loss, kld_loss = md(x, beta=beta, eps=eps)
        scale = 1. / float(D)
        loss = scale * loss
        loss.backward()
        optimizer.step()
        st = eng.stats()
        assert relerr(loss.item() / scale, st["loss"]) <= TOL_LOSS and relerr(recon_loss.item(), st["recon"]) <= TOL_MEAN
        assert relerr(kld_loss.item(), st["kld"]) <= TOL_MEAN
        for (name, p), q in zip(md.named_parameters(), me.parameters()):
            assert rel(p.detach().cpu(), q.detach().cpu()) <= TOL_PARAM, (i_ep, name)
            assert rel(p.detach().cpu(), fx[f"{i_ep}/p/{name}"]) <= TOL_PARAM, (i_ep, name)
