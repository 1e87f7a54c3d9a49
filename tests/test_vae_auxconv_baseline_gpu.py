"""The hierarchical conv Gaussian baseline on the device (ardae_model_desc.kind 17; vae.py --model auxconv): forward / backward against the reference's
fixtures through the C ABI and through autograd on NaN-filled buffers with guard rows, the in-kernel draws, the recipe's widths against the float64
restatement of tests/test_vae_auxconv_baseline.py, the engine's trajectory, replay == eager, resume, the three-stage IWAE evaluation on fixed groups,
the drop-in route, and the decoder's last two stages as one kernel (ardae_conv_tail) against that restatement and the unfused launches.

Tolerances are those of tests/test_vae_conv_baseline_gpu.py and tests/test_vae_aux_baseline_gpu.py, unchanged: scalar losses 1e-4 relative, recon / kld
means 2e-5, gradients 2e-3 relative L2 per tensor, updated parameters 5e-3 relative L2, IWAE log-probability 1e-4 against the float64 fixture, latents
1e-5 relative L2."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import rng
from test_ardae_uncond import rel
from test_vae_baseline import BETAS, load
from test_vae_baseline_gpu import TOL_IWAE, TOL_LATENT, TOL_LOSS, TOL_MEAN, TOL_PARAM, check_losses, cuda, relerr
from test_vae_conv_baseline import decode_logit, relaxed_sample
from test_vae_conv_baseline_gpu import check_grads64, check_grads_fixture, check_guard, guarded, p64_of
from test_vae_auxconv_baseline import (CASES, D, auxconv_params, logprob_rows, logq_rows, loss_and_grads, shape_of, summary_err, tail_logit)

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
KNOB_ENV = {"ARDAE_DEBUG_KNOBS": "1", "ARDAE_CONV_TAIL_UNFUSED": "1"}
KNOB_ON = all(os.environ.get(k) == v for k, v in KNOB_ENV.items())      # (the child process of the last test)
ALL_ACTS = ("relu", "softplus", "elu", "tanh", "leaky_relu", "swish")


def build(nd, z, act, sd=None, **kw):
    m = net.MNISTConvAuxVAE(z0_dim=nd, z_dim=z, nonlinearity=act, **kw)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV)


def from_fixture(fx):
    (B, nd, z), act = shape_of(fx)
    return build(nd, z, act, auxconv_params(fx)), B, nd, z, act


def seeded(nd, z, act, seed):
    """A model with torch's default initialisation (non-zero biases everywhere) from a seed"""
    torch.manual_seed(seed)
    return build(nd, z, act, do_xavier=False)


def abi_forward_backward(m, x, eps, beta, grads_beta=0.0, grads=None, seed=0, offset=0):
    """-> z, losses [3], flat grads, eps_out through ardae_vae_forward / ardae_vae_backward on NaN-filled buffers: the workspace, every output, and
    guard rows behind each of them (and behind the workspace's declared end)"""
    B = x.size(0)
    wsf = L.query("ardae_model_workspace_floats", m._desc, B, 1, 1)
    ws = torch.full((wsf + 4096,), NAN, device=DEV)
    zo, eo, losses = guarded(B, m.z_dim), guarded(B, m._eps_width), guarded(3, 1)
    L.call("ardae_vae_forward", m._desc, m._flat, m._packed_weights(), x, eps, B, beta, 1.0 / D, seed, offset, None, ws, wsf, zo, eo, losses)
    n = m._flat.numel()
    g = torch.full((n + 64,), NAN, device=DEV)
    if grads is not None:
        g[:n] = grads
    L.call("ardae_vae_backward", m._desc, m._flat, m._packed_weights(), x, B, beta, 1.0 / D, ws, wsf, g, grads_beta)
    for buf, rows, what in ((zo, B, "z_out"), (eo, B, "eps_out"), (losses, 3, "losses")):
        check_guard(buf, rows, what)
    assert bool(torch.isnan(ws[wsf:]).all()) and bool(torch.isnan(g[n:]).all()) and bool(torch.isfinite(g[:n]).all())
    if eps is not None:
        assert torch.equal(eo[:B], eps)
    return zo[:B].clone(), losses[:3, 0].clone(), g[:n].clone(), eo[:B].clone()


# ---- 1. both fixtures, both betas --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_forward_backward_against_the_reference(golden_dir, case):
    fx = load(golden_dir, "vae_" + case)
    m, B, nd, z, act = from_fixture(fx)
    p64 = auxconv_params(fx, torch.float64)
    x, eps, dec = cuda(fx["x"]), cuda(fx["eps"]), cuda(fx["dec_noise"])
    wsf = L.query("ardae_model_workspace_floats", m._desc, B, 1, 0)
    ws, mu0, lv0 = torch.full((wsf + 4096,), NAN, device=DEV), guarded(B, nd), guarded(B, nd)
    L.call("ardae_vae_encode_stats", m._desc, m._flat, m._packed_weights(), x, B, ws, wsf, mu0, lv0)
    check_guard(mu0, B, "mu0"), check_guard(lv0, B, "lv0")
    assert bool(torch.isnan(ws[wsf:]).all())
    assert rel(mu0[:B].cpu(), fx["mu0"]) <= TOL_LATENT and rel(lv0[:B].cpu(), fx["lv0"]) <= TOL_LATENT
    assert all(torch.equal(a, b[:B]) for a, b in zip(m.encode_stats(x.view(B, 1, 28, 28)), (mu0, lv0)))
    assert L.query("ardae_vae_head_fused_ok", m._desc) == 1       # the z head's fused form (kind 11's tail form) is the default at z <= 64
    for b, beta in BETAS.items():
        want = {k: fx[f"{b}/{k}"] for k in ("loss", "recon", "kld")}
        _, g64 = loss_and_grads(p64, act, x.double().cpu(), eps.double().cpu(), beta, 1.0 / D)
        # the C ABI
        zc, losses, grads, _ = abi_forward_backward(m, x, eps, beta)
        assert rel(zc.cpu(), fx[f"{b}/z"]) <= TOL_LATENT
        check_losses(losses.tolist(), want, f"auxconv {case} {b} abi")
        check_grads_fixture(m, m.param_views(grads), fx, b, f"auxconv {case} {b} abi")
        check_grads64(m, m.param_views(grads), g64, f"auxconv {case} {b} abi")
        # grads = grads_beta * grads + ...: a second call on top of the first doubles them
        _, _, acc, _ = abi_forward_backward(m, x, eps, beta, grads_beta=1.0, grads=grads)
        assert rel(acc.cpu(), 2 * grads.cpu()) <= 1e-6
        # the module's autograd
        for p in m.parameters():
            p.grad = None
        xs, mean, zm, loss, recon, kld = m(x, beta=beta, eps=eps, dec_noise=dec)
        (loss / float(D)).backward()
        assert torch.equal(zm, zc) and not recon.requires_grad and not kld.requires_grad
        check_losses((loss.detach(), recon, kld), want, f"auxconv {case} {b} module")
        check_grads_fixture(m, [p.grad for p in m.parameters()], fx, b, f"auxconv {case} {b} module")
        check_grads64(m, [p.grad for p in m.parameters()], g64, f"auxconv {case} {b} module")
        assert xs.shape == mean.shape == (B, D)
        assert rel(mean.cpu(), fx[f"{b}/mean"]) <= TOL_LATENT
        assert rel(xs.cpu(), fx[f"{b}/x_sample"]) <= 1e-4        # the decoder's relaxed-Bernoulli sample on the injected draw


# ---- 2. the in-kernel draws ----------------------------------------------------------------------------------------------------------
def test_eps_null_draws_the_documented_philox_elements():
    B, nd, zd = 7, 5, 3                                    # B nd = 35: the second draw starts at element 36
    m = seeded(nd, zd, "softplus", 1)
    x = torch.bernoulli(torch.full((B, D), 0.3)).to(DEV)
    z, losses, grads, eps_out = abi_forward_backward(m, x, None, 0.7, seed=11, offset=5)
    want0, want1 = torch.empty(B, nd, device=DEV), torch.empty(B, zd, device=DEV)
    L.call("ardae_philox_normal_at", want0, want0.numel(), 11, 5, None, 0)
    L.call("ardae_philox_normal_at", want1, want1.numel(), 11, 5, None, (B * nd + 3) // 4 * 4)
    assert torch.equal(eps_out, torch.cat([want0, want1], 1))                  # both draws, element for element
    z2, losses2, grads2, _ = abi_forward_backward(m, x, eps_out.clone(), 0.7)
    assert torch.equal(z, z2) and torch.equal(losses, losses2) and torch.equal(grads, grads2)
    # the module draws from the library's host stream
    net.manual_seed(5)
    offset = rng.HOST_STREAM | 0
    _, _, z1, loss1, _, _ = m(x)
    L.call("ardae_philox_normal_at", want0, want0.numel(), 5, offset, None, 0)
    L.call("ardae_philox_normal_at", want1, want1.numel(), 5, offset, None, (B * nd + 3) // 4 * 4)
    _, _, z2, loss2, _, _ = m(x, eps=torch.cat([want0, want1], 1))
    assert torch.equal(z1, z2) and torch.equal(loss1.detach(), loss2.detach())
    xs, mean, zg = m.generate(6)
    assert xs.shape == mean.shape == (6, D) and zg.shape == (6, zd) and bool(torch.isfinite(xs).all())


# ---- 3. the recipe's widths against the live float64 restatement ---------------------------------------------------------------------
def test_recipe_width_against_the_float64_restatement():
    B, nd, z, act = 70, 100, 32, "softplus"
    m = seeded(nd, z, act, 17)
    x, eps = torch.bernoulli(torch.full((B, D), 0.3)), torch.randn(B, nd + z)
    p64 = p64_of(m)
    for beta in (1.0, 0.3):
        out, g64 = loss_and_grads(p64, act, x.double(), eps.double(), beta, 1.0 / D)
        zc, losses, g, _ = abi_forward_backward(m, x.to(DEV), eps.to(DEV), beta)
        assert rel(zc.cpu(), out["z"]) <= TOL_LATENT
        check_losses(losses.tolist(), out, f"auxconv recipe width beta {beta}")
        check_grads64(m, m.param_views(g), g64, f"auxconv recipe width beta {beta}")


# ---- 4. the engine's trajectory, replay == eager, resume ----------------------------------------------------------------------------
def traj_config(fx, **kw):
    return net.VaeConfig(lr=float(fx["cfg/lr"]), beta1=float(fx["cfg/beta1"]), beta_init=float(fx["cfg/beta_init"]), beta_fin=float(fx["cfg/beta_fin"]),
                         beta_annealing=int(fx["cfg/beta_annealing"]), **kw)


def test_engine_trajectory_against_the_reference(golden_dir):
    fx = load(golden_dir, "vae_traj_auxconv")
    m, B, nd, z, act = from_fixture(fx)
    cfg = traj_config(fx)
    eng = net.VaeEngine(m, cfg, batch_size=B)
    assert eng.loss_scale == 1.0 / D and eng.eps.shape == (B, nd + z)
    for s in range(int(fx["cfg/steps"])):
        eng.step(cuda(fx[f"{s}/x"]), eps=cuda(fx[f"{s}/eps"]))
        st = eng.stats()
        assert st["beta"] == float(np.float32(cfg.beta_at(s))) == eng.beta_of_step(s + 1), (s, st["beta"])
        check_losses((st["loss"], st["recon"], st["kld"]), {k: fx[f"{s}/{k}"] for k in ("loss", "recon", "kld")}, f"auxconv step {s}")
        worst = max(summary_err(p.detach().double().cpu(), fx[f"{s}/ps/{k}"]) for k, p in m.named_parameters())
        print(f"auxconv step {s}: worst parameter summary {worst:.3g}")
        assert worst <= TOL_PARAM
    assert eng.step_count == 4 and eng.stats()["beta"] == 1.0


def test_replay_equals_eager_and_resume_continues_to_the_same_bits():
    """One optimiser with a weight average: the captured step replays through the beta ramp, the checkpoint carries the average"""
    nd, z, B = 10, 6, 10
    torch.manual_seed(3)
    sd0 = {k: v.clone() for k, v in build(nd, z, "elu").state_dict().items()}
    g = torch.Generator().manual_seed(4)
    xs = [torch.bernoulli(torch.full((B, D), 0.3), generator=g).to(DEV) for _ in range(6)]
    cfg = net.VaeConfig(optimizer="adam", lr=1e-3, beta_init=1e-4, beta_fin=1.0, beta_annealing=10, weight_avg="polyak", weight_avg_start=1)

    def run(graph, steps, resume=None):
        net.manual_seed(99)
        eng = net.VaeEngine(build(nd, z, "elu", sd0), cfg, batch_size=B, graph=graph)
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
        assert torch.equal(a.avg, other.avg) and a._n_avg() == other._n_avg() == 5
    # the step's draws are the documented elements at Philox offset RNG_STRIDE * step (+ 0), read through the state block
    want0, want1 = torch.empty(B, nd, device=DEV), torch.empty(B, z, device=DEV)
    L.call("ardae_philox_normal_at", want0, want0.numel(), 99, a.RNG_STRIDE * a.step_count, None, 0)
    L.call("ardae_philox_normal_at", want1, want1.numel(), 99, a.RNG_STRIDE * a.step_count, None, (B * nd + 3) // 4 * 4)
    assert a.step_count == 6 and torch.equal(a.eps, torch.cat([want0, want1], 1))
    assert not torch.equal(la[0], la[1])


# ---- 5. IWAE evaluation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_iwae_on_injected_draws_against_the_float64_fixture(golden_dir, case):
    fx = load(golden_dir, "vae_" + case)
    m, B, nd, z, act = from_fixture(fx)
    x, eps, fwd_eps = cuda(fx["x"]), cuda(fx["lp/eps"]), cuda(fx["eps"])
    k = int(eps.size(1))
    eng = net.VaeEngine(m, net.VaeConfig(), batch_size=B)
    elbo, logprob = eng.evaluate_iws(x, k, eps=eps, fwd_eps=fwd_eps)
    print(f"{case}: logprob {logprob:.7f} / {float(fx['lp/value_f64']):.7f}, elbo {elbo:.6f}")
    assert relerr(logprob, fx["lp/value_f64"]) <= TOL_IWAE
    assert relerr(float(m.logprob(x, sample_size=k, eps=eps)), fx["lp/value_f64"]) <= TOL_IWAE
    # elbo = -(recon + kld + aux_kld) of a forward on the same draw
    assert relerr(elbo, -(float(fx["b1/recon_f64"]) + float(fx["b1/kld_f64"]))) <= TOL_MEAN
    _, _, _, _, recon, kld = m(x, beta=1.0, eps=fwd_eps)
    assert relerr(elbo, -(float(recon) + float(kld))) <= 1e-6
    # row by row against the restatement
    rows = m.logprob_rows(x, k, eps=eps)
    want = logprob_rows(auxconv_params(fx, torch.float64), act, torch.tensor(fx["x"]).double(), torch.tensor(fx["lp/eps"]).double())
    assert rel(rows.cpu(), want) <= TOL_IWAE


@pytest.mark.parametrize("B,k", [(3, 16), (5, 4)])
def test_aux_iwae_draw_against_float64_with_guard_rows(B, k):
    nd, zd, act = 11, 6, "elu"
    m = seeded(nd, zd, act, B * k)
    x = torch.bernoulli(torch.full((B, D), 0.3))
    eps = torch.randn(B, k, nd + zd)
    mu0, lv0 = m.encode_stats(x.to(DEV))
    R = B * k
    z, logq, eps_out = guarded(R, zd), guarded(R, 1), guarded(R, nd + zd)
    wsf = L.query("ardae_model_workspace_floats", m._desc, B, k, 4)
    ws = torch.full((wsf + 4096,), NAN, device=DEV)
    L.call("ardae_vae_aux_iwae_draw", m._desc, m._flat, m._packed_weights(), x.to(DEV), mu0, lv0, eps.to(DEV), B, k, 0, 0, 0, 0, ws, wsf, z, logq, eps_out)
    zw, lw = logq_rows(p64_of(m), act, x.double(), eps.double())
    for buf, what in ((z, "z_out"), (logq, "logq"), (eps_out, "eps_out")):
        check_guard(buf, R, what)
    assert bool(torch.isnan(ws[wsf:]).all())
    assert torch.equal(eps_out[:R].cpu(), eps.view(R, nd + zd))
    assert rel(z[:R].cpu(), zw) <= TOL_LATENT
    print(f"aux_iwae_draw kind 17 B={B} k={k}: logq rel L2 {rel(logq[:R, 0].cpu(), lw):.3g}")
    assert rel(logq[:R, 0].cpu(), lw) <= TOL_MEAN


def test_iwae_own_draws_do_not_depend_on_the_chunking():
    """136 images at k = 4: one chunk against chunks of 64.  Every call runs on fixed groups (64 images for the statistics and the ELBO pass, 32 for
    the stages and the decoder), so elbo and logprob are equal to the bit."""
    N, k, nd, zd = 136, 4, 10, 6
    m = seeded(nd, zd, "softplus", 8)
    x = torch.bernoulli(torch.full((N, D), 0.3)).to(DEV)
    probe = net.GaussianIwaeEvaluator(m, k)
    assert probe.plan(N) == [(0, N)]
    results = []
    for budget, chunks in ((None, [(0, 136)]), (probe.floats_per_chunk(100), [(0, 64), (64, 128), (128, 136)])):
        ev = probe if budget is None else net.GaussianIwaeEvaluator(m, k, max_workspace_floats=budget)
        assert ev.plan(N) == chunks
        net.manual_seed(21)
        recon, kld, rows = ev.evaluate_rows(x)
        net.manual_seed(21)
        results.append(((recon.clone(), kld.clone(), rows.clone()), ev.evaluate(x)))
    assert all(torch.equal(a, b) for a, b in zip(results[1][0], results[0][0]))
    assert results[1][1] == results[0][1]                          # (elbo, logprob), to the bit
    # the ELBO rows are a forward's: the same draws through the model give their means
    e0, e1 = torch.empty(N, nd, device=DEV), torch.empty(N, zd, device=DEV)
    L.call("ardae_philox_normal_at", e0, e0.numel(), 21, rng.HOST_STREAM | 0, None, 0)
    L.call("ardae_philox_normal_at", e1, e1.numel(), 21, rng.HOST_STREAM | 1, None, 0)
    _, _, _, _, rec_mean, kld_mean = m(x, beta=1.0, eps=torch.cat([e0, e1], 1))
    assert relerr(results[0][0][0].double().mean(), rec_mean) <= TOL_MEAN and relerr(results[0][0][1].double().mean(), kld_mean) <= TOL_MEAN
    # the importance samples' draws are the documented elements of the next two offsets
    i0, i1 = torch.empty(N, k, nd, device=DEV), torch.empty(N, k, zd, device=DEV)
    L.call("ardae_philox_normal_at", i0, i0.numel(), 21, rng.HOST_STREAM | 2, None, 0)
    L.call("ardae_philox_normal_at", i1, i1.numel(), 21, rng.HOST_STREAM | 3, None, 0)
    net.manual_seed(33)
    assert torch.equal(probe.evaluate_rows(x, eps=torch.cat([i0, i1], 2), fwd_eps=torch.cat([e0, e1], 1))[2], results[0][0][2])
    net.manual_seed(22)
    assert not torch.equal(probe.evaluate_rows(x)[2], results[0][0][2])


def test_iwae_runs_under_the_averaged_weights_and_puts_the_trained_ones_back():
    B, nd, zd = 8, 10, 6
    m = seeded(nd, zd, "softplus", 9)
    eng = net.VaeEngine(m, net.VaeConfig(lr=1e-3, weight_avg="polyak", weight_avg_start=1, weight_avg_decay=0.5), batch_size=B)
    net.manual_seed(1)
    for _ in range(4):
        eng.step(torch.bernoulli(torch.full((B, D), 0.3)).to(DEV))
    trained = m._flat.clone()
    avg = eng.averaged_params().clone()
    assert not torch.equal(avg, trained) and bool(torch.isfinite(trained).all()) and bool(torch.isfinite(avg).all())
    x = torch.bernoulli(torch.full((12, D), 0.3)).to(DEV)
    eps, fwd_eps = torch.randn(12, 16, nd + zd, device=DEV), torch.randn(12, nd + zd, device=DEV)
    got = eng.evaluate_iws(x, 16, eps=eps, fwd_eps=fwd_eps)
    assert torch.equal(m._flat, trained)
    other = build(nd, zd, "softplus")
    with torch.no_grad():
        other._flat.copy_(avg)
    other.mark_dirty()
    assert net.GaussianIwaeEvaluator(other, 16).evaluate(x, eps, fwd_eps) == got
    with torch.no_grad():
        other._flat.copy_(trained)
    other.mark_dirty()
    assert net.GaussianIwaeEvaluator(other, 16).evaluate(x, eps, fwd_eps) != got


def test_drop_in_route_equals_the_engine(golden_dir):
    fx = load(golden_dir, "vae_traj_auxconv")
    cfg = traj_config(fx)
    me, B, nd, z, act = from_fixture(fx)
    eng = net.VaeEngine(me, cfg, batch_size=B)
    md = from_fixture(fx)[0]
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


# ---- 6. the decoder's last two stages in one launch ----------------------------------------------------------------------------------
R_MAX = 70
# The bound on the fused kernel (variant 1) is measured against the existing path: the unfused launches' own relative L2 error to float64 on the
# same inputs, times 2 for the different summation order, floored at the fp32 level the residual-conv tail's test uses (TOL_LATENT = 1e-5).
# Measured on one MI355X (printed by the test below): see the docstring of test_tail_kernel_against_float64_and_the_unfused_launches.


def padded_u1(R, seed):
    """u1 [R, 8, 8, 32] from N(0, 1) with the pad positions (row 7, column 7) zeroed, as conv_decode_fwd leaves them"""
    u1 = torch.randn(R, 8, 8, 32, generator=torch.Generator().manual_seed(seed))
    u1[:, 7, :, :] = 0.0
    u1[:, :, 7, :] = 0.0
    return u1.contiguous()


@pytest.fixture(scope="module")
def tail_case(golden_dir):
    """The softplus fixture's decoder weights, one u1 [70, 8, 8, 32] and its float64 logits, shared by the tests below and left unchanged"""
    fx = load(golden_dir, "vae_" + CASES[0])
    m, _, _, _, act = from_fixture(fx)
    u1 = padded_u1(R_MAX, 7502)
    return m, act, u1.to(DEV), tail_logit(auxconv_params(fx, torch.float64), act, u1.double())


def tail(m, u1, variant):
    """-> logits [R, 784] of ardae_conv_tail on NaN-filled buffers, guard rows checked behind the logits and the workspace"""
    R = u1.size(0)
    wsf = L.query("ardae_conv_tail_workspace_floats", m._desc, R, variant)
    assert (wsf > 0) == (variant == 2 or (variant == 0 and KNOB_ON))
    ws = torch.full((wsf + 4096,), NAN, device=DEV)
    out = guarded(R, D)
    L.call("ardae_conv_tail", m._desc, m._flat, m._packed_weights(), u1, R, variant, ws, wsf, out)
    check_guard(out, R, f"tail variant {variant} logits")
    assert bool(torch.isnan(ws[wsf:]).all())
    return out[:R].clone()


def check_tail(m, u1, want, what):
    fused, unfused = tail(m, u1, 1), tail(m, u1, 2)
    e1, e2 = rel(fused.cpu(), want), rel(unfused.cpu(), want)
    bound = max(2.0 * e2, TOL_LATENT)
    print(f"tail {what}: fused against float64 rel L2 {e1:.3g}, unfused {e2:.3g}, bound {bound:.3g}; fused against unfused {rel(fused.cpu(), unfused.cpu()):.3g}")
    assert e2 <= TOL_LATENT and e1 <= bound
    return fused, unfused


@pytest.mark.parametrize("R", [1, 5, R_MAX])
def test_tail_kernel_against_float64_and_the_unfused_launches(tail_case, R):
    """conv_tail_kernel (variant 1) and the four unfused launches (variant 2) against the float64 restatement of stages A and B.  Measured on one
    MI355X at R = 70: fused 1.99e-7, unfused 1.21e-7 relative L2 to float64, so the bound is its floor, 1e-5 (2 x 1.21e-7 lies below it); under the
    other activations at R = 3 the fused kernel measured 1.6e-7 .. 3.4e-7, the unfused launches 0.8e-7 .. 1.5e-7.  The kernel is the library's
    choice (variant 0): 0.375 ms against 1.359 ms at the evaluator's 8192 rows (profiles/vae_auxconv_baseline_timing.json)."""
    m, act, u1, want = tail_case
    fused, unfused = check_tail(m, u1[:R].contiguous(), want[:R], f"R={R} {act}")
    default = 1 if L.query("ardae_conv_tail_workspace_floats", m._desc, R, 0) == 0 else 2
    assert default == 1                                                      # the library's choice is the kernel (README: the measurement)
    assert torch.equal(tail(m, u1[:R].contiguous(), 0), fused if default == 1 else unfused)


@pytest.mark.parametrize("act", ALL_ACTS)
def test_tail_kernel_under_every_activation(act):
    m = seeded(10, 6, act, 7600)
    u1 = padded_u1(3, 7601)
    check_tail(m, u1.to(DEV), tail_logit(p64_of(m), act, u1.double()), f"R=3 {act}")


def test_tail_kernel_rows_do_not_depend_on_the_rows_of_the_call(tail_case):
    m, _, u1, _ = tail_case
    assert torch.equal(tail(m, u1, 1)[:5], tail(m, u1[:5].contiguous(), 1))


def decode(m, z):
    """-> logits [R, 784] of ardae_model_decode and the u1 [R, 8, 8, 32] it left in its workspace (the decode-only carve opens with d1 [R, 300],
    d2 [R, 512], g0 [R, 512], c1 [R, 16, 800], u1, each rounded up to 64 floats)"""
    R = z.size(0)
    wsf = L.query("ardae_model_workspace_floats", m._desc, R, 1, 2)
    ws = torch.full((wsf + 4096,), NAN, device=DEV)
    out = guarded(R, D)
    L.call("ardae_model_decode", m._desc, m._flat, m._packed_weights(), z, R, ws, wsf, out, None)
    check_guard(out, R, "decode out0")
    assert bool(torch.isnan(ws[wsf:]).all())
    al = lambda n: (n + 63) // 64 * 64      # noqa: E731
    off = al(R * 300) + 2 * al(R * 512) + al(R * 12800)
    return out[:R].clone(), ws[off:off + R * 2048].view(R, 8, 8, 32).clone()


def other_kinds():
    """One small model of each kind that shares the conv decoder"""
    torch.manual_seed(7700)
    return {2: net.ConvIPVAE(z_dim=6, noise_dim=4).to(DEV), 4: net.MNISTConvAuxIPVAE(z0_dim=4, z_dim=6).to(DEV), 11: net.MNISTConvVAE(z_dim=6).to(DEV)}


def test_decode_only_path_and_the_other_kinds(tmp_path):
    """ardae_model_decode of kind 17 equals the u1 -> tail route, to the bit, and float64.  Under ARDAE_CONV_TAIL_UNFUSED=1 (a child process of the
    next test) it runs the unfused launches - it equals variant 2, its workspace grows - while kinds 2, 4 and 11 give the bits the parent left in a
    file: the new path does not leak into them."""
    unfused = KNOB_ON
    R = 11
    m = seeded(10, 6, "elu", 7701)
    z = torch.randn(R, 6, generator=torch.Generator().manual_seed(7702))
    logit, u1 = decode(m, z.to(DEV))
    assert bool(torch.isfinite(u1).all()) and float(u1[:, 7].abs().max()) == 0.0 and float(u1[:, :, 7].abs().max()) == 0.0
    assert torch.equal(logit, tail(m, u1, 2 if unfused else 1)) and torch.equal(logit, tail(m, u1, 0))
    assert (L.query("ardae_conv_tail_workspace_floats", m._desc, R, 0) > 0) == unfused
    assert (L.query("ardae_model_workspace_floats", m._desc, 1024, 1, 2) > L.query("ardae_conv_tail_workspace_floats", m._desc, 1024, 2)) == unfused
    assert rel(logit.cpu(), decode_logit(p64_of(m), "elu", z.double())) <= TOL_LATENT
    assert torch.equal(m.decode_params(z.to(DEV))[0], logit)
    u = torch.rand(R, D, generator=torch.Generator().manual_seed(7703))
    xs, mean, zz = m.generate(R, z=z.to(DEV), dec_noise=u.to(DEV))
    assert torch.equal(zz.cpu(), z) and torch.equal(mean, torch.sigmoid(logit)) and rel(xs.cpu(), relaxed_sample(logit.double().cpu(), u.double())) <= 1e-4
    others = {}
    for kind, mod in other_kinds().items():
        wsf = L.query("ardae_model_workspace_floats", mod._desc, R, 1, 2)
        ws, out = torch.full((wsf,), NAN, device=DEV), guarded(R, D)
        L.call("ardae_model_decode", mod._desc, mod._flat, mod._packed_weights(), z.to(DEV), R, ws, wsf, out, None)
        check_guard(out, R, f"kind {kind} decode")
        others[kind] = out[:R].cpu()
    path = os.environ.get("AUXCONV_PARENT_OUTPUTS")
    if unfused:
        assert path, "the child process compares against the parent's outputs"
        parent = torch.load(path)
        for kind, out in others.items():
            assert torch.equal(out, parent[kind]), f"kind {kind}: ardae_model_decode changed under the knob"
        assert torch.equal(logit.cpu(), parent["variant2"])
        print("decode-only path, unfused launches: kind 17 equals variant 2; kinds 2, 4 and 11 unchanged")
    else:
        others["variant2"] = tail(m, u1, 2).cpu()
        torch.save(others, tmp_path / "parent.pt")


def test_decode_only_path_with_the_unfused_knob(tmp_path):
    """The library reads its debug knobs once per process, so the test above is re-run in a child process with the knob set."""
    test_decode_only_path_and_the_other_kinds(tmp_path)
    env = dict(os.environ, AUXCONV_PARENT_OUTPUTS=str(tmp_path / "parent.pt"), **KNOB_ENV)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "decode_only_path_and_the_other_kinds"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout and "kinds 2, 4 and 11 unchanged" in r.stdout, r.stdout[-500:]
