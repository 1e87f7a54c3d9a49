"""Auxiliary-variable Gaussian baselines on the device (ardae_model_desc.kind 14 / 15; vae.py --model auxmnist / auxtoy): forward / backward against
the reference's fixtures through the C ABI and through autograd, the pair-KL rows, the in-kernel draws, recipe widths against the float64 restatement
of tests/test_vae_aux_baseline.py, the engine's trajectory, replay == eager, resume, the three-stage IWAE evaluation, the drop-in route.

Tolerances are those of tests/test_vae_baseline_gpu.py, the project's for this driver: scalar losses 1e-4 relative, recon / kld means 2e-5, gradients
2e-3 relative L2 per tensor, updated parameters 5e-3 relative L2, IWAE log-probability 1e-4 against the float64 fixture, latents 1e-5 relative L2."""
import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import rng
from test_vae_aux_baseline import (BETAS, CASES, TRAJ, aux_params, forward_backward, load, logprob_rows, logq_rows, pair_kld_rows, params64, rel, shape_of,
                                   summary_err)

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_LOSS, TOL_MEAN, TOL_GRAD, TOL_PARAM, TOL_IWAE, TOL_LATENT = 1e-4, 2e-5, 2e-3, 5e-3, 1e-4, 1e-5


def relerr(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def build(family, D, nd, h, z, nl, act, clip=None, sd=None):
    ctor = net.MNISTAuxVAE if family == "mnist" else net.ToyAuxVAE
    m = ctor(input_dim=D, noise_dim=nd, h_dim=h, z_dim=z, nonlinearity=act, num_hidden_layers=nl, clip_logvar=clip)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV)


def from_fixture(fx):
    family, (B, D, h, nd, z, nl), act, clip = shape_of(fx)
    return build(family, D, nd, h, z, nl, act, clip, aux_params(fx)), (family, B, D, h, nd, z, nl, act, clip)


def cuda(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV).contiguous()


def np64(t):
    return t.detach().double().cpu().numpy()


def abi_forward_backward(m, x, eps, beta, loss_scale, seed=0, offset=0):
    """-> z, losses [3], flat grads, eps_out through ardae_vae_forward / ardae_vae_backward on NaN-filled buffers"""
    B = x.size(0)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)      # noqa: E731
    ws = nan(L.query("ardae_model_workspace_floats", m._desc, B, 1, 1))
    z, eps_out, losses = nan(B, m.z_dim), nan(B, m._eps_width), nan(3)
    L.call("ardae_vae_forward", m._desc, m._flat, m._packed_weights(), x, eps, B, beta, loss_scale, seed, offset, None, ws, ws.numel(), z, eps_out, losses)
    grads = torch.full_like(m._flat, float("nan"))          # (grads_beta 0: whatever was there is overwritten)
    L.call("ardae_vae_backward", m._desc, m._flat, m._packed_weights(), x, B, beta, loss_scale, ws, ws.numel(), grads, 0.0)
    if eps is not None:
        assert torch.equal(eps_out, eps)
    return z, losses, grads, eps_out, ws


def check_losses(got, want, what):
    loss, recon, kld = (float(v) for v in got)
    print(f"{what}: loss {loss:.7g} / {float(want['loss']):.7g}, recon {recon:.7g} / {float(want['recon']):.7g}, kld {kld:.7g} / {float(want['kld']):.7g}")
    assert relerr(loss, want["loss"]) <= TOL_LOSS
    assert relerr(recon, want["recon"]) <= TOL_MEAN and relerr(kld, want["kld"]) <= TOL_MEAN


def check_grads(m, views, full, summ, what):
    """full: {name: gradient}; summ: {name: [L2, sum, first 8]} for the tensors a fixture keeps as summaries"""
    worst = 0.0
    for (name, _), g in zip(m.named_parameters(), views):
        assert bool(torch.isfinite(g).all()), (what, name)
        e = rel(np64(g), full[name]) if name in full else summary_err(np64(g), summ[name])
        worst = max(worst, e)
        assert e <= TOL_GRAD, (what, name, e)
    print(f"{what}: worst gradient tensor {worst:.3g}")


# ---- 1. forward / backward against the reference's fixtures ------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_forward_backward_against_the_reference(golden_dir, case):
    fx = load(golden_dir, "vae_" + case)
    m, (family, B, D, h, nd, z, nl, act, clip) = from_fixture(fx)
    x, eps, dec = cuda(fx["x"]), cuda(fx["eps"]), cuda(fx["dec_noise"])
    mu0, lv0 = m.encode_stats(x)
    assert mu0.shape == lv0.shape == (B, nd)
    assert rel(np64(mu0), fx["mu0"]) <= TOL_LATENT and rel(np64(lv0), fx["lv0"]) <= TOL_LATENT
    for b, beta in BETAS.items():
        want = {k: fx[f"{b}/{k}"] for k in ("loss", "recon", "kld")}
        full = {k[len(b) + 3:]: v for k, v in fx.items() if k.startswith(f"{b}/g/")}
        summ = {k[len(b) + 4:]: v for k, v in fx.items() if k.startswith(f"{b}/gs/")}
        # the C ABI
        zc, losses, grads, _, ws = abi_forward_backward(m, x, eps, beta, 1.0 / D)
        assert rel(np64(zc), fx[f"{b}/z"]) <= TOL_LATENT
        check_losses(losses.tolist(), want, f"{case} {b} abi")
        check_grads(m, m.param_views(grads), full, summ, f"{case} {b} abi")
        # grads = grads_beta * grads + ...: a second call on top of the first doubles them
        acc = grads.clone()
        L.call("ardae_vae_backward", m._desc, m._flat, m._packed_weights(), x, B, beta, 1.0 / D, ws, ws.numel(), acc, 1.0)
        assert rel(np64(acc), 2 * np64(grads)) <= 1e-6
        # the module's autograd
        for p in m.parameters():
            p.grad = None
        xs, mean, zm, loss, recon, kld = m(x, beta=beta, eps=eps, dec_noise=dec)
        (loss / float(D)).backward()
        assert torch.equal(zm, zc) and not recon.requires_grad and not kld.requires_grad
        check_losses((loss.detach(), recon, kld), want, f"{case} {b} module")
        check_grads(m, [p.grad for p in m.parameters()], full, summ, f"{case} {b} module")
        assert rel(np64(mean), fx[f"{b}/mean"]) <= TOL_LATENT
        assert rel(np64(xs), fx[f"{b}/x_sample"]) <= 1e-4        # the decoder's relaxed-Bernoulli / Gaussian sample on the injected draw


# ---- 2. the pair KL -------------------------------------------------------------------------------------------------------------------
PAIR_SHAPES = [(1, 1), (5, 10), (70, 100), (129, 128)]


def pair_inputs(B, n):
    g = torch.Generator().manual_seed(100 * B + n)
    return [(torch.randn(B, n, generator=g) * s).to(DEV).contiguous() for s in (1.0, 1.5, 1.0, 0.7)]      # mu1, lv1, mu2, lv2


@pytest.fixture(scope="module")
def pair_at_129():
    mu1, lv1, mu2, lv2 = pair_inputs(129, 128)
    out = torch.full((130,), float("nan"), device=DEV)
    L.call("ardae_vae_pair_kld_rows", mu1, lv1, mu2, lv2, 129, 128, out)
    return (mu1, lv1, mu2, lv2), out


@pytest.mark.parametrize("B,n", PAIR_SHAPES)
def test_pair_kld_rows_against_float64(B, n, pair_at_129):
    if (B, n) == (129, 128):
        (mu1, lv1, mu2, lv2), out = pair_at_129
    else:
        mu1, lv1, mu2, lv2 = pair_inputs(B, n)
        out = torch.full((B + 1,), float("nan"), device=DEV)
        L.call("ardae_vae_pair_kld_rows", mu1, lv1, mu2, lv2, B, n, out)
    want = pair_kld_rows(np64(mu1), np64(lv1), np64(mu2), np64(lv2))
    assert bool(torch.isnan(out[B])) and rel(np64(out[:B]), want) <= TOL_MEAN
    assert float(np.max(np.abs(np64(out[:B]) - want) / np.abs(want))) <= TOL_MEAN      # row by row, not only in the norm


def test_pair_kld_row_bits_do_not_depend_on_the_batch(pair_at_129):
    (mu1, lv1, mu2, lv2), out = pair_at_129
    for r0 in (0, 63, 126):
        small = torch.empty(3, device=DEV)
        L.call("ardae_vae_pair_kld_rows", *(t[r0:r0 + 3].contiguous() for t in (mu1, lv1, mu2, lv2)), 3, 128, small)
        assert torch.equal(small, out[r0:r0 + 3]), r0


@pytest.mark.parametrize("B,n", PAIR_SHAPES)
def test_the_forward_adds_the_pair_kld_into_the_heads_rows(B, n):
    """losses[2] = mean(kld + aux_kld): the head's KL rows (ardae_vae_kld_rows on the head's statistics) + ardae_vae_pair_kld_rows, in float64"""
    torch.manual_seed(B + n)
    m = build("toy", 2, n, 24, 3, 2, "tanh", "spm6")
    x, eps = torch.randn(B, 2), torch.randn(B, n + 3)
    out, _ = forward_backward("toy", {k: np64(v) for k, v in m.named_parameters()}, "tanh", "spm6", x.double().numpy(), eps.double().numpy(), 1.0, 1.0)
    _, losses, _, _, _ = abi_forward_backward(m, x.to(DEV), eps.to(DEV), 1.0, 1.0)
    check_losses(losses.tolist(), out, f"pair KL in the forward B={B} n={n}")


# ---- 3. the in-kernel draws ----------------------------------------------------------------------------------------------------------
def test_eps_null_draws_the_documented_philox_elements():
    B, nd, zd = 7, 5, 3                                    # B nd = 35: the second draw starts at element 36
    torch.manual_seed(1)
    m = build("mnist", 20, nd, 24, zd, 2, "softplus", "hard")
    x = torch.bernoulli(torch.full((B, 20), 0.3)).to(DEV)
    z, losses, grads, eps_out, _ = abi_forward_backward(m, x, None, 0.7, 1.0 / 20, seed=11, offset=5)
    want0, want1 = torch.empty(B, nd, device=DEV), torch.empty(B, zd, device=DEV)
    L.call("ardae_philox_normal_at", want0, want0.numel(), 11, 5, None, 0)
    L.call("ardae_philox_normal_at", want1, want1.numel(), 11, 5, None, (B * nd + 3) // 4 * 4)
    assert torch.equal(eps_out, torch.cat([want0, want1], 1))
    z2, losses2, grads2, _, _ = abi_forward_backward(m, x, eps_out.clone(), 0.7, 1.0 / 20)
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
    assert xs.shape == mean.shape == (6, 20) and zg.shape == (6, zd) and bool(torch.isfinite(xs).all())


# ---- 4. recipe widths against the live float64 restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("family,D,nd,h,z,nl,act,B", [("mnist", 784, 100, 300, 32, 2, "softplus", 70), ("toy", 2, 2, 64, 2, 1, "tanh", 129)])
def test_recipe_width_against_the_float64_restatement(family, D, nd, h, z, nl, act, B):
    torch.manual_seed(17)
    m = build(family, D, nd, h, z, nl, act)
    x = (torch.bernoulli(torch.full((B, D), 0.3)) if family == "mnist" else torch.randn(B, D))
    eps = torch.randn(B, nd + z)
    p64 = {k: np64(v) for k, v in m.named_parameters()}
    for beta in (1.0, 0.3):
        out, grads = forward_backward(family, p64, act, None, x.double().numpy(), eps.double().numpy(), beta, 1.0 / D)
        zc, losses, g, _, _ = abi_forward_backward(m, x.to(DEV), eps.to(DEV), beta, 1.0 / D)
        assert rel(np64(zc), out["z"]) <= TOL_LATENT
        check_losses(losses.tolist(), out, f"{family} recipe width beta {beta}")
        check_grads(m, m.param_views(g), grads, {}, f"{family} recipe width beta {beta}")


# ---- 5. the engine's trajectory, replay == eager, resume ----------------------------------------------------------------------------
def traj_config(fx, **kw):
    return net.VaeConfig(lr=float(fx["cfg/lr"]), beta1=float(fx["cfg/beta1"]), beta_init=float(fx["cfg/beta_init"]), beta_fin=float(fx["cfg/beta_fin"]),
                         beta_annealing=int(fx["cfg/beta_annealing"]), **kw)


@pytest.mark.parametrize("name", TRAJ)
def test_engine_trajectory_against_the_reference(golden_dir, name):
    fx = load(golden_dir, "vae_traj_" + name)
    m, (family, B, D, h, nd, z, nl, act, clip) = from_fixture(fx)
    cfg = traj_config(fx)
    eng = net.VaeEngine(m, cfg, batch_size=B)
    assert eng.loss_scale == 1.0 / D and eng.eps.shape == (B, nd + z)
    for s in range(int(fx["cfg/steps"])):
        eng.step(cuda(fx[f"{s}/x"]), eps=cuda(fx[f"{s}/eps"]))
        st = eng.stats()
        assert st["beta"] == float(np.float32(cfg.beta_at(s))) == eng.beta_of_step(s + 1), (s, st["beta"])
        check_losses((st["loss"], st["recon"], st["kld"]), {k: fx[f"{s}/{k}"] for k in ("loss", "recon", "kld")}, f"{name} step {s}")
        worst = max(summary_err(np64(p), fx[f"{s}/ps/{k}"]) for k, p in m.named_parameters())
        print(f"{name} step {s}: worst parameter summary {worst:.3g}")
        assert worst <= TOL_PARAM
    assert eng.step_count == 4 and eng.stats()["beta"] == 1.0


@pytest.mark.parametrize("family,optimizer,avg", [("mnist", "adam", "swa"), ("toy", "amsgrad", "polyak")])
def test_replay_equals_eager_and_resume_continues_to_the_same_bits(family, optimizer, avg):
    D, nd, h, z, B = (36, 10, 48, 8, 10) if family == "mnist" else (2, 5, 40, 3, 12)
    torch.manual_seed(3)
    sd0 = {k: v.clone() for k, v in build(family, D, nd, h, z, 2, "softplus", "spm4").state_dict().items()}
    g = torch.Generator().manual_seed(4)
    xs = [(torch.bernoulli(torch.full((B, D), 0.3), generator=g) if family == "mnist" else torch.randn(B, D, generator=g)).to(DEV) for _ in range(6)]
    cfg = net.VaeConfig(optimizer=optimizer, lr=1e-3, beta_init=1e-4, beta_fin=1.0, beta_annealing=10, weight_avg=avg, weight_avg_start=1)

    def run(graph, steps, resume=None):
        net.manual_seed(99)
        m = build(family, D, nd, h, z, 2, "softplus", "spm4", sd0)
        eng = net.VaeEngine(m, cfg, batch_size=B, graph=graph)
        if resume is not None:
            eng.load_state_dict(resume)
        losses, draws, saved = [], [], None
        for s in steps:
            eng.step(xs[s])
            losses.append(eng.losses.clone())
            draws.append(eng.eps.clone())
            if s == 2:
                saved = eng.state_dict()
        return eng, losses, draws, saved

    a, la, da, sd3 = run(True, range(6))
    assert a._graph is not None                                     # captured at the third call, while beta was still moving
    b, lb, _, _ = run(False, range(6))
    assert b._graph is None
    c, lc, _, _ = run(True, range(3, 6), resume=sd3)
    for other, lo in ((b, lb), (c, lc)):
        assert torch.equal(a.model._flat, other.model._flat)
        for t, u in zip(a.opt.buffers(), other.opt.buffers()):
            assert torch.equal(t, u)
        assert all(torch.equal(x, y) for x, y in zip(la[-len(lo):], lo))
        assert torch.equal(a.state, other.state) and torch.equal(a.eps, other.eps)
        assert torch.equal(a.avg, other.avg) and a._n_avg() == other._n_avg() == 5
    # the step's draws are the documented elements at Philox offset RNG_STRIDE * step (+ 0), read through the state block ...
    want0, want1 = torch.empty(B, nd, device=DEV), torch.empty(B, z, device=DEV)
    L.call("ardae_philox_normal_at", want0, want0.numel(), 99, a.RNG_STRIDE * a.step_count, None, 0)
    L.call("ardae_philox_normal_at", want1, want1.numel(), 99, a.RNG_STRIDE * a.step_count, None, (B * nd + 3) // 4 * 4)
    assert a.step_count == 6 and torch.equal(a.eps, torch.cat([want0, want1], 1))
    # ... and two consecutive steps draw disjoint numbers
    for s in range(5):
        assert not bool(torch.isin(da[s].flatten(), da[s + 1].flatten()).any()), s
    assert not torch.equal(la[0], la[1])


# ---- 6. IWAE evaluation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_iwae_on_injected_draws_against_the_float64_fixture(golden_dir, case):
    fx = load(golden_dir, "vae_" + case)
    m, (family, B, D, h, nd, z, nl, act, clip) = from_fixture(fx)
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
    want = logprob_rows(family, params64(fx), act, clip, fx["x"].astype(np.float64), fx["lp/eps"].astype(np.float64))
    assert rel(np64(rows), want) <= TOL_IWAE


@pytest.mark.parametrize("B,k", [(3, 16), (5, 4)])
def test_aux_iwae_draw_against_float64_with_guard_rows(B, k):
    torch.manual_seed(B * k)
    D, nd, zd = 20, 11, 6
    m = build("mnist", D, nd, 24, zd, 2, "elu", "2tanh")
    x = torch.bernoulli(torch.full((B, D), 0.3))
    eps = torch.randn(B, k, nd + zd)
    mu0, lv0 = m.encode_stats(x.to(DEV))
    R = B * k
    z, logq, eps_out = (torch.full(s, float("nan"), device=DEV) for s in ((R + 1, zd), (R + 1,), (R + 1, nd + zd)))
    ws = torch.full((L.query("ardae_model_workspace_floats", m._desc, B, k, 4),), float("nan"), device=DEV)
    L.call("ardae_vae_aux_iwae_draw", m._desc, m._flat, m._packed_weights(), x.to(DEV), mu0, lv0, eps.to(DEV), B, k, 0, 0, 0, 0, ws, ws.numel(), z, logq, eps_out)
    zw, lw = logq_rows("mnist", {n: np64(v) for n, v in m.named_parameters()}, "elu", "2tanh", x.double().numpy(), eps.double().numpy())
    assert bool(torch.isnan(z[R]).all()) and bool(torch.isnan(logq[R])) and bool(torch.isnan(eps_out[R]).all())      # the guard rows
    assert torch.equal(eps_out[:R].cpu(), eps.view(R, nd + zd))
    assert rel(np64(z[:R]), zw) <= TOL_LATENT
    print(f"aux_iwae_draw B={B} k={k}: logq rel L2 {rel(np64(logq[:R]), lw):.3g}")
    assert rel(np64(logq[:R]), lw) <= TOL_MEAN


def test_iwae_own_draws_do_not_depend_on_the_chunking():
    torch.manual_seed(8)
    N, k, D, nd, zd = 40, 16, 36, 10, 8
    m = build("mnist", D, nd, 48, zd, 2, "softplus", "spm4")
    x = torch.bernoulli(torch.full((N, D), 0.3)).to(DEV)
    probe = net.GaussianIwaeEvaluator(m, k)
    results = []
    for c, nchunks in ((40, 1), (16, 3), (8, 5)):
        ev = net.GaussianIwaeEvaluator(m, k, max_workspace_floats=probe.floats_per_chunk(c))
        assert len(ev.plan(N)) == nchunks
        net.manual_seed(21)
        recon, kld, rows = ev.evaluate_rows(x)
        net.manual_seed(21)
        results.append(((recon.clone(), kld.clone(), rows.clone()), ev.evaluate(x)))
    for parts, result in results[1:]:
        assert all(torch.equal(a, b) for a, b in zip(parts, results[0][0]))
        assert result == results[0][1]                          # (elbo, logprob), to the bit
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
    with pytest.raises(ValueError, match="must be"):
        probe.evaluate_rows(x, eps=torch.zeros(N, k + 1, nd + zd, device=DEV))


def test_iwae_runs_under_the_averaged_weights_and_puts_the_trained_ones_back():
    torch.manual_seed(9)
    B, D, nd, zd = 8, 36, 10, 8
    m = build("mnist", D, nd, 48, zd, 2, "softplus")
    eng = net.VaeEngine(m, net.VaeConfig(lr=1e-2, weight_avg="polyak", weight_avg_start=1, weight_avg_decay=0.5), batch_size=B)
    net.manual_seed(1)
    for _ in range(4):
        eng.step(torch.bernoulli(torch.full((B, D), 0.3)).to(DEV))
    trained = m._flat.clone()
    avg = eng.averaged_params().clone()
    assert not torch.equal(avg, trained)
    x = torch.bernoulli(torch.full((12, D), 0.3)).to(DEV)
    eps, fwd_eps = torch.randn(12, 16, nd + zd, device=DEV), torch.randn(12, nd + zd, device=DEV)
    got = eng.evaluate_iws(x, 16, eps=eps, fwd_eps=fwd_eps)
    assert torch.equal(m._flat, trained)
    other = build("mnist", D, nd, 48, zd, 2, "softplus")
    with torch.no_grad():
        other._flat.copy_(avg)
    assert net.GaussianIwaeEvaluator(other, 16).evaluate(x, eps, fwd_eps) == got
    with torch.no_grad():
        other._flat.copy_(trained)
    other.mark_dirty()
    assert net.GaussianIwaeEvaluator(other, 16).evaluate(x, eps, fwd_eps) != got


# ---- 7. the drop-in route --------------------------------------------------------------------------------------------------------------
def test_drop_in_route_equals_the_engine(golden_dir):
    fx = load(golden_dir, "vae_traj_auxmnist")
    cfg = traj_config(fx)
    me, (family, B, D, h, nd, z, nl, act, clip) = from_fixture(fx)
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
            assert rel(np64(p), np64(q)) <= TOL_PARAM, (i_ep, name)
