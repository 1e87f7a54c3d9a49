"""The conv Gaussian-posterior baseline on the device (ardae_model_desc.kind 11; vae.py --model conv): forward / backward against the
reference's fixtures through the C ABI and through autograd, shapes the fixtures do not reach against the float64 restatement of
tests/test_vae_conv_baseline.py with NaN-filled buffers and guard rows, the Gaussian head at h = 800, the engine's trajectory, replay == eager,
resume, IWAE evaluation, the drop-in route.

Tolerances are the project's for these quantities, imported from tests/test_vae_baseline_gpu.py: scalar losses 1e-4 relative, recon / kld means
2e-5, gradients 2e-3 relative L2 per tensor, updated parameters 5e-3 relative L2, IWAE log-probability 1e-4 against the float64 fixture, latents
1e-5 relative L2."""
import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from test_ardae_uncond import rel
from test_vae_baseline import BETAS, load
from test_vae_baseline_gpu import TOL_GRAD, TOL_IWAE, TOL_LATENT, TOL_LOSS, TOL_MEAN, TOL_PARAM, check_losses, cuda, relerr
from test_vae_baseline import lin
from test_ardae_uncond import ACTS
from test_vae_conv_baseline import CASES, D, fixture_params, logprob_rows, loss_and_grads, recon_rows, relaxed_sample, trajectory

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def build(z, act, sd=None, **kw):
    m = net.MNISTConvVAE(z_dim=z, nonlinearity=act, **kw)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV)


def from_fixture(fx):
    B, z = (int(v) for v in fx["shape"])
    return build(z, str(fx["act"]), fixture_params(fx)), B, z


def p64_of(m):
    return {k: v.detach().double().cpu() for k, v in m.named_parameters()}


def guarded(rows, cols, extra=3):
    """[rows + extra, cols] of NaN: the call may write the first `rows` rows only"""
    return torch.full((rows + extra, cols), NAN, device=DEV)


def check_guard(buf, rows, what):
    assert bool(torch.isfinite(buf[:rows]).all()), f"{what}: a row below B was not written"
    assert bool(torch.isnan(buf[rows:]).all()), f"{what}: a row past B was written"


def abi_forward_backward(m, x, eps, beta, grads_beta=0.0, grads=None):
    """-> z, losses [3], flat grads through ardae_vae_forward / ardae_vae_backward on NaN-filled buffers: the workspace, every output, and guard
    rows behind each of them (and behind the workspace's declared end)"""
    B, z = x.size(0), m.z_dim
    wsf = L.query("ardae_model_workspace_floats", m._desc, B, 1, 1)
    ws = torch.full((wsf + 4096,), NAN, device=DEV)
    zo, eo, losses = guarded(B, z), guarded(B, z), guarded(3, 1)
    L.call("ardae_vae_forward", m._desc, m._flat, m._packed_weights(), x, eps, B, beta, 1.0 / D, 0, 0, None, ws, wsf, zo, eo, losses)
    n = m._flat.numel()
    g = torch.full((n + 64,), NAN, device=DEV)
    if grads is not None:
        g[:n] = grads
    L.call("ardae_vae_backward", m._desc, m._flat, m._packed_weights(), x, B, beta, 1.0 / D, ws, wsf, g, grads_beta)
    for buf, rows, what in ((zo, B, "z_out"), (eo, B, "eps_out"), (losses, 3, "losses")):
        check_guard(buf, rows, what)
    assert bool(torch.isnan(ws[wsf:]).all()) and bool(torch.isnan(g[n:]).all()) and bool(torch.isfinite(g[:n]).all())
    assert torch.equal(eo[:B], eps)
    return zo[:B].clone(), losses[:3, 0].clone(), g[:n].clone()


def check_grads64(m, views, want, what):
    """every gradient tensor in full against the float64 restatement"""
    worst = 0.0
    for (name, _), g in zip(m.named_parameters(), views):
        e = rel(g.cpu(), want[name])
        worst = max(worst, e)
        assert e <= TOL_GRAD, (what, name, e)
    print(f"{what}: worst gradient tensor against float64 {worst:.3g}")


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


# ---- 1. both fixtures, both betas --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_forward_backward_against_the_reference(golden_dir, case):
    fx = load(golden_dir, f"vae_conv_{case}")
    m, B, z = from_fixture(fx)
    act, p64 = str(fx["act"]), fixture_params(fx, torch.float64)
    x, eps, dec = cuda(fx["x"]), cuda(fx["eps"]), cuda(fx["dec_noise"])
    mu, lv = m.encode_stats(x)
    assert rel(mu.cpu(), fx["mu"]) <= TOL_LATENT and rel(lv.cpu(), fx["lv"]) <= TOL_LATENT
    zz, mu2, lv2 = m.encode(x.view(B, 1, 28, 28), eps=eps)
    assert torch.equal(mu2, mu) and torch.equal(lv2, lv) and rel(zz.cpu(), fx["b1/z"]) <= TOL_LATENT
    assert L.query("ardae_vae_head_fused_ok", m._desc) == 1       # this family's fused head is the default at every z <= 64 (README)
    for b, beta in BETAS.items():
        want = {k: fx[f"{b}/{k}"] for k in ("loss", "recon", "kld")}
        _, g64 = loss_and_grads(p64, act, x.double().cpu(), eps.double().cpu(), beta, 1.0 / D)
        # the C ABI
        zc, losses, grads = abi_forward_backward(m, x, eps, beta)
        assert rel(zc.cpu(), fx[f"{b}/z"]) <= TOL_LATENT
        check_losses(losses.tolist(), want, f"conv {case} {b} abi")
        check_grads_fixture(m, m.param_views(grads), fx, b, f"conv {case} {b} abi")
        check_grads64(m, m.param_views(grads), g64, f"conv {case} {b} abi")
        # grads = grads_beta * grads + ...: a second call on top of the first doubles them
        _, _, acc = abi_forward_backward(m, x, eps, beta, grads_beta=1.0, grads=grads)
        assert rel(acc.cpu(), 2 * grads.cpu()) <= 1e-6
        # the module's autograd
        for p in m.parameters():
            p.grad = None
        xs, mean, zm, loss, recon, kld = m(x, beta=beta, eps=eps, dec_noise=dec)
        (loss / float(D)).backward()
        assert torch.equal(zm, zc) and not recon.requires_grad and not kld.requires_grad
        check_losses((loss.detach(), recon, kld), want, f"conv {case} {b} module")
        check_grads_fixture(m, [p.grad for p in m.parameters()], fx, b, f"conv {case} {b} module")
        check_grads64(m, [p.grad for p in m.parameters()], g64, f"conv {case} {b} module")
        assert xs.shape == mean.shape == (B, D)
        assert rel(mean.cpu(), fx[f"{b}/mean"]) <= TOL_LATENT
        assert rel(xs.cpu(), fx[f"{b}/x_sample"]) <= 1e-4        # the decoder's relaxed-Bernoulli sample on the injected draw


# ---- 2. shapes the fixtures do not reach, against the float64 restatement ----------------------------------------------------------
@pytest.mark.parametrize("B,z,act", [(1, 32, "softplus"), (9, 32, "softplus"), (70, 6, "tanh")])
def test_other_batches_against_the_float64_restatement_with_guard_rows(B, z, act):
    """B = 1; one row past the head's 8-row tile; past a 64-row tile with the unaligned head.  Every buffer starts as NaN, so a read of something
    never written shows in the results, and nothing past B rows of any caller buffer (or past the workspace's declared size) may be written."""
    torch.manual_seed(100 + B)
    m = build(z, act)
    x, eps = torch.bernoulli(torch.full((B, D), 0.3)), torch.randn(B, z)
    p64 = p64_of(m)
    xd, ed = x.to(DEV), eps.to(DEV)
    for beta in (1.0, 0.3):
        out, g64 = loss_and_grads(p64, act, x.double(), eps.double(), beta, 1.0 / D)
        zc, losses, g = abi_forward_backward(m, xd, ed, beta)
        assert rel(zc.cpu(), out["z"]) <= TOL_LATENT
        check_losses(losses.tolist(), out, f"conv B={B} z={z} beta {beta}")
        check_grads64(m, m.param_views(g), g64, f"conv B={B} z={z} beta {beta}")
    # encode_stats, the head alone, decode: the same guards
    wsf = L.query("ardae_model_workspace_floats", m._desc, B, 1, 0)
    ws = torch.full((wsf + 4096,), NAN, device=DEV)
    mu, lv = guarded(B, z), guarded(B, z)
    L.call("ardae_vae_encode_stats", m._desc, m._flat, m._packed_weights(), xd, B, ws, wsf, mu, lv)
    check_guard(mu, B, "mu_out"), check_guard(lv, B, "lv_out")
    assert bool(torch.isnan(ws[wsf:]).all())
    assert rel(mu[:B].cpu(), out["mu"]) <= TOL_LATENT and rel(lv[:B].cpu(), out["lv"]) <= TOL_LATENT
    hid = torch.nn.functional.softplus(torch.randn(B, 800)).to(DEV).contiguous()
    for variant in (1, 2):
        o = [guarded(B, z) for _ in range(4)] + [guarded(B, 1)]
        L.call("ardae_vae_head", m._desc, m._flat, m._packed_weights(), hid, ed, B, 7, 0, None, variant, o[0], o[1], o[2], o[3], o[4])
        for buf, what in zip(o, ("mu", "lv", "z", "eps", "kld")):
            check_guard(buf, B, f"head variant {variant} {what}")
    wsf = L.query("ardae_model_workspace_floats", m._desc, B, 1, 2)
    ws = torch.full((wsf + 4096,), NAN, device=DEV)
    logit = guarded(B, D)
    L.call("ardae_model_decode", m._desc, m._flat, m._packed_weights(), zc, B, ws, wsf, logit, None)
    check_guard(logit, B, "decode out0")
    assert bool(torch.isnan(ws[wsf:]).all())
    assert rel(logit[:B].cpu(), out["logit"]) <= TOL_LATENT


# ---- 3. the head at h = 800 ----------------------------------------------------------------------------------------------------------
def head(m, hid, variant, eps=None, seed=123, offset=5):
    B, z = hid.size(0), m.z_dim
    out = {k: torch.full((B, z), NAN, device=DEV) for k in ("mu", "lv", "z", "eps")}
    out["kld"] = torch.full((B,), NAN, device=DEV)
    L.call("ardae_vae_head", m._desc, m._flat, m._packed_weights(), hid, eps, B, seed, offset, None, variant, out["mu"], out["lv"], out["z"], out["eps"],
           out["kld"])
    return out


@pytest.mark.parametrize("B,z", [(9, 32), (5, 6)])
def test_head_variants_at_h_800(B, z):
    """Variant 1 (this family's fused head: the two products on the MFMA linears, then ONE launch for the draw, the reparameterisation and the KL
    rows) against variant 2 (the five unfused launches) on 800-wide hidden rows, own draw and injected eps: both against float64 on the host, and
    eps / mu / lv / z / kld bit for bit.  The figures are printed before the last assertion.  (gauss_head_kernel, the fused head of kinds 8 / 9,
    adds one FMA chain per output where the MFMA linears split k over four waves: it agrees with the unfused launches to 2.8 - 7.6e-7 relative
    L2 here, not to the bit, and took 51.0 us against their 19.8 at 128 x 800 -> 2 x 32 - which is why this family's fused head keeps the linears.)"""
    torch.manual_seed(B)
    m = build(z, "softplus")
    # the default is what the README says it is for this family: its fused head, at every z <= 64
    assert L.query("ardae_vae_head_fused_ok", m._desc) == 1
    hid = torch.nn.functional.softplus(torch.randn(B, 800)).to(DEV).contiguous()
    draw = torch.empty(B, z, device=DEV)
    L.call("ardae_philox_normal_at", draw, draw.numel(), 123, 5, None, 0)
    given = torch.randn(B, z).to(DEV)
    p = p64_of(m)
    hd = hid.double().cpu()
    mu = hd @ p["encode.reparam.mean_fn.weight"].t() + p["encode.reparam.mean_fn.bias"]
    lv = hd @ p["encode.reparam.logvar_fn.weight"].t() + p["encode.reparam.logvar_fn.bias"]
    equal = True
    for eps, used in ((None, draw), (given, given)):
        fused, unfused = head(m, hid, 1, eps), head(m, hid, 2, eps)
        assert torch.equal(fused["eps"], used) and torch.equal(unfused["eps"], used)
        for v in (fused, unfused):      # both against float64 on the host
            assert rel(v["mu"].cpu(), mu) <= TOL_LATENT and rel(v["lv"].cpu(), lv) <= TOL_LATENT
            assert rel(v["z"].cpu(), mu + torch.exp(0.5 * lv) * used.double().cpu()) <= TOL_LATENT
            assert rel(v["kld"].cpu(), -0.5 * (1 + lv - mu ** 2 - lv.exp()).sum(1)) <= TOL_MEAN
        for k in ("mu", "lv", "z", "kld"):
            share = float((fused[k] == unfused[k]).float().mean())
            print(f"head B={B} h=800 z={z} {'own draw' if eps is None else 'injected'} {k}: rel L2 {rel(fused[k].cpu(), unfused[k].cpu()):.3g}, "
                  f"bit-identical {100 * share:.1f} %")
            equal = equal and torch.equal(fused[k], unfused[k])
        auto = head(m, hid, 0, eps)
        assert all(torch.equal(auto[k], fused[k]) for k in ("mu", "lv", "z", "eps", "kld"))
    assert equal, "variant 1 and variant 2 differ in at least one bit (figures above)"


# ---- 4. the engine -------------------------------------------------------------------------------------------------------------------
def test_engine_trajectory_against_the_reference(golden_dir):
    fx = load(golden_dir, "vae_traj_conv")
    m, B, z = from_fixture(fx)
    cfg = net.VaeConfig(lr=float(fx["cfg/lr"]), beta1=float(fx["cfg/beta1"]), beta_init=float(fx["cfg/beta_init"]), beta_fin=float(fx["cfg/beta_fin"]),
                        beta_annealing=int(fx["cfg/beta_annealing"]))
    eng = net.VaeEngine(m, cfg, batch_size=B)
    assert eng.loss_scale == 1.0 / D
    for s, _, p in trajectory(fx):
        eng.step(cuda(fx[f"{s}/x"]).view(B, 1, 28, 28), eps=cuda(fx[f"{s}/eps"]))
        st = eng.stats()
        assert st["beta"] == eng.beta_of_step(s + 1) == float(np.float32(float(fx[f"{s}/beta"]))), (s, st["beta"])
        check_losses((st["loss"], st["recon"], st["kld"]), {k: fx[f"{s}/{k}_f64"] for k in ("loss", "recon", "kld")}, f"conv step {s}")
        worst = max(rel(q.detach().cpu(), p[name]) for name, q in m.named_parameters())
        print(f"conv step {s}: worst parameter tensor against float64 {worst:.3g}")
        assert worst <= TOL_PARAM
    assert eng.step_count == 4 and eng.stats()["beta"] == 1.0


@pytest.mark.parametrize("avg", ["none", "polyak"])
def test_replay_equals_eager_and_resume_continues_to_the_same_bits(avg):
    B, z = 8, 8
    torch.manual_seed(3)
    sd0 = {k: v.clone() for k, v in build(z, "softplus").state_dict().items()}
    g = torch.Generator().manual_seed(4)
    xs = [torch.bernoulli(torch.full((B, D), 0.3), generator=g).to(DEV) for _ in range(6)]
    cfg = net.VaeConfig(lr=1e-3, beta_init=1e-4, beta_fin=1.0, beta_annealing=10, weight_avg=avg, weight_avg_start=1)

    def run(graph, steps, resume=None):
        net.manual_seed(99)
        eng = net.VaeEngine(build(z, "softplus", sd0), cfg, batch_size=B, graph=graph)
        if resume is not None:
            eng.load_state_dict(resume)
        saved = None
        for s in steps:
            eng.step(xs[s])
            if s == 3:
                saved = eng.state_dict()
        return eng, saved

    a, sd4 = run(True, range(6))
    assert a._graph is not None
    b, _ = run(False, range(6))
    assert b._graph is None
    c, _ = run(True, range(4, 6), resume=sd4)       # a fresh engine continues for 2 steps
    for other in (b, c):
        assert torch.equal(a.model._flat, other.model._flat)
        assert torch.equal(a.state, other.state) and torch.equal(a.eps, other.eps) and torch.equal(a.losses, other.losses)
        if avg != "none":
            assert torch.equal(a.avg, other.avg) and a._n_avg() == other._n_avg() == 5
    assert a.step_count == 6 and a.stats()["beta"] == float(np.float32(cfg.beta_at(5))) < 1.0


def test_one_rmsprop_step_against_the_restatement():
    B, z = 5, 8
    torch.manual_seed(12)
    m = build(z, "softplus")
    p64 = p64_of(m)
    x, eps = torch.bernoulli(torch.full((B, D), 0.3)), torch.randn(B, z)
    eng = net.VaeEngine(m, net.VaeConfig(optimizer="rmsprop", lr=1e-3, momentum=0.5, beta_fin=0.7), batch_size=B)
    eng.step(x.to(DEV), eps=eps.to(DEV))
    out, grads = loss_and_grads(p64, "softplus", x.double(), eps.double(), 0.7, 1.0 / D)
    params = [v.clone().requires_grad_(True) for v in p64.values()]
    opt = torch.optim.RMSprop(params, lr=1e-3, momentum=0.5)            # vae.py:323-324
    for v, name in zip(params, p64):
        v.grad = grads[name]
    opt.step()
    st = eng.stats()
    check_losses((st["loss"], st["recon"], st["kld"]), out, "conv rmsprop step")
    worst = max(rel(q.detach().cpu(), v.detach()) for q, v in zip(m.parameters(), params))
    print(f"conv rmsprop step: worst parameter tensor against float64 {worst:.3g}")
    assert worst <= TOL_PARAM and st["beta"] == float(np.float32(0.7))


# ---- 5. evaluate_iws -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_iwae_on_injected_draws_against_the_float64_fixture(golden_dir, case):
    fx = load(golden_dir, f"vae_conv_{case}")
    m, B, z = from_fixture(fx)
    x, eps, fwd_eps = cuda(fx["x"]), cuda(fx["lp/eps"]), cuda(fx["eps"])
    k = int(eps.size(1))
    eng = net.VaeEngine(m, net.VaeConfig(), batch_size=B)
    elbo, logprob = eng.evaluate_iws(x, k, eps=eps, fwd_eps=fwd_eps)
    print(f"conv {case}: logprob {logprob:.7f} / {float(fx['lp/value_f64']):.7f}, elbo {elbo:.6f}")
    assert relerr(logprob, fx["lp/value_f64"]) <= TOL_IWAE
    # the ELBO of the restatement (pinned to these fixture values in tests/test_vae_conv_baseline.py), and of the model's own forward
    assert relerr(elbo, -(float(fx["b1/recon_f64"]) + float(fx["b1/kld_f64"]))) <= TOL_MEAN
    _, _, _, _, recon, kld = m(x, beta=1.0, eps=fwd_eps)
    assert relerr(elbo, -(float(recon) + float(kld))) <= 1e-6
    # model.logprob is the evaluator's bound on the same draws: at B <= 16 both run the encoder on B images and the decoder on B k rows in one
    # call, so the rows are equal to the bit (the means differ by fp32 against double accumulation); both against the restatement
    rows = m.logprob_rows(x, k, eps=eps)
    assert torch.equal(rows, net.GaussianIwaeEvaluator(m, k).evaluate_rows(x, eps, fwd_eps)[2])
    assert relerr(float(m.logprob(x, sample_size=k, eps=eps)), logprob) <= 1e-6
    want = logprob_rows(fixture_params(fx, torch.float64), str(fx["act"]), x.double().cpu(), eps.double().cpu())
    assert rel(rows.cpu(), want) <= TOL_IWAE


def test_iwae_does_not_depend_on_the_chunking():
    """One chunk of 208 images against chunks of 64: the two lengths lie on either side of the row counts at which the library changes the
    kernel of the trunk's linears (conv1 leaves the small-M kernel above 83 images per call).  The evaluator calls the encoder and the ELBO
    pass's decoder on 64 images and the importance samples' decoder on 16 under either plan, so everything is equal to the bit."""
    torch.manual_seed(8)
    m = build(8, "softplus")
    N, k = 208, 16                                 # three whole groups of 64 images and a tail of 16
    x = torch.bernoulli(torch.full((N, D), 0.3)).to(DEV)
    eps, fwd_eps = torch.randn(N, k, 8).to(DEV), torch.randn(N, 8).to(DEV)
    assert m._eval_groups == (64, 16)
    probe = net.GaussianIwaeEvaluator(m, k)
    results = []
    for c, lengths in ((208, [208]), (100, [64, 64, 64, 16])):      # two budgets, two chunk lengths (whole groups under a budget of 100 images)
        ev = net.GaussianIwaeEvaluator(m, k, max_workspace_floats=probe.floats_per_chunk(c))
        assert [b - a for a, b in ev.plan(N)] == lengths
        net.manual_seed(21)
        own = tuple(t.clone() for t in ev.evaluate_rows(x))
        net.manual_seed(21)
        results.append((own, ev.evaluate(x), tuple(t.clone() for t in ev.evaluate_rows(x, eps, fwd_eps)), ev.evaluate(x, eps, fwd_eps)))
    (own0, res0, inj0, rinj0), (own1, res1, inj1, rinj1) = results
    assert all(torch.equal(a, b) for a, b in zip(own0, own1)) and res0 == res1             # own draws: rows and (elbo, logprob), to the bit
    assert all(torch.equal(a, b) for a, b in zip(inj0, inj1)) and rinj0 == rinj1           # injected draws
    assert all(bool(torch.isfinite(t).all()) for t in own0 + inj0) and not torch.equal(own0[2], inj0[2])
    # what the groups are for: the encoder on all 208 images in one call takes other kernels than on 64 (printed, not asserted: rounding)
    mu_all, mu_64 = m.encode_stats(x)[0], torch.cat([m.encode_stats(x[i:i + 64].contiguous())[0] for i in range(0, N, 64)])
    print(f"encode_stats on 208 images at once against 64 per call: bit-identical {100 * float((mu_all == mu_64).float().mean()):.1f} %")


# ---- 6. drop-in ----------------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_and_generate():
    torch.manual_seed(5)
    a = build(8, "softplus", do_xavier=True, do_m5bias=True)
    b = build(8, "softplus")
    assert not torch.equal(a.flat_params(), b.flat_params())
    b.load_state_dict({k: v.cpu() for k, v in a.state_dict().items()})
    assert torch.equal(a.flat_params(), b.flat_params())
    net.manual_seed(5)
    xs, mean, z = b.generate(7)
    assert xs.shape == mean.shape == (7, D) and z.shape == (7, 8)
    assert all(bool(torch.isfinite(t).all()) for t in (xs, mean, z))
    x = torch.bernoulli(torch.full((3, D), 0.3)).to(DEV)
    eps = torch.randn(3, 8).to(DEV)
    la, lb = a(x, eps=eps)[3], b(x.view(3, 1, 28, 28), eps=eps)[3]
    assert torch.equal(la.detach(), lb.detach())
    # the decoder's sample of forward() is the relaxed Bernoulli of its logits on the injected uniform draw
    u = torch.rand(3, D).to(DEV)
    xs, mean, zz, _, _, _ = b(x, eps=eps, dec_noise=u)
    logit = b.decode_params(zz)[0]
    assert rel(xs.cpu(), relaxed_sample(logit.double().cpu(), u.double().cpu())) <= 1e-4 and rel(mean.cpu(), torch.sigmoid(logit.double().cpu())) <= TOL_LATENT


# ---- 7. the shared decoder's backward at an activation with act'(0) != 0, on the family that owned it ---------------------------------
@pytest.mark.parametrize("act", ["tanh", "elu"])
def test_conv_implicit_model_gradients_at_tanh_and_elu(act):
    """ConvIPVAE (kind 2) runs the decoder this family shares.  ZeroPad2d after deconv1 passes no gradient; conv_decoder_bwd used to multiply the
    gradient there by act'(0), which is 0 for the relu / softplus every earlier test of kinds 2 / 4 uses and 1 for tanh / elu.  Every gradient
    tensor against a float64 restatement of models/ivae/conv.py (the trunk, fc4 on [h3 | noise], fc5, this file's decoder, N(0, I) energy)."""
    import math
    B, nz, nd, z, beta = 3, 2, 5, 8, 0.7
    torch.manual_seed(31)
    m = net.ConvIPVAE(z_dim=z, noise_dim=nd, nonlinearity=act).to(DEV)
    m.return_samples = False
    x, noise = torch.bernoulli(torch.full((B, D), 0.3)), torch.randn(B * nz, nd)
    p = {k: v.clone().requires_grad_(True) for k, v in p64_of(m).items()}
    a = ACTS[act]
    hdn = (2 * x.double() - 1).view(B, 1, 28, 28)
    for i in (1, 2, 3):
        hdn = a(torch.nn.functional.conv2d(hdn, p[f"encode.conv{i}.weight"], p[f"encode.conv{i}.bias"], stride=2, padding=2))
    t1 = a(lin(p, "encode.fc4", torch.cat([hdn.reshape(B, -1).repeat_interleave(nz, 0), noise.double()], 1)))
    zz = lin(p, "encode.fc5", t1)
    rec, _ = recon_rows(p, act, x.double().repeat_interleave(nz, 0), zz)
    want = (rec + beta * 0.5 * (zz ** 2 + math.log(2 * math.pi)).sum(1)).mean()
    g64 = dict(zip(p, torch.autograd.grad(want / D, list(p.values()))))
    _, _, zd, loss, _, _ = m(x.to(DEV), beta=beta, nz=nz, noise=noise.to(DEV))
    (loss / float(D)).backward()
    assert rel(zd.reshape(B * nz, z).cpu(), zz.detach()) <= TOL_LATENT and relerr(loss.detach(), want.detach()) <= TOL_LOSS
    check_grads64(m, [q.grad for q in m.parameters()], g64, f"ConvIPVAE {act}")
