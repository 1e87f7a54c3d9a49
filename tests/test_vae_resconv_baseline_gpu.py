"""The residual-conv Gaussian-posterior baseline on the device (ardae_model_desc.kind 12; vae.py --model resconv): forward / backward against the
reference's fixtures through the C ABI and through autograd, shapes the fixtures do not reach against the float64 restatement of
tests/test_vae_resconv_baseline.py with NaN-filled buffers and guard rows, the decoder's last stage as one kernel (ardae_resconv_tail) against that
restatement and against the unfused launches, the decode-only path, the Gaussian head at c_dim 450 / 42, the engine's trajectory, replay == eager,
resume, IWAE evaluation.

Tolerances are the project's for these quantities, imported from tests/test_vae_baseline_gpu.py: scalar losses 1e-4 relative, recon / kld means
2e-5, gradients 2e-3 relative L2 per tensor, updated parameters 5e-3 relative L2, IWAE log-probability 1e-4 against the float64 fixture, latents
(and logits) 1e-5 relative L2."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from test_ardae_uncond import rel
from test_vae_baseline import BETAS, load
from test_vae_baseline_gpu import TOL_GRAD, TOL_IWAE, TOL_LATENT, TOL_LOSS, TOL_MEAN, TOL_PARAM, check_losses, cuda, relerr  # noqa: F401
from test_vae_conv_baseline import relaxed_sample
from test_vae_conv_baseline_gpu import check_grads64, check_grads_fixture, check_guard, guarded
from test_vae_resconv_baseline import (CASES, D, decode_logit, fixture_params, logprob_rows, loss_and_grads, resconv_params, tail_logit,
                                       trajectory)

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
KNOB_ENV = {"ARDAE_DEBUG_KNOBS": "1", "ARDAE_RESCONV_TAIL_UNFUSED": "1"}


def build(z, c_dim, center=False, sd=None, **kw):
    m = net.MNISTResConvVAE(z_dim=z, c_dim=c_dim, do_center=center, **kw)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV)


def seeded(z, c_dim, center, seed):
    """a module on the oracle's initialiser: weight-norm scales spread over [0.7, 1.3], not torch's 1"""
    return build(z, c_dim, center, resconv_params(z, c_dim, seed, False))


def from_fixture(fx):
    B, z, c = (int(v) for v in fx["shape"])
    return build(z, c, bool(int(fx["do_center"])), fixture_params(fx)), B, z


def p64_of(m):
    return {k: v.detach().double().cpu() for k, v in m.named_parameters()}


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


# ---- 1. both fixtures, both betas --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_forward_backward_against_the_reference(golden_dir, case):
    fx = load(golden_dir, f"vae_resconv_{case}")
    m, B, z = from_fixture(fx)
    center, p64 = bool(int(fx["do_center"])), fixture_params(fx, torch.float64)
    x, eps, dec = cuda(fx["x"]), cuda(fx["eps"]), cuda(fx["dec_noise"])
    mu, lv = m.encode_stats(x)
    assert rel(mu.cpu(), fx["mu"]) <= TOL_LATENT and rel(lv.cpu(), fx["lv"]) <= TOL_LATENT
    zz, mu2, lv2 = m.encode(x.view(B, 1, 28, 28), eps=eps)
    assert torch.equal(mu2, mu) and torch.equal(lv2, lv) and rel(zz.cpu(), fx["b1/z"]) <= TOL_LATENT
    for b, beta in BETAS.items():
        want = {k: fx[f"{b}/{k}"] for k in ("loss", "recon", "kld")}
        _, g64 = loss_and_grads(p64, center, x.double().cpu(), eps.double().cpu(), beta, 1.0 / D)
        # the C ABI
        zc, losses, grads = abi_forward_backward(m, x, eps, beta)
        assert rel(zc.cpu(), fx[f"{b}/z"]) <= TOL_LATENT
        check_losses(losses.tolist(), want, f"resconv {case} {b} abi")
        check_grads_fixture(m, m.param_views(grads), fx, b, f"resconv {case} {b} abi")
        check_grads64(m, m.param_views(grads), g64, f"resconv {case} {b} abi")
        # grads = grads_beta * grads + ...: a second call on top of the first doubles them
        _, _, acc = abi_forward_backward(m, x, eps, beta, grads_beta=1.0, grads=grads)
        assert rel(acc.cpu(), 2 * grads.cpu()) <= 1e-6
        # the module's autograd
        for p in m.parameters():
            p.grad = None
        xs, mean, zm, loss, recon, kld = m(x, beta=beta, eps=eps, dec_noise=dec)
        (loss / float(D)).backward()
        assert torch.equal(zm, zc) and not recon.requires_grad and not kld.requires_grad
        check_losses((loss.detach(), recon, kld), want, f"resconv {case} {b} module")
        check_grads_fixture(m, [p.grad for p in m.parameters()], fx, b, f"resconv {case} {b} module")
        check_grads64(m, [p.grad for p in m.parameters()], g64, f"resconv {case} {b} module")
        assert xs.shape == mean.shape == (B, D)
        assert rel(mean.cpu(), fx[f"{b}/mean"]) <= TOL_LATENT            # the sample pass of forward(): the decode-only path
        assert rel(xs.cpu(), fx[f"{b}/x_sample"]) <= 1e-4                # the decoder's relaxed-Bernoulli sample on the injected draw


# ---- 2. shapes the fixtures do not reach, against the float64 restatement ----------------------------------------------------------
@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("B", [1, 9, 70])
def test_other_batches_against_the_float64_restatement_with_guard_rows(B, center):
    """B = 1; one row past the head's 8-row tile; past a 64-row tile.  do_center on runs the narrow model (c_dim 42, z 6: head rows off the 16-byte
    grid), off the recipe's widths.  Every buffer starts as NaN, so a read of something never written shows in the results, and nothing past B rows
    of any caller buffer (or past the workspace's declared size) may be written."""
    z, c = (6, 42) if center else (32, 450)
    torch.manual_seed(100 + B)
    m = seeded(z, c, center, 7000 + B)
    x, eps = torch.bernoulli(torch.full((B, D), 0.3)), torch.randn(B, z)
    p64 = p64_of(m)
    xd, ed = x.to(DEV), eps.to(DEV)
    beta = 0.3
    out, g64 = loss_and_grads(p64, center, x.double(), eps.double(), beta, 1.0 / D)
    zc, losses, g = abi_forward_backward(m, xd, ed, beta)
    assert rel(zc.cpu(), out["z"]) <= TOL_LATENT
    check_losses(losses.tolist(), out, f"resconv B={B} center={center}")
    check_grads64(m, m.param_views(g), g64, f"resconv B={B} center={center}")
    # encode_stats and decode: the same guards
    wsf = L.query("ardae_model_workspace_floats", m._desc, B, 1, 0)
    ws = torch.full((wsf + 4096,), NAN, device=DEV)
    mu, lv = guarded(B, z), guarded(B, z)
    L.call("ardae_vae_encode_stats", m._desc, m._flat, m._packed_weights(), xd, B, ws, wsf, mu, lv)
    check_guard(mu, B, "mu_out"), check_guard(lv, B, "lv_out")
    assert bool(torch.isnan(ws[wsf:]).all())
    assert rel(mu[:B].cpu(), out["mu"]) <= TOL_LATENT and rel(lv[:B].cpu(), out["lv"]) <= TOL_LATENT
    wsf = L.query("ardae_model_workspace_floats", m._desc, B, 1, 2)
    ws = torch.full((wsf + 4096,), NAN, device=DEV)
    logit = guarded(B, D)
    L.call("ardae_model_decode", m._desc, m._flat, m._packed_weights(), zc, B, ws, wsf, logit, None)
    check_guard(logit, B, "decode out0")
    assert bool(torch.isnan(ws[wsf:]).all())
    assert rel(logit[:B].cpu(), out["logit"]) <= TOL_LATENT


# ---- 3. the decoder's last stage in one launch ---------------------------------------------------------------------------------------
R_MAX = 67


@pytest.fixture(scope="module")
def tail_case():
    """One model (randomly initialised, non-unit scales), one y14 [67, 14, 14, 16] with values above -1 as ELU outputs are - different at every
    pixel and channel - and its float64 logits, shared by the tests below and left unchanged."""
    m = seeded(6, 42, False, 7301)
    g = torch.Generator().manual_seed(7302)
    y = torch.nn.functional.elu(1.5 * torch.randn(R_MAX, 14, 14, 16, generator=g)).contiguous()
    assert float(y.min()) > -1.0
    want = tail_logit(p64_of(m), y.double())
    return m, y.to(DEV), want


def tail(m, y, variant):
    """-> logits [R, 784] of ardae_resconv_tail on NaN-filled buffers, guard rows checked behind the logits and the workspace"""
    R = y.size(0)
    wsf = L.query("ardae_resconv_tail_workspace_floats", m._desc, R, variant)
    assert (wsf > 0) == (variant == 2)
    ws = torch.full((wsf + 4096,), NAN, device=DEV)
    out = guarded(R, D)
    L.call("ardae_resconv_tail", m._desc, m._flat, m._packed_weights(), y, R, variant, ws, wsf, out)
    check_guard(out, R, f"tail variant {variant} logits")
    assert bool(torch.isnan(ws[wsf:]).all())
    return out[:R].clone()


def border_mask():
    b = torch.zeros(28, 28, dtype=torch.bool)
    b[0, :] = b[27, :] = b[:, 0] = b[:, 27] = True
    return b.reshape(D)


@pytest.mark.parametrize("R", [1, 3, R_MAX])
def test_tail_kernel_against_float64_and_the_unfused_launches(tail_case, R):
    """Variant 1 against the float64 restatement (F.interpolate(align_corners=True), then O.res_conv of decode.dec.17) and against variant 2, over
    all pixels and over the border pixels alone: the padding taps at the four edges, and output index 27, where the source index lands on 13."""
    m, y, want = tail_case
    yr, wr = y[:R].contiguous(), want[:R]
    fused, unfused = tail(m, yr, 1), tail(m, yr, 2)
    edge = border_mask()
    for name, got in (("fused", fused), ("unfused", unfused)):
        e_all, e_edge = rel(got.cpu(), wr), rel(got.cpu()[:, edge], wr[:, edge])
        print(f"tail R={R} {name} against float64: rel L2 {e_all:.3g}, border pixels {e_edge:.3g}")
        assert e_all <= TOL_LATENT and e_edge <= TOL_LATENT
    e_all, e_edge = rel(fused.cpu(), unfused.cpu()), rel(fused.cpu()[:, edge], unfused.cpu()[:, edge])
    print(f"tail R={R} fused against unfused: rel L2 {e_all:.3g}, border pixels {e_edge:.3g}, bit-identical {100 * float((fused == unfused).float().mean()):.1f} %")
    assert e_all <= TOL_LATENT and e_edge <= TOL_LATENT
    assert torch.equal(tail(m, yr, 0), fused)                  # the library's choice is the kernel (README)


def test_tail_kernel_rows_do_not_depend_on_the_rows_of_the_call(tail_case):
    m, y, _ = tail_case
    full = tail(m, y, 1)
    for r in (0, R_MAX - 1):
        assert torch.equal(tail(m, y[r:r + 1].contiguous(), 1)[0], full[r]), r


# ---- 4. the decode-only path ---------------------------------------------------------------------------------------------------------
def test_decode_only_path_against_the_restatement(tmp_path):
    """decode_params and generate (injected z and dec_noise) against float64.  Under ARDAE_RESCONV_TAIL_UNFUSED=1 (a child process of the next
    test) the path runs the unfused launches, its workspace grows, and the logits equal the kernel's, which the parent left in a file."""
    unfused = all(os.environ.get(k) == v for k, v in KNOB_ENV.items())
    m = seeded(6, 42, False, 7401)
    R = 11
    g = torch.Generator().manual_seed(7402)
    z, u = torch.randn(R, 6, generator=g), torch.rand(R, D, generator=g)
    want = decode_logit(p64_of(m), z.double())
    assert (L.query("ardae_resconv_tail_workspace_floats", m._desc, R, 0) > 0) == unfused
    # the last stage's own buffers (u28, dec[6]'s columns) outweigh everything the kernel's path keeps
    assert (L.query("ardae_model_workspace_floats", m._desc, 2048, 1, 2) > L.query("ardae_resconv_tail_workspace_floats", m._desc, 2048, 2)) == unfused
    logit = m.decode_params(z.to(DEV))[0]
    assert logit.shape == (R, D) and rel(logit.cpu(), want) <= TOL_LATENT
    xs, mean, zz = m.generate(R, z=z.to(DEV), dec_noise=u.to(DEV))
    assert torch.equal(zz.cpu(), z) and rel(mean.cpu(), torch.sigmoid(want)) <= TOL_LATENT
    assert rel(xs.cpu(), relaxed_sample(want, u.double())) <= 1e-4
    path = os.environ.get("RESCONV_FUSED_LOGITS")
    if unfused:
        assert path, "the child process compares against the parent's logits"
        e = rel(logit.cpu(), torch.load(path))
        print(f"decode-only path, unfused launches against the kernel: rel L2 {e:.3g}")
        assert e <= TOL_LATENT
    else:
        torch.save(logit.cpu(), tmp_path / "fused.pt")


def test_decode_only_path_with_the_unfused_knob(tmp_path):
    """The library reads its debug knobs once per process, so the test above is re-run in a child process with the knob set."""
    test_decode_only_path_against_the_restatement(tmp_path)
    env = dict(os.environ, RESCONV_FUSED_LOGITS=str(tmp_path / "fused.pt"), **KNOB_ENV)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "decode_only_path_against_the_restatement"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout and "unfused launches against the kernel" in r.stdout, r.stdout[-500:]


# ---- 5. the head at c_dim 450 and 42 -------------------------------------------------------------------------------------------------
def head(m, hid, variant, eps=None, seed=123, offset=5):
    B, z = hid.size(0), m.z_dim
    out = {k: guarded(B, z) for k in ("mu", "lv", "z", "eps")}
    out["kld"] = guarded(B, 1)
    L.call("ardae_vae_head", m._desc, m._flat, m._packed_weights(), hid, eps, B, seed, offset, None, variant, out["mu"], out["lv"], out["z"], out["eps"],
           out["kld"])
    for k, v in out.items():
        check_guard(v, B, f"head variant {variant} {k}")
    return {k: (v[:B, 0] if k == "kld" else v[:B]).clone() for k, v in out.items()}


@pytest.mark.parametrize("c,z", [(450, 32), (42, 6)])
@pytest.mark.parametrize("B", [1, 70])
def test_head_variants_against_float64(B, c, z):
    """gauss_head_kernel (variant 1) and the unfused launches (variant 2) on c_dim-wide hidden rows, own draw and injected eps, against float64 on
    the host.  The default is what README says: the unfused launches (450 is no multiple of 4: the kernel reads float by float and loses)."""
    torch.manual_seed(B + c)
    m = seeded(z, c, False, 7500 + c)
    assert L.query("ardae_vae_head_fused_ok", m._desc) == 0
    hid = torch.nn.functional.elu(torch.randn(B, c)).to(DEV).contiguous()
    draw = torch.empty(B, z, device=DEV)
    L.call("ardae_philox_normal_at", draw, draw.numel(), 123, 5, None, 0)
    given = torch.randn(B, z).to(DEV)
    p = p64_of(m)
    hd = hid.double().cpu()
    mu = hd @ p["encode.reparam.mean_fn.weight"].t() + p["encode.reparam.mean_fn.bias"]
    lv = hd @ p["encode.reparam.logvar_fn.weight"].t() + p["encode.reparam.logvar_fn.bias"]
    for eps, used in ((None, draw), (given, given)):
        fused, unfused = head(m, hid, 1, eps), head(m, hid, 2, eps)
        assert torch.equal(fused["eps"], used) and torch.equal(unfused["eps"], used)
        for v in (fused, unfused):
            assert rel(v["mu"].cpu(), mu) <= TOL_LATENT and rel(v["lv"].cpu(), lv) <= TOL_LATENT
            assert rel(v["z"].cpu(), mu + torch.exp(0.5 * lv) * used.double().cpu()) <= TOL_LATENT
            assert rel(v["kld"].cpu(), -0.5 * (1 + lv - mu ** 2 - lv.exp()).sum(1)) <= TOL_MEAN
        auto = head(m, hid, 0, eps)
        assert all(torch.equal(auto[k], unfused[k]) for k in ("mu", "lv", "z", "eps", "kld"))


# ---- 6. the engine -------------------------------------------------------------------------------------------------------------------
def test_engine_trajectory_against_the_reference(golden_dir):
    fx = load(golden_dir, "vae_traj_resconv")
    m, B, z = from_fixture(fx)
    cfg = net.VaeConfig(lr=float(fx["cfg/lr"]), beta1=float(fx["cfg/beta1"]), beta_init=float(fx["cfg/beta_init"]), beta_fin=float(fx["cfg/beta_fin"]),
                        beta_annealing=int(fx["cfg/beta_annealing"]))
    eng = net.VaeEngine(m, cfg, batch_size=B)
    assert eng.loss_scale == 1.0 / D
    for s, _, p in trajectory(fx):
        eng.step(cuda(fx[f"{s}/x"]).view(B, 1, 28, 28), eps=cuda(fx[f"{s}/eps"]))
        st = eng.stats()
        assert st["beta"] == eng.beta_of_step(s + 1) == float(np.float32(float(fx[f"{s}/beta"]))), (s, st["beta"])
        check_losses((st["loss"], st["recon"], st["kld"]), {k: fx[f"{s}/{k}_f64"] for k in ("loss", "recon", "kld")}, f"resconv step {s}")
        worst = max(rel(q.detach().cpu(), p[name]) for name, q in m.named_parameters())
        print(f"resconv step {s}: worst parameter tensor against float64 {worst:.3g}")
        assert worst <= TOL_PARAM
    assert eng.step_count == 4 and eng.stats()["beta"] == 1.0


@pytest.mark.parametrize("avg", ["none", "polyak"])
def test_replay_equals_eager_and_resume_continues_to_the_same_bits(avg):
    B, z, c = 8, 8, 40
    torch.manual_seed(3)
    sd0 = {k: v.clone() for k, v in build(z, c).state_dict().items()}
    g = torch.Generator().manual_seed(4)
    xs = [torch.bernoulli(torch.full((B, D), 0.3), generator=g).to(DEV) for _ in range(6)]
    cfg = net.VaeConfig(lr=1e-3, beta1=0.9, beta_init=1e-4, beta_fin=1.0, beta_annealing=10, weight_avg=avg, weight_avg_start=1)

    def run(graph, steps, resume=None):
        net.manual_seed(99)
        eng = net.VaeEngine(build(z, c, sd=sd0), cfg, batch_size=B, graph=graph)
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
    c2, _ = run(True, range(4, 6), resume=sd4)       # a fresh engine continues for 2 steps
    for other in (b, c2):
        assert torch.equal(a.model._flat, other.model._flat)
        assert torch.equal(a.state, other.state) and torch.equal(a.eps, other.eps) and torch.equal(a.losses, other.losses)
        if avg != "none":
            assert torch.equal(a.avg, other.avg) and a._n_avg() == other._n_avg() == 5
    assert a.step_count == 6 and a.stats()["beta"] == float(np.float32(cfg.beta_at(5))) < 1.0


# ---- 7. evaluate_iws -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_iwae_on_injected_draws_against_the_float64_fixture(golden_dir, case):
    fx = load(golden_dir, f"vae_resconv_{case}")
    m, B, z = from_fixture(fx)
    x, eps, fwd_eps = cuda(fx["x"]), cuda(fx["lp/eps"]), cuda(fx["eps"])
    k = int(eps.size(1))
    eng = net.VaeEngine(m, net.VaeConfig(), batch_size=B)
    elbo, logprob = eng.evaluate_iws(x, k, eps=eps, fwd_eps=fwd_eps)
    print(f"resconv {case}: logprob {logprob:.7f} / {float(fx['lp/value_f64']):.7f}, elbo {elbo:.6f}")
    assert relerr(logprob, fx["lp/value_f64"]) <= TOL_IWAE
    assert relerr(elbo, -(float(fx["b1/recon_f64"]) + float(fx["b1/kld_f64"]))) <= TOL_MEAN
    # model.logprob is the evaluator's bound on the same draws: at B <= 8 both run the encoder on B images and the decoder on B k rows in one
    # call, so the rows are equal to the bit (the means differ by fp32 against double accumulation); both against the restatement
    rows = m.logprob_rows(x, k, eps=eps)
    assert torch.equal(rows, net.GaussianIwaeEvaluator(m, k).evaluate_rows(x, eps, fwd_eps)[2])
    assert relerr(float(m.logprob(x, sample_size=k, eps=eps)), logprob) <= 1e-6
    want = logprob_rows(fixture_params(fx, torch.float64), bool(int(fx["do_center"])), x.double().cpu(), eps.double().cpu())
    assert rel(rows.cpu(), want) <= TOL_IWAE


def test_iwae_does_not_depend_on_the_chunking():
    """One chunk of 200 images against chunks of 64 (three encoder groups and a tail of 8) at k = 4: the evaluator calls the encoder and the ELBO
    pass's decoder on 64 images and the importance samples' decoder on 8 under either plan, so everything is equal to the bit."""
    torch.manual_seed(8)
    zd = 8
    m = build(zd, 40)
    N, k = 200, 4
    x = torch.bernoulli(torch.full((N, D), 0.3)).to(DEV)
    eps, fwd_eps = torch.randn(N, k, zd).to(DEV), torch.randn(N, zd).to(DEV)
    assert m._eval_groups == (64, 8)
    probe = net.GaussianIwaeEvaluator(m, k)
    results = []
    for c, lengths in ((200, [200]), (100, [64, 64, 64, 8])):       # two budgets, two chunk lengths (whole groups under a budget of 100 images)
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
