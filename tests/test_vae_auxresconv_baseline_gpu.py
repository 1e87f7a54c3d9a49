"""The hierarchical resconv Gaussian baseline on the device (ardae_model_desc.kind 19; vae.py --model auxresconv / auxresconvct): forward / backward
against the reference's fixtures through the C ABI and through autograd on NaN-filled buffers with guard rows, other batches against the float64
restatement of tests/test_vae_auxresconv_baseline.py, the decoder's 14 x 14 stage as one kernel (ardae_resconv_mid) against that restatement and the
unfused launches, the decode-only path with and without the knob, the engine's trajectory, replay == eager, resume, and the three-stage IWAE evaluation
on fixed groups.

Tolerances are those of the sibling GPU tests, unchanged: scalar losses 1e-4 relative, recon / kld means 2e-5, gradients 2e-3 relative L2 per tensor,
updated parameters 5e-3 relative L2, IWAE log-probability 1e-4 against the float64 fixture, latents 1e-5 relative L2."""
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
from test_vae_baseline_gpu import TOL_IWAE, TOL_LATENT, TOL_MEAN, TOL_PARAM, check_losses, cuda, relerr
from test_vae_conv_baseline_gpu import check_grads64, check_grads_fixture, check_guard, guarded, p64_of
from test_vae_resconv_baseline import decode_logit
from test_vae_auxconv_baseline import summary_err
from test_vae_auxresconv_baseline import CASES, D, auxres_params, head_map, logprob_rows, loss_and_grads, mid_map, shape_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
KNOB_ENV = {"ARDAE_DEBUG_KNOBS": "1", "ARDAE_RESCONV_MID_UNFUSED": "1"}
KNOB_ON = all(os.environ.get(k) == v for k, v in KNOB_ENV.items())      # (the child process of the last decode test)


def build(nd, z, c, center, sd=None):
    m = net.MNISTResConvAuxVAE(z0_dim=nd, z_dim=z, c_dim=c, do_center=center)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV)


def from_fixture(fx):
    (B, nd, z, c), center = shape_of(fx)
    return build(nd, z, c, center, auxres_params(fx)), B, nd, z, center


def seeded(nd, z, c, center, seed):
    torch.manual_seed(seed)
    return build(nd, z, c, center)


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
    m, B, nd, z, center = from_fixture(fx)
    p64 = auxres_params(fx, torch.float64)
    x, eps, dec = cuda(fx["x"]), cuda(fx["eps"]), cuda(fx["dec_noise"])
    wsf = L.query("ardae_model_workspace_floats", m._desc, B, 1, 0)
    ws, mu0, lv0 = torch.full((wsf + 4096,), NAN, device=DEV), guarded(B, nd), guarded(B, nd)
    L.call("ardae_vae_encode_stats", m._desc, m._flat, m._packed_weights(), x, B, ws, wsf, mu0, lv0)
    check_guard(mu0, B, "mu0"), check_guard(lv0, B, "lv0")
    assert bool(torch.isnan(ws[wsf:]).all())
    assert rel(mu0[:B].cpu(), fx["mu0"]) <= TOL_LATENT and rel(lv0[:B].cpu(), fx["lv0"]) <= TOL_LATENT
    assert all(torch.equal(a, b[:B]) for a, b in zip(m.encode_stats(x.view(B, 1, 28, 28)), (mu0, lv0)))
    assert L.query("ardae_vae_head_fused_ok", m._desc) == 0       # kind 12's policy: the unfused launches
    for b, beta in BETAS.items():
        want = {k: fx[f"{b}/{k}"] for k in ("loss", "recon", "kld")}
        _, g64 = loss_and_grads(p64, center, x.double().cpu(), eps.double().cpu(), beta, 1.0 / D)
        # the C ABI
        zc, losses, grads, _ = abi_forward_backward(m, x, eps, beta)
        assert rel(zc.cpu(), fx[f"{b}/z"]) <= TOL_LATENT
        check_losses(losses.tolist(), want, f"auxresconv {case} {b} abi")
        check_grads_fixture(m, m.param_views(grads), fx, b, f"auxresconv {case} {b} abi")
        check_grads64(m, m.param_views(grads), g64, f"auxresconv {case} {b} abi")
        # grads = grads_beta * grads + ...: a second call on top of the first doubles them
        _, _, acc, _ = abi_forward_backward(m, x, eps, beta, grads_beta=1.0, grads=grads)
        assert rel(acc.cpu(), 2 * grads.cpu()) <= 1e-6
        # the module's autograd
        for p in m.parameters():
            p.grad = None
        xs, mean, zm, loss, recon, kld = m(x, beta=beta, eps=eps, dec_noise=dec)
        (loss / float(D)).backward()
        assert torch.equal(zm, zc) and not recon.requires_grad and not kld.requires_grad
        check_losses((loss.detach(), recon, kld), want, f"auxresconv {case} {b} module")
        check_grads_fixture(m, [p.grad for p in m.parameters()], fx, b, f"auxresconv {case} {b} module")
        check_grads64(m, [p.grad for p in m.parameters()], g64, f"auxresconv {case} {b} module")
        assert xs.shape == mean.shape == (B, D)
        assert rel(mean.cpu(), fx[f"{b}/mean"]) <= TOL_LATENT
        assert rel(xs.cpu(), fx[f"{b}/x_sample"]) <= 1e-4        # the decoder's relaxed-Bernoulli sample on the injected draw


# ---- 2. other batches against the live float64 restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,nd,z,c,center", [(1, 10, 6, 42, True), (9, 10, 6, 42, True), (65, 10, 6, 42, True), (9, 100, 32, 450, False)])
def test_other_batches_against_the_float64_restatement(B, nd, z, c, center):
    m = seeded(nd, z, c, center, 17 + B)
    g = torch.Generator().manual_seed(B)
    x, eps = torch.bernoulli(torch.full((B, D), 0.3), generator=g), torch.randn(B, nd + z, generator=g)
    out, g64 = loss_and_grads(p64_of(m), center, x.double(), eps.double(), 0.3, 1.0 / D)
    zc, losses, gr, _ = abi_forward_backward(m, x.to(DEV), eps.to(DEV), 0.3)
    assert rel(zc.cpu(), out["z"]) <= TOL_LATENT
    check_losses(losses.tolist(), out, f"auxresconv B={B} c_dim {c}")
    check_grads64(m, m.param_views(gr), g64, f"auxresconv B={B} c_dim {c}")


# ---- 3. the decoder's 14 x 14 stage in one launch ------------------------------------------------------------------------------------
R_MAX = 5
MID_DEFAULT = 1      # the library's choice (README: the measurement at both call shapes)


@pytest.fixture(scope="module")
def mid_case(golden_dir):
    """The recipe fixture's decoder weights, one y8 [5, 8, 8, 32] whose cropped strip (row 7, column 7) is NaN, and the float64 y14 of the same numbers,
    shared by the tests below and left unchanged"""
    fx = load(golden_dir, "vae_" + CASES[0])
    m = from_fixture(fx)[0]
    y8 = torch.randn(R_MAX, 8, 8, 32, generator=torch.Generator().manual_seed(7702))
    want = mid_map(auxres_params(fx, torch.float64), y8.double())
    y8[:, 7, :, :] = NAN
    y8[:, :, 7, :] = NAN
    return m, y8.contiguous().to(DEV), want


def mid(m, y8, variant):
    """-> y14 [R, 14, 14, 16] of ardae_resconv_mid on NaN-filled buffers, guard rows checked behind y14 and the workspace"""
    R = y8.size(0)
    wsf = L.query("ardae_resconv_mid_workspace_floats", m._desc, R, variant)
    assert (wsf > 0) == (variant == 2 or (variant == 0 and KNOB_ON))
    ws = torch.full((wsf + 4096,), NAN, device=DEV)
    out = guarded(R, 196 * 16)
    L.call("ardae_resconv_mid", m._desc, m._flat, m._packed_weights(), y8, R, variant, ws, wsf, out)
    check_guard(out, R, f"mid variant {variant} y14")
    assert bool(torch.isnan(ws[wsf:]).all())
    return out[:R].view(R, 14, 14, 16).clone()


def border(t):
    """the output positions whose source index lands on 0 or 6: index 0 and 13 in each direction"""
    return torch.cat([t[:, 0].reshape(-1), t[:, 13].reshape(-1), t[:, 1:13, 0].reshape(-1), t[:, 1:13, 13].reshape(-1)])


@pytest.mark.parametrize("R", [1, 3, R_MAX])
def test_mid_kernel_against_float64_and_the_unfused_launches(mid_case, R):
    """resconv_mid_kernel (variant 1) and the ten unfused launches (variant 2) against the float64 restatement of the stage, over all positions and over
    the border positions alone; y8's cropped strip is NaN, so any read of it shows.  Both are fp32 chains over the same 288 + 144 products per output;
    the kernel's relative L2 error may be at most twice the launches' on the same inputs (the factor covers the summation order).  The figures are
    printed; measured on one MI355X at R = 5: fused 5.76e-7, unfused 3.77e-7 over all positions (bound 7.54e-7), 5.12e-7 against 3.44e-7 on the border.
    The kernel is the library's choice (variant 0): 0.072 against 0.248 ms at 128 rows, 0.719 against 3.479 ms at the evaluator's 4096
    (profiles/vae_auxresconv_baseline_timing.json)."""
    m, y8, want = mid_case
    fused, unfused = mid(m, y8[:R].contiguous(), 1), mid(m, y8[:R].contiguous(), 2)
    for what, f in (("all positions", lambda t: t.reshape(-1)), ("border positions", border)):
        e1, e2 = rel(f(fused.cpu()), f(want[:R])), rel(f(unfused.cpu()), f(want[:R]))
        print(f"mid R={R} {what}: fused against float64 rel L2 {e1:.3g}, unfused {e2:.3g}, bound {2 * e2:.3g}; fused against unfused "
              f"{rel(f(fused.cpu()), f(unfused.cpu())):.3g}")
        assert e2 <= TOL_LATENT and e1 <= 2.0 * e2
    default = 1 if L.query("ardae_resconv_mid_workspace_floats", m._desc, R, 0) == 0 else 2
    assert default == (2 if KNOB_ON else MID_DEFAULT)
    assert torch.equal(mid(m, y8[:R].contiguous(), 0), fused if default == 1 else unfused)


def test_mid_kernel_rows_do_not_depend_on_the_rows_of_the_call(mid_case):
    m, y8, _ = mid_case
    whole = mid(m, y8, 1)
    for r in (0, 4):
        assert torch.equal(whole[r], mid(m, y8[r:r + 1].contiguous(), 1)[0])


def decode(m, z, unfused):
    """-> logits [R, 784] of ardae_model_decode and the y8 [R, 8, 8, 32] it left in its workspace (the decode-only carve opens with the two columns
    scratches, then hidden map and output of dec[0] .. dec[3], each rounded up to 64 floats)"""
    R = z.size(0)
    wsf = L.query("ardae_model_workspace_floats", m._desc, R, 1, 2)
    ws = torch.full((wsf + 4096,), NAN, device=DEV)
    out = guarded(R, D)
    L.call("ardae_model_decode", m._desc, m._flat, m._packed_weights(), z, R, ws, wsf, out, None)
    check_guard(out, R, "decode out0")
    assert bool(torch.isnan(ws[wsf:]).all())
    al = lambda n: (n + 63) // 64 * 64      # noqa: E731
    cols = al(R * 196 * 288) + al(R * 196 * 144) if unfused else 2 * al(R * 64 * 288)
    off = cols + 2 * al(R * m.c_dim) + 2 * al(R * 512) + 3 * al(R * 2048)
    return out[:R].clone(), ws[off:off + R * 2048].view(R, 8, 8, 32).clone()


def tail(m, y14):
    R = y14.size(0)
    out = guarded(R, D)
    L.call("ardae_resconv_tail", m._desc, m._flat, m._packed_weights(), y14.contiguous(), R, 1, None, 0, out)
    check_guard(out, R, "tail logits")
    return out[:R].clone()


def test_decode_only_path_and_kind_12(tmp_path):
    """ardae_model_decode of kind 19 equals dec[0 .. 3] -> ardae_resconv_mid -> ardae_resconv_tail, to the bit, and float64.  Under
    ARDAE_RESCONV_MID_UNFUSED=1 (a child process of the next test) it runs the unfused launches - it equals variant 2, its workspace grows - while
    kind 12 gives the bits the parent left in a file: the new path does not leak into it."""
    unfused = KNOB_ON
    R = 11
    m = seeded(10, 6, 42, True, 7701)
    z = torch.randn(R, 6, generator=torch.Generator().manual_seed(7702))
    logit, y8 = decode(m, z.to(DEV), unfused)
    assert bool(torch.isfinite(y8).all())
    assert rel(y8.cpu(), head_map(p64_of(m), z.double())) <= TOL_LATENT
    assert torch.equal(logit, tail(m, mid(m, y8, 2 if unfused else 1)))
    if not unfused and MID_DEFAULT == 1:
        assert torch.equal(logit, tail(m, mid(m, y8, 0)))
    assert (L.query("ardae_resconv_mid_workspace_floats", m._desc, R, 0) > 0) == (unfused or MID_DEFAULT == 2)
    assert rel(logit.cpu(), decode_logit(p64_of(m), z.double())) <= TOL_LATENT
    assert torch.equal(m.decode_params(z.to(DEV))[0], logit)
    torch.manual_seed(7700)
    m12 = net.MNISTResConvVAE(z_dim=6, c_dim=42).to(DEV)
    wsf = L.query("ardae_model_workspace_floats", m12._desc, R, 1, 2)
    ws, out = torch.full((wsf,), NAN, device=DEV), guarded(R, D)
    L.call("ardae_model_decode", m12._desc, m12._flat, m12._packed_weights(), z.to(DEV), R, ws, wsf, out, None)
    check_guard(out, R, "kind 12 decode")
    ws19 = L.query("ardae_model_workspace_floats", m._desc, 1024, 1, 2)
    path = os.environ.get("AUXRESCONV_PARENT_OUTPUTS")
    if unfused:
        assert path, "the child process compares against the parent's outputs"
        parent = torch.load(path)
        assert torch.equal(out[:R].cpu(), parent["kind12"]), "kind 12: ardae_model_decode changed under the knob"
        assert torch.equal(logit.cpu(), parent["variant2"])
        assert ws19 > parent["ws19"]
        print("decode-only path, unfused launches: kind 19 equals variant 2, its workspace grows; kind 12 unchanged")
    else:
        torch.save({"kind12": out[:R].cpu(), "variant2": tail(m, mid(m, y8, 2)).cpu(), "ws19": ws19}, tmp_path / "parent.pt")


def test_decode_only_path_with_the_unfused_knob(tmp_path):
    """The library reads its debug knobs once per process, so the test above is re-run in a child process with the knob set."""
    test_decode_only_path_and_kind_12(tmp_path)
    env = dict(os.environ, AUXRESCONV_PARENT_OUTPUTS=str(tmp_path / "parent.pt"), **KNOB_ENV)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "decode_only_path_and_kind_12"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout and "kind 12 unchanged" in r.stdout, r.stdout[-500:]


# ---- 4. the engine's trajectory, replay == eager, resume ----------------------------------------------------------------------------
def traj_config(fx, **kw):
    return net.VaeConfig(lr=float(fx["cfg/lr"]), beta1=float(fx["cfg/beta1"]), beta_init=float(fx["cfg/beta_init"]), beta_fin=float(fx["cfg/beta_fin"]),
                         beta_annealing=int(fx["cfg/beta_annealing"]), **kw)


def test_engine_trajectory_against_the_reference(golden_dir):
    fx = load(golden_dir, "vae_traj_auxresconv")
    m, B, nd, z, _ = from_fixture(fx)
    cfg = traj_config(fx)
    eng = net.VaeEngine(m, cfg, batch_size=B)
    assert eng.loss_scale == 1.0 / D and eng.eps.shape == (B, nd + z)
    for s in range(int(fx["cfg/steps"])):
        eng.step(cuda(fx[f"{s}/x"]), eps=cuda(fx[f"{s}/eps"]))
        st = eng.stats()
        assert st["beta"] == float(np.float32(cfg.beta_at(s))) == eng.beta_of_step(s + 1), (s, st["beta"])
        check_losses((st["loss"], st["recon"], st["kld"]), {k: fx[f"{s}/{k}"] for k in ("loss", "recon", "kld")}, f"auxresconv step {s}")
        worst = max(summary_err(p.detach().double().cpu(), fx[f"{s}/ps/{k}"]) for k, p in m.named_parameters())
        print(f"auxresconv step {s}: worst parameter summary {worst:.3g}")
        assert worst <= TOL_PARAM
    assert eng.step_count == 4 and eng.stats()["beta"] == 1.0


def test_replay_equals_eager_and_resume_continues_to_the_same_bits():
    """One optimiser with a weight average: the captured step replays through the beta ramp, the checkpoint carries the average"""
    nd, z, c, B = 5, 8, 40, 8
    torch.manual_seed(3)
    sd0 = {k: v.clone() for k, v in build(nd, z, c, True).state_dict().items()}
    g = torch.Generator().manual_seed(4)
    xs = [torch.bernoulli(torch.full((B, D), 0.3), generator=g).to(DEV) for _ in range(6)]
    cfg = net.VaeConfig(optimizer="adam", lr=1e-3, beta_init=1e-4, beta_fin=1.0, beta_annealing=10, weight_avg="polyak", weight_avg_start=1)

    def run(graph, steps, resume=None):
        net.manual_seed(99)
        eng = net.VaeEngine(build(nd, z, c, True, sd0), cfg, batch_size=B, graph=graph)
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
    c3, lc, _ = run(True, range(3, 6), resume=sd3)
    for other, lo in ((b, lb), (c3, lc)):
        assert torch.equal(a.model._flat, other.model._flat)
        for t, u in zip(a.opt.buffers(), other.opt.buffers()):
            assert torch.equal(t, u)
        assert all(torch.equal(x, y) for x, y in zip(la[-len(lo):], lo))
        assert torch.equal(a.state, other.state) and torch.equal(a.eps, other.eps)
        assert torch.equal(a.avg, other.avg) and a._n_avg() == other._n_avg() == 5
    want0, want1 = torch.empty(B, nd, device=DEV), torch.empty(B, z, device=DEV)
    L.call("ardae_philox_normal_at", want0, want0.numel(), 99, a.RNG_STRIDE * a.step_count, None, 0)
    L.call("ardae_philox_normal_at", want1, want1.numel(), 99, a.RNG_STRIDE * a.step_count, None, (B * nd + 3) // 4 * 4)
    assert a.step_count == 6 and torch.equal(a.eps, torch.cat([want0, want1], 1))
    assert not torch.equal(la[0], la[1])


# ---- 5. IWAE evaluation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_iwae_on_injected_draws_against_the_float64_fixture(golden_dir, case):
    fx = load(golden_dir, "vae_" + case)
    m, B, nd, z, center = from_fixture(fx)
    x, eps, fwd_eps = cuda(fx["x"]), cuda(fx["lp/eps"]), cuda(fx["eps"])
    k = int(eps.size(1))
    eng = net.VaeEngine(m, net.VaeConfig(), batch_size=B)
    elbo, logprob = eng.evaluate_iws(x, k, eps=eps, fwd_eps=fwd_eps)
    print(f"{case}: logprob {logprob:.7f} / {float(fx['lp/value_f64']):.7f}, elbo {elbo:.6f}")
    assert relerr(logprob, fx["lp/value_f64"]) <= TOL_IWAE
    assert relerr(float(m.logprob(x, sample_size=k, eps=eps)), fx["lp/value_f64"]) <= TOL_IWAE
    # elbo = -(recon + kld + aux_kld) of a forward on the same draw
    assert relerr(elbo, -(float(fx["b1/recon_f64"]) + float(fx["b1/kld_f64"]))) <= TOL_MEAN
    # row by row against the restatement
    rows = m.logprob_rows(x, k, eps=eps)
    want = logprob_rows(auxres_params(fx, torch.float64), center, torch.tensor(fx["x"]).double(), torch.tensor(fx["lp/eps"]).double())
    assert rel(rows.cpu(), want) <= TOL_IWAE


def test_iwae_own_draws_do_not_depend_on_the_chunking():
    """200 images at k = 4: one chunk against chunks of 64.  Every call runs on fixed groups (64 images for the statistics and the ELBO pass, 16 for the
    stages and the decoder), so elbo and logprob are equal to the bit."""
    N, k, nd, zd = 200, 4, 10, 6
    m = seeded(nd, zd, 42, True, 8)
    x = torch.bernoulli(torch.full((N, D), 0.3)).to(DEV)
    probe = net.GaussianIwaeEvaluator(m, k)
    assert probe.plan(N) == [(0, N)]
    results = []
    for budget, chunks in ((None, [(0, 200)]), (probe.floats_per_chunk(100), [(0, 64), (64, 128), (128, 192), (192, 200)])):
        ev = probe if budget is None else net.GaussianIwaeEvaluator(m, k, max_workspace_floats=budget)
        assert ev.plan(N) == chunks
        net.manual_seed(21)
        recon, kld, rows = ev.evaluate_rows(x)
        net.manual_seed(21)
        results.append(((recon.clone(), kld.clone(), rows.clone()), ev.evaluate(x)))
    assert all(torch.equal(a, b) for a, b in zip(results[1][0], results[0][0]))
    assert results[1][1] == results[0][1]                          # (elbo, logprob), to the bit
    assert all(bool(torch.isfinite(t).all()) for t in results[0][0])
