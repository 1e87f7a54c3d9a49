"""Unconditional AR-DAE score networks on the device: C ABI kinds 2 / 3, the fused front end, the modules and ArdaeScoreEngine.

Bars: loss 2e-5 relative, every gradient tensor and glogprob 1e-4 relative L2 against the reference's fp32 fixtures - the bars
tests/test_cdae_gpu.py states for the conditional kinds.  The float64 oracle is the restatement in tests/score_restate.py, which
tests/test_ardae_uncond.py pins to the reference's fp64 fixtures to 1e-12."""
import os

import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from oracle import ardae_oracle as O
from score_gpu_checks import (Harness, check_abi_against_fixture, check_module_forward_backward, check_refusals, check_replay_equals_eager, check_resume,
                              flat_of, fresh_module, fused, init_params, split_flat, unfused)
from score_restate import ARDAE, DAE, LOSS_TOL, TENSOR_TOL, cast, grads_on_xbar, load, rel, state_dict_of
from test_cdae_gpu import CdaeHarness, oracle64_grads

pytestmark = pytest.mark.gpu
FIXTURE_IDS = [f"{k}_{c}" for k in ("grad", "res") for c in ("n60_d3_elu", "n64_d2_relu1", "n64_d2_softplus", "n64_d2_swish", "n96_d8_tanh")]


# ---- 5. C ABI against every fixture ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FIXTURE_IDS)
def test_abi_matches_the_reference_fixtures(golden_dir, fid):
    check_abi_against_fixture(ARDAE, golden_dir, fid)


# ---- 6. against float64 at sizes a user runs, with the conditional sibling as the yardstick ---------------------------------------
USER_SHAPES = [(10240, 2, 256, 3, "softplus"), (2560, 2, 128, 3, "softplus"), (4096, 32, 256, 3, "softplus"), (300, 3, 100, 2, "elu"),
               (1000, 1, 64, 4, "tanh")]


def sibling_error(kind, N, d, h, nl, act, xbar, sigma, eps):
    """E_cond: the conditional network of the same widths (B = N / 4, S = 4, context_dim = d) through ardae_cdae_loss_grads against
    float64, worst relative L2 over the tensors whose gradient sums over the N rows (input encoder and score network)."""
    cc = O.CdaeCfg(kind, d, d, h, nl, act)
    pc = O.init_params(O.cdae_param_spec(cc), 11)
    ctx = torch.randn(N // 4, d, generator=torch.Generator().manual_seed(5))
    _, g64, _ = oracle64_grads(cc, pc, xbar, sigma, eps, ctx, 4)
    _, grads, _ = CdaeHarness(cc, torch.cat([pc[n].reshape(-1).float() for n, _ in O.cdae_param_spec(cc)])).loss_grads(xbar, sigma, eps, ctx, N // 4, 4)
    g = split_flat(grads, O.cdae_param_spec(cc))
    return max(rel(g[n], g64[n]) for n in g if not n.startswith("ctx_encode.") and g64[n] is not None)


@pytest.mark.parametrize("kind", ["grad", "res"])
@pytest.mark.parametrize("N,d,h,nl,act", USER_SHAPES, ids=[f"n{s[0]}_d{s[1]}_h{s[2]}" for s in USER_SHAPES])
def test_gradients_against_float64_at_user_sizes(kind, N, d, h, nl, act):
    """e <= max(2 E_cond, 3 e_ref32 + 2e-6) per gradient tensor (e_ref32: the fp32 restatement's own distance to float64)."""
    g = torch.Generator().manual_seed(N + d)
    x, sigma, eps = torch.randn(N, d, generator=g), 0.1 * torch.randn(N, 1, generator=g), torch.randn(N, d, generator=g)
    spec = ARDAE.spec_of(kind, d, h, nl)
    p = init_params(spec, 3)
    xbar = torch.addcmul(x, sigma, eps)

    def oracle(dtype):                          # the restatement's loss on the SAME fp32 xbar: mse(sigma g(xbar, sigma), -eps)
        pp, xb, sg, ep = cast(dtype, p, xbar, sigma, eps)
        return grads_on_xbar(kind, pp, act, xb, sg, ep, True)
    loss64, g64 = oracle(torch.float64)
    loss32, g32 = oracle(torch.float32)
    loss, grads, _ = Harness(ARDAE, kind, d, h, nl, act, flat_of(p, spec)).loss_grads(xbar, sigma, eps)
    try:
        E_cond, sib = sibling_error(kind, N, d, h, nl, act, xbar, sigma.reshape(-1), eps), f"d={d}"
    except ValueError as exc:                   # the sibling refuses the shape: the nearest one it accepts (d + 1), on draws of its own
        d2 = d + 1
        xb2, ep2 = torch.randn(N, d2, generator=g), torch.randn(N, d2, generator=g)
        E_cond, sib = sibling_error(kind, N, d2, h, nl, act, xb2, sigma.reshape(-1), ep2), f"d={d2} (d={d} refused: {exc})"
    assert abs(float(loss) - float(loss64)) <= LOSS_TOL * abs(float(loss64))
    bad = []
    for n in g64:
        if g64[n] is None:
            assert torch.isnan(grads[n]).all()
            continue
        e, e32 = rel(grads[n], g64[n]), rel(g32[n], g64[n])
        bar = max(2 * E_cond, 3 * e32 + 2e-6)
        print(f"{kind} N={N} d={d} h={h} L={nl} {act} {n}: e={e:.2e} E_cond={E_cond:.2e} [{sib}] e_ref32={e32:.2e} bar={bar:.2e}")
        if e > bar:
            bad.append((n, e, bar))
    assert not bad, bad


# ---- 7. fused front end -----------------------------------------------------------------------------------------------------------
FUSED_SHAPES = [(1024, 10, 2, 256, 3, "softplus"), (256, 10, 2, 128, 3, "softplus"), (30, 10, 2, 64, 3, "relu"), (50, 20, 1, 64, 4, "tanh"),
                (64, 4, 8, 128, 2, "elu"), (25, 12, 3, 256, 2, "swish")]


@pytest.mark.parametrize("kind", ["grad", "res"])
@pytest.mark.parametrize("B,ns,d,h,nl,act", FUSED_SHAPES, ids=[f"b{s[0]}x{s[1]}_d{s[2]}_h{s[3]}_{s[5]}" for s in FUSED_SHAPES])
def test_fused_front_end_equals_the_three_launches(kind, B, ns, d, h, nl, act):
    spec = ARDAE.spec_of(kind, d, h, nl)
    hn = Harness(ARDAE, kind, d, h, nl, act, flat_of(init_params(spec, 9), spec))
    assert L.query("ardae_dae_perturb_fused_ok", hn.d, ns) == 1
    x = torch.randn(B, d, generator=torch.Generator().manual_seed(B)).cuda()
    delta, seed = 0.7, 1234
    state = torch.zeros(4, dtype=torch.int64, device="cuda")
    L.call("ardae_step_state_advance", state, 16 * 5, 1e-3, 0.5, 0.999)
    for st in (None, state):
        lf, gf, xb_f, sg_f, ep_f, h1_f = fused(hn, x, B, ns, delta, seed, 0, st)
        lu, gu, xb_u, sg_u, ep_u, h1_u = unfused(hn, x, B, ns, delta, seed, 0, st)
        assert torch.equal(xb_f, xb_u) and torch.equal(sg_f, sg_u) and torch.equal(ep_f, ep_u)
        same = float((h1_f == h1_u).float().mean())
        print(f"{kind} B={B} ns={ns} d={d} h={h} {act}: h_1 bit-identical on {100 * same:.3f} % of its elements, relL2 {rel(h1_f.cpu(), h1_u.cpu()):.2e}")
        assert rel(h1_f.cpu(), h1_u.cpu()) <= 1e-6
        assert abs(float(lf) - float(lu)) <= LOSS_TOL * abs(float(lu))
        for n in gu:
            if torch.isnan(gu[n]).all():
                assert torch.isnan(gf[n]).all()
            else:
                assert rel(gf[n], gu[n]) <= TENSOR_TOL, n
    assert not torch.equal(sg_f, fused(hn, x, B, ns, delta, seed)[3])              # the state's base offset moved the draws
    # rows 4 k ... of the larger draw: the samples from b0 on, first_row = b0 ns (a multiple of 4)
    b0 = next(b for b in range(1, B) if (b * ns) % 4 == 0)
    _, _, xb_all, sg_all, ep_all, _ = fused(hn, x, B, ns, delta, seed)
    _, _, xb_t, sg_t, ep_t, _ = fused(hn, x[b0:].contiguous(), B - b0, ns, delta, seed, b0 * ns)
    assert torch.equal(xb_t, xb_all[b0 * ns:]) and torch.equal(sg_t, sg_all[b0 * ns:]) and torch.equal(ep_t, ep_all[b0 * ns:])


def test_perturb_is_one_fma_on_the_broadcast_batch():
    B, ns, d = 37, 7, 3
    g = torch.Generator().manual_seed(0)
    x, sigma, eps = torch.randn(B, d, generator=g).cuda(), torch.randn(B * ns, generator=g).cuda(), torch.randn(B * ns, d, generator=g).cuda()
    xbar = torch.empty(B * ns, d, device="cuda")
    L.call("ardae_dae_perturb", x, sigma, eps, B, ns, d, xbar)
    rows = x.unsqueeze(1).expand(B, ns, d).reshape(B * ns, d)
    want = (rows.double() + sigma.double()[:, None] * eps.double()).float()       # a single rounding
    assert torch.equal(xbar, want)


# ---- 8. modules -------------------------------------------------------------------------------------------------------------------
def module_of(fx, device="cuda"):
    m = ARDAE.module(str(fx["kind"]), *(int(v) for v in fx["shape"][1:]), str(fx["act"]))
    m.load_state_dict(state_dict_of(fx))
    return m.to(device)


@pytest.mark.parametrize("fid", FIXTURE_IDS)
def test_module_forward_backward(golden_dir, fid):
    check_module_forward_backward(ARDAE, golden_dir, fid)


@pytest.mark.parametrize("opt_name", ["torch_rmsprop", "net_rmsprop", "torch_sgd"])
@pytest.mark.parametrize("fid", ["grad_n64_d2_softplus", "res_n96_d8_tanh", "grad_n60_d3_elu", "res_n64_d2_relu1"])
def test_training_cell_follows_the_recorded_trajectory(golden_dir, fid, opt_name):
    """The training cell of notebooks/ardae_toy.ipynb, teacher-forced: parameters reset to the fixture's before each step."""
    fx = ARDAE.fixture(golden_dir, fid)
    traj = "traj_sgd" if opt_name == "torch_sgd" else "traj_rmsprop"
    m = module_of(fx)
    lr = float(fx[traj + "/lr"])
    opt = {"torch_rmsprop": lambda: torch.optim.RMSprop(m.parameters(), lr=lr, momentum=0.5), "net_rmsprop": lambda: net.RMSprop(m.parameters(), lr=lr, momentum=0.5),
           "torch_sgd": lambda: torch.optim.SGD(m.parameters(), lr=lr)}[opt_name]()
    for s in range(6):
        pre = f"{traj}/{s}/"
        x, std, eps = (torch.tensor(fx[pre + k]).cuda() for k in ("x", "std", "eps"))
        opt.zero_grad()
        _, loss = m(x, std, eps=eps)
        loss.backward()
        opt.step()
        assert abs(float(loss.detach()) - float(fx[pre + "loss"])) <= LOSS_TOL * abs(float(fx[pre + "loss"])), (s, float(loss.detach()))
        with torch.no_grad():
            for n, p in m.named_parameters():
                want = torch.tensor(fx[pre + "p/" + n])
                assert rel(p.cpu(), want) <= TENSOR_TOL, (s, n, rel(p.cpu(), want))
                p.copy_(want)                                # teacher forcing
        m.mark_dirty()


# ---- 9. engine --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optimizer", ["rmsprop", "adam", "sgd", "amsgrad"])
@pytest.mark.parametrize("kind,B,ns,d,h,nl,act", [("grad", 256, 10, 2, 128, 3, "softplus"), ("res", 64, 10, 2, 64, 3, "softplus"), ("grad", 30, 10, 3, 100, 2, "elu")])
def test_engine_replay_equals_eager(kind, B, ns, d, h, nl, act, optimizer):
    cfg = net.ScoreConfig(delta=1.0, nsigma=ns, lr=1e-3, optimizer=optimizer)
    data = [(torch.randn(B, d, generator=torch.Generator().manual_seed(s)).cuda(),) for s in range(8)]
    check_replay_equals_eager(ARDAE, lambda: fresh_module(ARDAE, kind, d, h, nl, act), cfg, B, (), data, {})


@pytest.mark.parametrize("kind", ["grad", "res"])
def test_engine_with_injected_noise_equals_the_module_path(kind):
    B, ns, d, h, nl, act = 64, 10, 2, 128, 3, "softplus"
    g = torch.Generator().manual_seed(3)
    x, sigma, eps = torch.randn(B, d, generator=g).cuda(), torch.randn(B * ns, generator=g).cuda(), torch.randn(B * ns, d, generator=g).cuda()
    m = fresh_module(ARDAE, kind, d, h, nl, act)
    rows = x.unsqueeze(1).expand(B, ns, d).contiguous().view(B * ns, d)       # the notebooks' broadcast
    _, loss = m(rows, sigma[:, None], eps=eps)
    loss.backward()
    eng = net.ArdaeScoreEngine(fresh_module(ARDAE, kind, d, h, nl, act), net.ScoreConfig(nsigma=ns, optimizer="sgd", lr=1e-2), B)
    before = eng.dae.flat_params().clone()
    eng.step(x, noise={"sigma": sigma, "eps": eps})
    st = eng.stats()
    assert abs(st["loss"] - float(loss.detach())) <= LOSS_TOL * abs(float(loss.detach()))
    assert abs(st["sigma_abs_mean"] - float(sigma.abs().mean())) <= 1e-6
    grads = split_flat(eng.grads.cpu(), ARDAE.spec_of(kind, d, h, nl))
    for n, p in m.named_parameters():
        if p.grad is not None:
            assert rel(grads[n], p.grad.cpu()) <= TENSOR_TOL, n
    n_grad = eng.n_grad
    # the SGD step was applied: p - lr g, rounded to fp32 once or twice (2 ulps of the larger operand, elementwise)
    want = before.double() - 1e-2 * eng.grads.double()
    slack = 2.0 ** -22 * (before.abs().double() + 1e-2 * eng.grads.abs().double())
    assert ((eng.dae.flat_params().double() - want).abs() <= slack)[:n_grad].all()
    assert not torch.equal(before[:n_grad], eng.dae.flat_params()[:n_grad])
    assert torch.equal(before[n_grad:], eng.dae.flat_params()[n_grad:])
    # score() == glogprob, with the updated weights
    pts = torch.randn(500, d, generator=g).cuda()
    lv = torch.rand(500, generator=g).cuda()
    assert torch.equal(eng.score(pts, lv), eng.dae.glogprob(pts, lv[:, None]))
    assert torch.equal(eng.score(pts), eng.dae.glogprob(pts))


def test_engine_refuses_bad_batches():
    fresh = lambda: fresh_module(ARDAE, "grad", 2, 64, 3, "softplus")
    good = torch.zeros(32, 2, device="cuda")
    eng = check_refusals(ARDAE, fresh, lambda: fresh_module(DAE, "grad", 2, 64, 3, "softplus"), 32, (), (good,), good[:31])
    with pytest.raises(ValueError, match="batch_size=32"):
        eng.step(torch.zeros(32, 3, device="cuda"))
    with pytest.raises(ValueError, match="contiguous"):
        eng.step(torch.zeros(32, 4, device="cuda")[:, ::2])
    with pytest.raises(ValueError, match="expected a tensor on cuda"):
        eng.step(torch.zeros(32, 2))
    with pytest.raises(ValueError, match="float32"):
        eng.step(good.double())
    assert eng.step_count == 0
    with pytest.raises(TypeError):
        net.ArdaeScoreEngine(net.MLPGradCARDAE(input_dim=2, context_dim=2, h_dim=16, nonlinearity="softplus").cuda(), net.ScoreConfig(), 32)
    with pytest.raises(NotImplementedError):
        net.ArdaeScoreEngine(fresh(), net.ScoreConfig(optimizer="lbfgs"), 32)


def test_engine_refuses_noise_on_another_device():
    """Injected noise is validated like a batch: a tensor on the host or on another GPU is refused before anything is launched."""
    B, ns, d = 30, 4, 3
    eng = net.ArdaeScoreEngine(fresh_module(ARDAE, "grad", d, 64, 2, "elu"), net.ScoreConfig(nsigma=ns), B)
    before = [eng.dae.flat_params().clone(), eng.state.clone(), eng.sigma.clone()] + [b.clone() for b in eng.opt.buffers()]
    x, eps = torch.zeros(B, d, device="cuda:0"), torch.zeros(B * ns, d, device="cuda:0")
    for other in ["cpu"] + (["cuda:1"] if torch.cuda.device_count() > 1 else []):
        with pytest.raises(ValueError, match="sigma must be"):
            eng.step(x, noise={"sigma": torch.zeros(B * ns, device=other), "eps": eps})
        with pytest.raises(ValueError, match="eps must be"):
            eng.step(x, noise={"sigma": torch.zeros(B * ns, device="cuda:0"), "eps": eps.to(other)})
    after = [eng.dae.flat_params(), eng.state, eng.sigma] + eng.opt.buffers()
    assert eng.step_count == 0 and all(torch.equal(a, b) for a, b in zip(before, after)), "a refused call reached the device"


@pytest.mark.parametrize("kind,optimizer", [("grad", "rmsprop"), ("grad", "amsgrad"), ("res", "adam")])
def test_score_engine_resumes_bit_identically(kind, optimizer):
    """state_dict() after step 4 into a fresh engine under another library seed: steps 5 - 8 (eager, eager, captured, replayed there) leave
    what the uninterrupted run leaves.  B 30 x 4 levels, d 3, h 64: the trailing bias without gradient (grad), three optimiser buffers
    (amsgrad), a partial 64-row tile and the fused front end."""
    B, ns, d, h, nl, act = 30, 4, 3, 64, 2, "elu"
    cfg = net.ScoreConfig(delta=1.0, nsigma=ns, lr=1e-3, optimizer=optimizer)
    data = [(torch.randn(B, d, generator=torch.Generator().manual_seed(s)).cuda(),) for s in range(8)]
    check_resume(ARDAE, lambda seed: fresh_module(ARDAE, kind, d, h, nl, act, seed=seed), cfg, None, B, (), data, 4, dict(fused_front=True))


# ---- 10. quality: device seeds against the reference's seeds ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["grad", "res"])
def test_training_quality_against_the_reference_seeds(golden_dir, kind):
    """The training cell of notebooks/ardae_toy.ipynb on x ~ N(0, I_2) with the notebook's optimiser (torch.optim.Adam over the module's
    parameters); every constant comes from the fixture tools/gen_score_golden.py (family ardae) wrote with the reference classes."""
    q = load(os.path.join(golden_dir, "ardae_uncond_quality.npz"))
    B, ns, steps, tail, delta, lr = int(q["B"]), int(q["nsigma"]), int(q["steps"]), int(q["tail"]), float(q["delta"]), float(q["lr"])
    xt = torch.tensor(q["x_t"]).cuda()
    ref_loss, ref_err = q[f"{kind}/loss"], q[f"{kind}/score_err"]
    dev_loss, dev_err = [], []
    for seed in (int(s) for s in q["seeds"]):
        torch.manual_seed(2000 + seed)
        net.manual_seed(2000 + seed)
        m = ARDAE.module(kind, 2, int(q["h"]), int(q["L"]), str(q["act"])).cuda()
        opt = torch.optim.Adam(m.parameters(), lr=lr)
        hist = []
        for _ in range(steps):
            opt.zero_grad()
            x = torch.randn(B, 2, device="cuda")
            sigma = delta * torch.randn(B * ns, 1, device="cuda")
            x = x.unsqueeze(1).expand(B, ns, 2).contiguous().view(B * ns, 2)
            _, loss = m(x, sigma)
            loss.backward()
            opt.step()
            hist.append(loss.detach())
        dev_loss.append(float(torch.stack(hist[-tail:]).mean()))
        row = []
        for s in q["levels"]:
            exact = -xt / (1.0 + float(s) ** 2)
            row.append(float((m.glogprob(xt, torch.full((xt.size(0), 1), float(s), device="cuda")) - exact).norm() / exact.norm()))
        dev_err.append(row)
    dev_loss, dev_err = np.array(dev_loss), np.array(dev_err)
    n = len(dev_loss)
    gap, bar = abs(dev_loss.mean() - ref_loss.mean()), 3 * np.sqrt(ref_loss.var(ddof=1) / len(ref_loss) + dev_loss.var(ddof=1) / n)
    print(f"{kind}: loss device {dev_loss.mean():.4f} +- {dev_loss.std(ddof=1):.4f}, reference {ref_loss.mean():.4f} +- {ref_loss.std(ddof=1):.4f}; gap {gap:.4f} <= {bar:.4f}")
    print(f"{kind}: score error device mean {dev_err.mean(0)}, reference mean {ref_err.mean(0)}, reference per-seed max {ref_err.max(0)}")
    assert gap <= bar
    assert (dev_err.mean(0) <= ref_err.max(0)).all()
