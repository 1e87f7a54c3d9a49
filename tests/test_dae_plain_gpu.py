"""Plain DAE score networks on the device: C ABI kinds 6 / 7, the perturbation, the sigma schedule, the modules and ArdaeScoreEngine
with a DaeConfig (notebooks/dae_toy.ipynb).

Bars: loss 2e-5 relative, every gradient tensor and glogprob 1e-4 relative L2 against the reference's fp32 fixtures - the bars
tests/test_cdae_gpu.py and tests/test_ardae_uncond_gpu.py state.  The float64 oracle is the restatement in tests/score_restate.py, which
tests/test_dae_plain.py pins to the reference's fp64 fixtures to 1e-12."""
import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from score_gpu_checks import (STRIDE, Harness, check_abi_against_fixture, check_drop_in_route, check_module_forward_backward, check_recorded_trajectory,
                              check_refusals, check_replay_equals_eager, check_resume, check_zero_sigma_column, dae_block, flat_of, fresh_module, front,
                              guarded, init_params)
from score_restate import ARDAE, DAE, LOSS_TOL, cast, grads_on_xbar, rel

pytestmark = pytest.mark.gpu
FIXTURE_IDS = [f"{k}_{c}" for k in ("grad", "res") for c in ("n60_d3_elu", "n64_d2_relu1", "n64_d2_softplus", "n64_d2_swish", "n96_d8_tanh")]


# ---- 1. C ABI against every fixture ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FIXTURE_IDS)
def test_abi_matches_the_reference_fixtures(golden_dir, fid):
    check_abi_against_fixture(DAE, golden_dir, fid)


# ---- 2. the AR-DAE kinds with a zero sigma column are the same function: existing code as the oracle -------------------------------
ORACLE_SHAPES = [(60, 3, 100, 2, "elu"), (64, 2, 64, 3, "softplus"), (300, 8, 256, 3, "softplus"), (1000, 1, 64, 4, "tanh")]


@pytest.mark.parametrize("kind", ["grad", "res"])
@pytest.mark.parametrize("N,d,h,nl,act", ORACLE_SHAPES, ids=[f"n{s[0]}_d{s[1]}_h{s[2]}" for s in ORACLE_SHAPES])
def test_plain_kinds_equal_the_ardae_kinds_with_a_zero_sigma_column(kind, N, d, h, nl, act):
    check_zero_sigma_column(DAE, kind, N, 1, d, 0, h, nl, act)


# ---- 3. against float64 at sizes a user runs, with the AR-DAE sibling as the yardstick ---------------------------------------------
USER_SHAPES = [(2560, 2, 128, 3, "softplus"), (300, 3, 100, 2, "elu"), (1000, 1, 64, 4, "tanh")]


def sibling_error(kind, d, h, nl, act, xbar, sigma, eps):
    """E_sibling: the AR-DAE network of the same widths (kind 2 / 3) through ardae_cdae_loss_grads against float64, worst relative L2
    over its gradient tensors."""
    spec = ARDAE.spec_of(kind, d, h, nl)
    p = init_params(spec, 11)
    pp, xb, sg, ep = cast(torch.float64, p, xbar, sigma, eps)
    _, g64 = grads_on_xbar(kind, pp, act, xb, sg, ep, True)
    _, grads, _ = Harness(ARDAE, kind, d, h, nl, act, flat_of(p, spec)).loss_grads(xbar, sigma, eps)
    return max(rel(grads[n], g64[n]) for n in grads if g64[n] is not None)


@pytest.mark.parametrize("kind", ["grad", "res"])
@pytest.mark.parametrize("N,d,h,nl,act", USER_SHAPES, ids=[f"n{s[0]}_d{s[1]}_h{s[2]}" for s in USER_SHAPES])
def test_gradients_against_float64_at_user_sizes(kind, N, d, h, nl, act):
    """e <= max(2 E_sibling, 3 e_ref32 + 2e-6) per gradient tensor (e_ref32: the fp32 restatement's own distance to float64)."""
    g = torch.Generator().manual_seed(N + d)
    x, sigma, eps = torch.randn(N, d, generator=g), 0.1 * torch.randn(N, 1, generator=g), torch.randn(N, d, generator=g)
    spec = DAE.spec_of(kind, d, h, nl)
    p = init_params(spec, 3)
    xbar = torch.addcmul(x, sigma, eps)

    def oracle(dtype):                          # the restatement's loss on the SAME fp32 xbar: mse(sigma g(xbar), -eps)
        pp, xb, sg, ep = cast(dtype, p, xbar, sigma, eps)
        return grads_on_xbar(kind, pp, act, xb, sg, ep, False)
    loss64, g64 = oracle(torch.float64)
    loss32, g32 = oracle(torch.float32)
    loss, grads, _ = Harness(DAE, kind, d, h, nl, act, flat_of(p, spec)).loss_grads(xbar, sigma, eps)
    E_sib = sibling_error(kind, d, h, nl, act, xbar, sigma, eps)
    assert abs(float(loss) - float(loss64)) <= LOSS_TOL * abs(float(loss64))
    bad = []
    for n in g64:
        if g64[n] is None:
            assert torch.isnan(grads[n]).all()
            continue
        e, e32 = rel(grads[n], g64[n]), rel(g32[n], g64[n])
        bar = max(2 * E_sib, 3 * e32 + 2e-6)
        print(f"{kind} N={N} d={d} h={h} L={nl} {act} {n}: e={e:.2e} E_sibling={E_sib:.2e} e_ref32={e32:.2e} bar={bar:.2e}")
        if e > bar:
            bad.append((n, e, bar))
    assert not bad, bad


# ---- 4. the front end: draw, perturbation, loss and gradients as the engine launches them --------------------------------------------
FRONT_SHAPES = [(1, 1, 1, 64, 2, "tanh"), (16, 4, 2, 128, 3, "softplus"), (30, 10, 3, 256, 2, "elu"), (25, 12, 8, 64, 3, "swish"),
                (256, 10, 2, 128, 3, "softplus")]


@pytest.mark.parametrize("kind", ["grad", "res"])
@pytest.mark.parametrize("B,ns,d,h,nl,act", FRONT_SHAPES, ids=[f"b{s[0]}x{s[1]}_d{s[2]}_h{s[3]}_{s[5]}" for s in FRONT_SHAPES])
def test_front_end_is_the_same_for_a_value_and_for_the_device_block(kind, B, ns, d, h, nl, act):
    """(A fused draw + perturbation + first-layer kernel was built, measured and deleted - DESIGN.md section 6; what remains to pin is that
    the two sources of sigma and the step state's base offset give what they should.)"""
    spec = DAE.spec_of(kind, d, h, nl)
    hn = Harness(DAE, kind, d, h, nl, act, flat_of(init_params(spec, 9), spec))
    x = torch.randn(B, d, generator=torch.Generator().manual_seed(B)).cuda()
    seed, N = 1234, B * ns
    block = dae_block(3, 1.0, 0.1, 4)                        # sigma of i = 2, Philox base offset 3 * STRIDE
    s = float(np.float32(net.dae_sigma(1.0, 0.1, 4, 2)))
    outs = {}
    for form, sig, dst in (("value", s, None), ("block", 0.0, block)):
        for st in (None, block):
            loss, grads, xbar, sg, eps, h1 = front(hn, x, B, ns, sig, dst, seed, 0, st)
            assert torch.equal(sg, torch.full((N,), s, device="cuda"))
            rows = x.unsqueeze(1).expand(B, ns, d).reshape(N, d)
            assert torch.equal(xbar, (rows.double() + s * eps.double()).float())
            assert torch.isfinite(loss).all() and all(torch.isfinite(g).all() or n == "neglogprob.fc.bias" for n, g in grads.items())
            outs[form, st is not None] = (loss, xbar, eps, h1)
    for with_state in (False, True):                          # the two forms of sigma: the same bits
        assert all(torch.equal(u, v) for u, v in zip(outs["value", with_state], outs["block", with_state]))
    assert not torch.equal(outs["value", False][2], outs["value", True][2])          # the state's base offset moved the draw
    ref = torch.empty(N, d, device="cuda")
    L.call("ardae_philox_normal_at", ref, N * d, seed, 4 + 3 * STRIDE, None, 0)
    assert torch.equal(outs["value", True][2], ref)


# ---- 5. the unfused perturbation ---------------------------------------------------------------------------------------------------
def test_noise_perturb_is_one_fma_on_the_broadcast_batch():
    B, ns, d = 37, 7, 3
    g = torch.Generator().manual_seed(0)
    x, eps = torch.randn(B, d, generator=g).cuda(), torch.randn(B * ns, d, generator=g).cuda()
    rows = x.unsqueeze(1).expand(B, ns, d).reshape(B * ns, d)
    block = dae_block(2, 5.0, 0.05, 4000)
    for s, sig, dst in ((0.3, 0.3, None), (net.dae_sigma(5.0, 0.05, 4000, 1), 123.0, block)):      # with a block the argument is not read
        s32 = float(np.float32(s))
        (xb_all, xbar), (sg_all, sg) = guarded(B * ns, d), guarded(B * ns)
        L.call("ardae_dae_noise_perturb", x, eps, B, ns, d, sig, dst, xbar, sg)
        want = (rows.double() + s32 * eps.double()).float()       # a single rounding
        assert torch.equal(xbar, want) and torch.equal(sg, torch.full((B * ns,), s32, device="cuda"))
        assert torch.isnan(xb_all[B * ns:]).all() and torch.isnan(sg_all[B * ns:]).all()


# ---- 6. the schedule on the device -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smax,smin,ann,t0,steps", [(1.0, 0.1, 4, 0, 6), (5.0, 0.05, 4000, 3994, 11), (5.0, 0.05, 0, 0, 2), (2.0, 0.3, -1, 7, 2)],
                         ids=["ramp4_t1-6", "ramp4000_t3995-4005", "no_ramp_0", "no_ramp_negative"])
def test_dae_state_advance_equals_the_host_bit_for_bit(smax, smin, ann, t0, steps):
    lr, beta1 = 5e-3, 0.9
    st, twin = (torch.zeros(4, dtype=torch.int64, device="cuda") for _ in range(2))
    for b in (st, twin):                                      # the block written, not t0 launches
        b[0], b[1] = STRIDE * t0, t0
    for t in range(t0 + 1, t0 + steps + 1):
        L.call("ardae_dae_state_advance", st, STRIDE, lr, beta1, 0.999, smax, smin, ann)
        L.call("ardae_step_state_advance", twin, STRIDE, lr, beta1, 0.999)
        got, ref = st.cpu(), twin.cpu()
        assert torch.equal(got[:3], ref[:3]) and got[:2].tolist() == [STRIDE * t, t]            # rng offset, t, Adam's two coefficients
        tail = got[3:].view(torch.float32)
        want = np.float32(net.dae_sigma(smax, smin, ann, t - 1))
        assert tail[0].numpy().tobytes() == want.tobytes(), (t, float(tail[0]), float(want))
        assert float(tail[1]) == 0.0 and int(ref[3]) == 0


# ---- 7. modules --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FIXTURE_IDS)
def test_module_forward_backward(golden_dir, fid):
    check_module_forward_backward(DAE, golden_dir, fid)


# ---- 8. engine ---------------------------------------------------------------------------------------------------------------------
def inputs(B, d, n):
    return [(torch.randn(B, d, generator=torch.Generator().manual_seed(s)).cuda(),) for s in range(n)]


@pytest.mark.parametrize("kind,B,ns,d,h,nl,act,optimizer", [("grad", 30, 4, 3, 64, 2, "elu", "adam_torch"), ("res", 16, 4, 2, 64, 3, "softplus", "adam_torch"),
                                                             ("grad", 30, 10, 3, 100, 2, "elu", "adam_torch"), ("res", 256, 10, 2, 128, 3, "softplus", "rmsprop")])
def test_engine_replay_equals_eager(kind, B, ns, d, h, nl, act, optimizer):
    cfg = net.DaeConfig(sigma_max=1.0, sigma_min=0.1, sigma_annealing=4, nsigma=ns, optimizer=optimizer, momentum=0.5)
    check_replay_equals_eager(DAE, lambda: fresh_module(DAE, kind, d, h, nl, act), cfg, B, (), inputs(B, d, 6), dict(fused_front=False))


@pytest.mark.parametrize("kind", ["grad", "res"])
def test_engine_follows_the_recorded_trajectory(golden_dir, kind):
    """The notebook's loop on the fixture's x / eps."""
    check_recorded_trajectory(DAE, golden_dir, kind)


@pytest.mark.parametrize("kind", ["grad", "res"])
def test_engine_equals_the_drop_in_module_route(kind):
    """The same six steps through ArdaeScoreEngine and through the module + torch.optim.Adam with a host-computed sigma."""
    B, ns, d, h, nl, act = 30, 4, 3, 64, 2, "elu"
    eng, m, g = check_drop_in_route(DAE, kind, d, h, nl, act, 0, B, (), ns, lambda g: ((0.5 * torch.randn(B, d, generator=g)).cuda(),))
    pts = torch.randn(100, d, generator=g).cuda()
    assert torch.equal(eng.score(pts), m.glogprob(pts)) and torch.equal(eng.score(pts), eng.score(pts, torch.rand(100, generator=g).cuda()))


@pytest.mark.parametrize("kind,optimizer", [("grad", "adam_torch"), ("res", "adam_torch"), ("grad", "amsgrad")])
def test_dae_engine_resumes_bit_identically_across_the_end_of_the_ramp(kind, optimizer):
    """state_dict() after step 2 into a fresh engine under another library seed: steps 3 - 8 (the ramp of 4 steps ends among them; eager,
    eager, captured, replayed there) leave what the uninterrupted run leaves."""
    B, ns, d, h, nl, act = 30, 4, 3, 64, 2, "elu"
    cfg = net.DaeConfig(sigma_max=1.0, sigma_min=0.1, sigma_annealing=4, nsigma=ns, optimizer=optimizer, beta1=0.5)
    other = net.DaeConfig(sigma_max=5.0, sigma_min=0.05, sigma_annealing=4000, nsigma=ns, optimizer=optimizer, beta1=0.5)
    check_resume(DAE, lambda seed: fresh_module(DAE, kind, d, h, nl, act, seed=seed), cfg, other, B, (), inputs(B, d, 8), 2, {})


def test_engine_refuses_mismatched_configs_and_bad_batches():
    good = torch.zeros(32, 2, device="cuda")
    eng = check_refusals(DAE, lambda: fresh_module(DAE, "grad", 2, 64, 3, "softplus"), lambda: fresh_module(ARDAE, "res", 2, 64, 3, "softplus"), 32, (),
                         (good,), good[:31])
    assert eng.step_count == 0 and eng.input_buffer().shape == (32, 2)


# ---- 9. quality, kept small --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["grad", "res"])
def test_learned_score_points_down_the_density(kind):
    """x ~ N(0, 0.25 I_2), sigma 1.0 -> 0.1 over 300 of 400 steps: the learned score against the analytic score of the sigma-smoothed
    density, -x / (0.25 + 0.01), by cosine similarity on 1024 fresh points - and against the drop-in module route on the same data."""
    B, ns, d, h, nl, act, steps = 128, 10, 2, 64, 3, "softplus", 400
    cfg = net.DaeConfig(sigma_max=1.0, sigma_min=0.1, sigma_annealing=300, nsigma=ns)
    g = torch.Generator().manual_seed(2024)
    data = (0.5 * torch.randn(steps, B, d, generator=g)).cuda()
    pts = (0.5 * torch.randn(1024, d, generator=g)).cuda()
    exact = -pts / (0.25 + 0.01)
    net.manual_seed(11)
    eng = net.ArdaeScoreEngine(fresh_module(DAE, kind, d, h, nl, act), cfg, B)
    m = fresh_module(DAE, kind, d, h, nl, act)
    opt = torch.optim.Adam(m.parameters(), lr=cfg.lr)
    for i in range(steps):
        eng.step(data[i])
        opt.zero_grad()
        _, loss = m(data[i].unsqueeze(1).expand(B, ns, d).contiguous().view(B * ns, d), net.dae_sigma(1.0, 0.1, 300, i))
        loss.backward()
        opt.step()
    cos = torch.nn.functional.cosine_similarity
    got, ref = float(cos(eng.score(pts), exact).mean()), float(cos(m.glogprob(pts), exact).mean())
    print(f"{kind}: mean cosine similarity with the analytic score: engine {got:.4f}, drop-in module route {ref:.4f}; last losses {eng.stats()['loss']:.4f} / {float(loss.detach()):.4f}")
    assert got > 0 and got > ref - 0.05
