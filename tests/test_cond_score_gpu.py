"""Plain conditional DAE score networks on the device (C ABI kinds 10 / 11, the two one-noise-level perturbation kernels, the modules) and
ArdaeCondScoreEngine for both conditional families.

Bars: loss 2e-5 relative, every gradient tensor and glogprob 1e-4 relative L2 against the reference's fp32 fixtures - the bars
tests/test_cdae_gpu.py and tests/test_dae_plain_gpu.py state.  The float64 oracle is the restatement in tests/score_restate.py, which
tests/test_cond_score.py pins to the reference's fp64 fixtures to 1e-12."""
import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from oracle import ardae_oracle as O
from score_gpu_checks import (STRIDE, Harness, check_abi_against_fixture, check_drop_in_route, check_module_forward_backward, check_recorded_trajectory,
                              check_refusals, check_replay_equals_eager, check_resume, check_zero_sigma_column, dae_block, flat_of, fresh_module, guarded,
                              init_params)
from score_restate import CARDAE, CDAE, LOSS_TOL, TENSOR_TOL, cast, grads_on_xbar, rel, score

pytestmark = pytest.mark.gpu
FIXTURE_IDS = [f"{k}_{c}" for k in ("grad", "res") for c in ("b4_s16_d2_softplus", "b5_s12_d3_elu", "b6_s16_d8_tanh", "b8_s8_d2_relu1", "b4_s16_d2_swish")]
FAMILY = {True: CDAE, False: CARDAE}      # by `plain`


# ---- 1. C ABI against every fixture ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FIXTURE_IDS)
def test_abi_matches_the_reference_fixtures(golden_dir, fid):
    check_abi_against_fixture(CDAE, golden_dir, fid)


# ---- 2. the AR-DAE kinds with a zero sigma column are the same function: existing code as the oracle -------------------------------
ORACLE_SHAPES = [(1, 1, 2, 2, 64, 1, "tanh"), (5, 20, 3, 5, 100, 2, "elu"), (4, 16, 2, 2, 64, 3, "softplus"), (8, 40, 8, 24, 256, 3, "softplus"),
                 (64, 1, 32, 32, 256, 3, "softplus")]


@pytest.mark.parametrize("kind", ["grad", "res"])
@pytest.mark.parametrize("B,S,d,c,h,nl,act", ORACLE_SHAPES, ids=[f"b{s[0]}_s{s[1]}_d{s[2]}_h{s[4]}" for s in ORACLE_SHAPES])
def test_plain_kinds_equal_the_ardae_kinds_with_a_zero_sigma_column(kind, B, S, d, c, h, nl, act):
    check_zero_sigma_column(CDAE, kind, B, S, d, c, h, nl, act)


# ---- 3. against float64, with the AR-DAE sibling as the yardstick ------------------------------------------------------------------
F64_SHAPES = [(16, 64, 32, 32, 256, 3, "softplus"), (10, 30, 3, 5, 100, 2, "elu")]


def oracle_grads(kind, p, act, xbar, sigma, eps, ctx, S, dtype, with_sigma_input):
    """The restatement's loss on the SAME fp32 xbar, mse(sigma g(xbar), -eps), and its gradients, in `dtype`"""
    pp, xb, sg, ep, cx = cast(dtype, p, xbar, sigma.reshape(-1, 1), eps, ctx)
    return grads_on_xbar(kind, pp, act, xb, sg, ep, with_sigma_input, cx, S)


@pytest.mark.parametrize("kind", ["grad", "res"])
@pytest.mark.parametrize("B,S,d,c,h,nl,act", F64_SHAPES, ids=[f"b{s[0]}_s{s[1]}_d{s[2]}_h{s[4]}" for s in F64_SHAPES])
def test_gradients_against_float64(kind, B, S, d, c, h, nl, act):
    """e <= max(2 E_sibling, 3 e_ref32 + 2e-6) per gradient tensor (e_ref32: the fp32 restatement's own distance to float64; E_sibling: the
    kind 0 / 1 network of the same widths through the same entry point against float64, worst tensor)."""
    N = B * S
    g = torch.Generator().manual_seed(N + d)
    x, sigma, eps, ctx = torch.randn(N, d, generator=g), 0.1 * torch.randn(N, generator=g), torch.randn(N, d, generator=g), torch.randn(B, c, generator=g)
    xbar = torch.addcmul(x, sigma[:, None], eps)
    spec, spec_sib = CDAE.spec_of(kind, d, h, nl, c), CARDAE.spec_of(kind, d, h, nl, c)
    p, p_sib = init_params(spec, 3), init_params(spec_sib, 11)
    _, g64_sib = oracle_grads(kind, p_sib, act, xbar, sigma, eps, ctx, S, torch.float64, True)
    _, grads_sib, _ = Harness(CARDAE, kind, d, h, nl, act, flat_of(p_sib, spec_sib), c).loss_grads(xbar, sigma, eps, ctx, B, S)
    E_sib = max(rel(grads_sib[n], g64_sib[n]) for n in grads_sib if g64_sib[n] is not None)
    loss64, g64 = oracle_grads(kind, p, act, xbar, sigma, eps, ctx, S, torch.float64, False)
    _, g32 = oracle_grads(kind, p, act, xbar, sigma, eps, ctx, S, torch.float32, False)
    loss, grads, _ = Harness(CDAE, kind, d, h, nl, act, flat_of(p, spec), c).loss_grads(xbar, sigma, eps, ctx, B, S)
    assert abs(float(loss) - float(loss64)) <= LOSS_TOL * abs(float(loss64))
    bad = []
    for n in g64:
        if g64[n] is None:
            assert torch.isnan(grads[n]).all()
            continue
        e, e32 = rel(grads[n], g64[n]), rel(g32[n], g64[n])
        bar = max(2 * E_sib, 3 * e32 + 2e-6)
        print(f"{kind} B={B} S={S} d={d} h={h} L={nl} {act} {n}: e={e:.2e} E_sibling={E_sib:.2e} e_ref32={e32:.2e} bar={bar:.2e}")
        if e > bar:
            bad.append((n, e, bar))
    assert not bad, bad


# ---- 4. the two perturbation kernels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,nz,nstd,z", [(1, 1, 1, 1), (3, 20, 1, 3), (4, 16, 2, 8), (5, 12, 1, 32)])
def test_latent_noise_perturb_kernels(B, nz, nstd, z):
    N, std_scale, seed, first_row = B * nz * nstd, 1.5, 4321, 8
    g = torch.Generator().manual_seed(B + z)
    latent, z0, eps = torch.randn(B, nz, z, generator=g).cuda(), torch.randn(B, z, generator=g).cuda(), torch.randn(N, z, generator=g).cuda()
    u = torch.empty(B * nz, z, device="cuda")
    L.call("ardae_center_scale", latent, z0, B, nz, z, std_scale, u)
    rows = u.view(B, nz, 1, z).expand(B, nz, nstd, z).reshape(N, z)           # row (b, i, j) <- u[b, i]
    block = dae_block(3, 1.0, 0.1, 4)                                          # sigma of i = 2, Philox base offset 3 * STRIDE
    s_block = float(np.float32(net.dae_sigma(1.0, 0.1, 4, 2)))
    outs = {}
    for form, s32, sig, dst in (("value", float(np.float32(0.3)), 0.3, None), ("block", s_block, 123.0, block), ("value_of_block", s_block, s_block, None)):
        (xb_all, xbar), (sg_all, sg) = guarded(N, z), guarded(N)
        L.call("ardae_latent_noise_perturb", latent, z0, eps, B, nz, nstd, z, std_scale, sig, dst, xbar, sg)
        want = (rows.double() + s32 * eps.double()).float()                    # one fma on u as ardae_center_scale rounds it: a single rounding
        assert torch.equal(xbar, want) and torch.equal(sg, torch.full((N,), s32, device="cuda")), form
        assert torch.isnan(xb_all[N:]).all() and torch.isnan(sg_all[N:]).all()
        outs[form] = xbar.clone()
    assert torch.equal(outs["block"], outs["value_of_block"])                  # the two sources of sigma: the same bits
    assert int(L.query("ardae_latent_noise_perturb_draw_ok", nz, nstd, z)) == 1
    # the draw form: ardae_philox_normal_at + the kernel above, bit for bit, with a first row, the block's base offset and guard rows
    for sig, dst, s32 in ((0.3, None, float(np.float32(0.3))), (0.0, block, s_block)):
        drawn = torch.empty(N, z, device="cuda")
        L.call("ardae_philox_normal_at", drawn, N * z, seed, 1, dst, first_row * z)
        ref_x, ref_s = torch.empty(N, z, device="cuda"), torch.empty(N, device="cuda")
        L.call("ardae_latent_noise_perturb", latent, z0, drawn, B, nz, nstd, z, std_scale, sig, dst, ref_x, ref_s)
        (xb_all, xbar), (sg_all, sg), (ep_all, ep) = guarded(N, z), guarded(N), guarded(N, z)
        L.call("ardae_latent_noise_perturb_draw", latent, z0, B, nz, nstd, z, std_scale, sig, dst, seed, 1, first_row, xbar, sg, ep)
        assert torch.equal(ep, drawn) and torch.equal(xbar, ref_x) and torch.equal(sg, ref_s)
        assert torch.equal(sg, torch.full((N,), s32, device="cuda")) and not torch.isnan(ep).any()
        assert torch.isnan(xb_all[N:]).all() and torch.isnan(sg_all[N:]).all() and torch.isnan(ep_all[N:]).all()
    other = torch.empty(N, z, device="cuda")
    L.call("ardae_philox_normal_at", other, N * z, seed, 1 + 3 * STRIDE, None, first_row * z)
    assert torch.equal(ep, other)                                               # the block's base offset moved the draw


# ---- 5. modules --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FIXTURE_IDS)
def test_module_forward_backward(golden_dir, fid):
    check_module_forward_backward(CDAE, golden_dir, fid)


# ---- 6. the AR-DAE kinds: ArdaeEngine's cDAE phase behind its sampler --------------------------------------------------------------
@pytest.mark.parametrize("kind,nstd", [("grad", 1), ("res", 3)])
def test_ar_step_is_the_cdae_phase_of_the_vae_engine(kind, nstd):
    """The same ABI calls at the same shapes: with injected noise, a step on the latent / z0 / context that a tiny ArdaeEngine's cdae_phase
    used leaves the same loss, parameters and optimiser buffers, bit for bit."""
    from test_engine_gpu import build as build_pair
    mc, cc = O.ModelCfg("mnist", 24, 10, 64, 8, 2, "softplus"), O.CdaeCfg(kind, 8, 8, 64, 3)
    B, nz = 4, 16
    N = B * nz * nstd
    tcfg = net.TrainConfig(nz_cdae=nz, nstd_cdae=nstd)
    model, cdae = build_pair(mc, cc)
    model.load_state_dict(O.init_params(O.model_param_spec(mc), 0, O.model_init_special(mc)))
    cdae.load_state_dict(O.init_params(O.cdae_param_spec(cc), 1))
    twin = CARDAE.module(kind, 8, 64, 3, cc.nonlin, 8)
    twin.load_state_dict(cdae.state_dict())
    eng = net.ArdaeEngine(model.cuda(), cdae.cuda(), tcfg, batch_size=B)
    g = torch.Generator().manual_seed(9)
    x = torch.bernoulli(torch.full((B, 24), 0.3), generator=g).cuda()
    noise = {"sampler": torch.randn(B * nz, model._noise_width, generator=g).cuda(), "sigma": torch.randn(B, nz * nstd, 1, generator=g).cuda(),
             "eps": torch.randn(N, 8, generator=g).cuda()}
    eng.cdae_phase(x, noise=noise)
    assert tcfg.d_optimizer == "rmsprop"
    cfg = net.ScoreConfig(delta=tcfg.delta, nsigma=nstd, lr=tcfg.d_lr, optimizer="rmsprop", momentum=tcfg.d_momentum)
    own = net.ArdaeCondScoreEngine(twin.cuda(), cfg, B, nz, std_scale=tcfg.std_scale)
    own.step(eng.latent.view(B, nz, 8), eng.ctx_c, eng.z0, noise={"sigma": noise["sigma"].reshape(-1), "eps": noise["eps"]})
    torch.cuda.synchronize()
    assert torch.equal(own.xbar, eng.xbar) and torch.equal(own.sigma, eng.sigma) and torch.equal(own.std_b, eng.std_b)
    assert torch.equal(own.loss, eng.loss_c) and torch.equal(own.cdae.flat_params(), eng.cdae.flat_params())
    assert all(torch.equal(a, b) for a, b in zip(own.opt.buffers(), eng.opt_c.buffers())) and len(own.opt.buffers()) == 2
    st = own.stats()
    assert st["loss"] == float(eng.loss_c) and st["std_min"] <= st["std_mean"] <= st["std_max"] and st["std_min"] > 0


@pytest.mark.parametrize("kind", ["grad", "res"])
def test_ar_own_draw_forms_equal_the_unfused_launches(kind):
    """One own-draw step in its three forms (draws + first layer in the perturbation kernel; draws in it; two draws and the perturbation): the
    same xbar / sigma / eps bit for bit - the draws are remade at the step's offsets - and loss and parameters within the tolerances."""
    B, S, z, c, h, nl, act = 4, 32, 32, 8, 64, 2, "softplus"
    g = torch.Generator().manual_seed(3)
    mean = torch.randn(B, z, generator=g).cuda()
    latent = (mean[:, None, :] + 0.01 * torch.randn(B, S, z, generator=g).cuda()).contiguous()
    ctx = torch.randn(B, c, generator=g).cuda()
    cfg = net.ScoreConfig(delta=0.1, nsigma=1, lr=1e-4)
    runs = {}
    for form in ("first_layer", "draw", "unfused"):
        net.manual_seed(55)
        eng = net.ArdaeCondScoreEngine(fresh_module(CARDAE, kind, z, h, nl, act, c), cfg, B, S, std_scale=100.0, graph=False)
        assert eng.fused_first and eng.fused_draw
        eng.fused_first, eng.fused_draw = form == "first_layer", form != "unfused"
        eng.step(latent, ctx, mean)
        runs[form] = [t.clone() for t in (eng.xbar, eng.sigma, eng.eps, eng.std_b, eng.loss, eng.cdae.flat_params())]
    xi, eps = torch.empty(B * S, device="cuda"), torch.empty(B * S, z, device="cuda")
    L.call("ardae_philox_normal_at", xi, B * S, 55, STRIDE + 0, None, 0)             # in-step offsets RNG_STRIDE * step + {0: xi, 1: eps}, step 1
    L.call("ardae_philox_normal_at", eps, B * S * z, 55, STRIDE + 1, None, 0)
    assert torch.equal(runs["unfused"][2], eps)
    assert torch.equal(runs["unfused"][1], runs["unfused"][3].repeat_interleave(S) * xi)
    for form in ("first_layer", "draw"):
        assert all(torch.equal(a, b) for a, b in zip(runs[form][:4], runs["unfused"][:4])), form
        assert abs(float(runs[form][4]) - float(runs["unfused"][4])) <= LOSS_TOL * abs(float(runs["unfused"][4]))
        assert rel(runs[form][5].cpu(), runs["unfused"][5].cpu()) <= TENSOR_TOL


# ---- 7. engine ---------------------------------------------------------------------------------------------------------------------
def batches(B, S, z, c, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        mean = torch.randn(B, z, generator=g)
        out.append(((mean[:, None, :] + 0.5 * torch.randn(B, S, z, generator=g)).cuda(), torch.randn(B, c, generator=g).cuda(), mean.cuda()))
    return out


ENGINE_CASES = [(True, "grad", 6, 8, 2, 3, 3, 64, 2, "elu", "adam_torch"), (True, "res", 8, 16, 1, 2, 2, 64, 3, "softplus", "rmsprop"),
                (False, "grad", 4, 32, 1, 32, 8, 64, 2, "softplus", "rmsprop"), (False, "res", 6, 8, 2, 3, 5, 64, 2, "elu", "adam_torch")]


def make_cfg(plain, ns, optimizer):
    if plain:
        return net.DaeConfig(sigma_max=1.0, sigma_min=0.1, sigma_annealing=4, nsigma=ns, optimizer=optimizer, momentum=0.5)
    return net.ScoreConfig(delta=0.1, nsigma=ns, lr=1e-3, optimizer=optimizer, momentum=0.5)


@pytest.mark.parametrize("plain,kind,B,S,ns,z,c,h,nl,act,optimizer", ENGINE_CASES, ids=[f"{'plain' if e[0] else 'ar'}_{e[1]}_{e[10]}" for e in ENGINE_CASES])
def test_engine_replay_equals_eager(plain, kind, B, S, ns, z, c, h, nl, act, optimizer):
    cfg = make_cfg(plain, ns, optimizer)
    raw = batches(B, S, z, c, 6)
    data = [(lat, ctx.view(B, 1, c), mean.view(B, 1, z) if i % 2 else mean) for i, (lat, ctx, mean) in enumerate(raw)]
    flags = dict(fused_first=not plain and z == 32, draw_form=plain)
    eng = check_replay_equals_eager(FAMILY[plain], lambda: fresh_module(FAMILY[plain], kind, z, h, nl, act, c), cfg, B, (S,), data, flags, std_scale=2.0)
    lat_b, mean_b, ctx_b = eng.input_buffers()
    assert lat_b.shape == (B, S, z) and mean_b.shape == (B, z) and ctx_b.shape == (B, c)
    assert torch.equal(lat_b, raw[-1][0]) and torch.equal(ctx_b, raw[-1][1]) and torch.equal(mean_b, raw[-1][2])
    eng.step(lat_b, ctx_b, mean_b)                                              # the static buffers themselves: no copies
    eng.step(lat_b, ctx_b)                                                      # latent_mean=None: zeros
    assert eng.step_count == 8 and not mean_b.any()
    # score(): glogprob(std_scale (latent - mean), ctx, sigma = 0) with the engine's weights, for any B', S'
    lat, ctx, mean = batches(3, 5, z, c, 1, seed=9)[0]
    got = eng.score(lat, ctx.view(3, 1, c), mean)
    u = 2.0 * (lat - mean[:, None, :])
    want = eng.cdae.glogprob(u, ctx.view(3, 1, c)) if plain else eng.cdae.glogprob(u, ctx.view(3, 1, c), torch.zeros(3, 5, 1, device="cuda"))
    assert got.shape == (3, 5, z) and torch.equal(got, want)
    assert torch.equal(eng.score(lat, ctx), eng.score(lat, ctx, torch.zeros(3, 1, z, device="cuda")))


@pytest.mark.parametrize("kind", ["grad", "res"])
def test_plain_engine_draw_form_equals_its_two_launches(kind):
    """The default step (eps made in the perturbation kernel) and draw_form=False (ardae_philox_normal_at, then the perturbation): the same bits."""
    B, S, ns, z, c, h, nl, act = 5, 12, 2, 3, 5, 64, 2, "elu"
    cfg = make_cfg(True, ns, "adam_torch")
    runs = []
    for draw_form in (None, False):
        net.manual_seed(31)
        eng = net.ArdaeCondScoreEngine(fresh_module(CDAE, kind, z, h, nl, act, c), cfg, B, S, std_scale=2.0, draw_form=draw_form)
        assert eng.draw_form == (draw_form is None)
        trace = []
        for lat, ctx, mean in batches(B, S, z, c, 4):
            eng.step(lat, ctx, mean)
            trace += [eng.eps.clone(), eng.xbar.clone(), eng.sigma.clone(), eng.loss.clone(), eng.cdae.flat_params().clone()]
        runs.append(trace)
    assert all(torch.equal(a, b) for a, b in zip(*runs)) and not torch.equal(runs[0][0], runs[0][5])
    want = torch.empty(B * S * ns, z, device="cuda")
    L.call("ardae_philox_normal_at", want, want.numel(), 31, 4 * STRIDE + 1, None, 0)          # step 4's eps: offset RNG_STRIDE * step + 1
    assert torch.equal(runs[0][15], want)


@pytest.mark.parametrize("kind", ["grad", "res"])
def test_plain_engine_follows_the_recorded_trajectory(golden_dir, kind):
    """The update on the fixture's samples / eps."""
    check_recorded_trajectory(CDAE, golden_dir, kind)


@pytest.mark.parametrize("plain,kind", [(True, "grad"), (True, "res"), (False, "grad"), (False, "res")])
def test_engine_equals_the_drop_in_module_route(plain, kind):
    """The same six steps through the engine and through the module + torch.optim with host-computed noise levels."""
    B, S, ns, z, c, h, nl, act = 6, 8, 2, 3, 5, 64, 2, "elu"
    data = iter(batches(B, S, z, c, 6, seed=1))
    check_drop_in_route(FAMILY[plain], kind, z, h, nl, act, c, B, (S,), ns, lambda g: next(data), scale=2.0)


@pytest.mark.parametrize("plain,kind,optimizer", [(True, "grad", "adam_torch"), (True, "res", "amsgrad"), (False, "grad", "rmsprop")])
def test_engine_resumes_bit_identically_across_the_end_of_the_ramp(plain, kind, optimizer):
    """state_dict() after step 2 into a fresh engine under another library seed: steps 3 - 8 (the ramp of 4 steps ends among them; eager,
    eager, captured, replayed there) leave what the uninterrupted run leaves."""
    B, S, ns, z, c, h, nl, act = 6, 8, 2, 3, 5, 64, 2, "elu"
    other = net.DaeConfig(sigma_max=5.0, sigma_min=0.05, sigma_annealing=4000, nsigma=ns, optimizer=optimizer, momentum=0.5)
    check_resume(FAMILY[plain], lambda seed: fresh_module(FAMILY[plain], kind, z, h, nl, act, c, seed=seed), make_cfg(plain, ns, optimizer), other, B, (S,),
                 batches(B, S, z, c, 8), 2, {})


def test_engine_refusals_leave_the_step_count_at_zero():
    z, c = 2, 3
    fresh = lambda plain: lambda: fresh_module(FAMILY[plain], "grad", z, 64, 3, "softplus", c)
    from test_engine_gpu import build as build_pair
    model, _ = build_pair(O.ModelCfg("mnist", 24, 10, 64, 2, 2, "softplus"), O.CdaeCfg("grad", 2, 2, 64, 3))
    with pytest.raises(TypeError, match="ArdaeCondScoreEngine"):       # the VAE loop's engine has no slot for a noise level beside beta
        net.ArdaeEngine(model.cuda(), fresh_module(CDAE, "grad", 2, 64, 3, "softplus", 2), net.TrainConfig(nz_cdae=8), batch_size=4)
    lat, ctx, mean = torch.zeros(4, 8, z, device="cuda"), torch.zeros(4, c, device="cuda"), torch.zeros(4, z, device="cuda")
    for plain in (True, False):
        eng = check_refusals(FAMILY[plain], fresh(plain), fresh(not plain), 4, (8,), (lat, ctx, mean), lat[:3])
        with pytest.raises(ValueError, match="batch_size=4"):
            eng.step(lat, ctx[:3], mean)
        with pytest.raises(ValueError, match="batch_size=4"):
            eng.step(lat, ctx, torch.zeros(4, z + 1, device="cuda"))
        with pytest.raises(ValueError, match="batch_size=4"):
            eng.step(torch.zeros(4, 7, z, device="cuda"), ctx, mean)
        with pytest.raises(ValueError, match="step\\(latent\\)"):
            eng.step(lat.cpu(), ctx, mean)
        with pytest.raises(ValueError, match="score\\(ctx\\)"):
            eng.score(lat, ctx[:3])
        assert eng.step_count == 0 and eng.opt.steps == 0 and eng.state[:2].tolist() == [STRIDE, 1]
    with pytest.raises(ValueError, match="sample_size >= 2"):
        net.ArdaeCondScoreEngine(fresh(False)(), net.ScoreConfig(), 4, 1)


# ---- 8. quality, kept small --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["grad", "res"])
def test_learned_conditional_score_points_at_the_context(kind):
    """z | c ~ N(c, 0.25 I_2), sigma 1.0 -> 0.1 over 300 of 400 steps: the learned score(z, c) against the analytic score of the
    sigma-smoothed conditional, -(z - c) / (0.25 + 0.01), by cosine similarity on 1024 fresh pairs - and against the PyTorch autograd
    restatement (tests/score_restate.py) trained with torch.optim.Adam on the same data."""
    B, S, d, c, h, nl, act, steps = 64, 8, 2, 2, 64, 3, "softplus", 400
    cfg = net.DaeConfig(sigma_max=1.0, sigma_min=0.1, sigma_annealing=300, nsigma=1)
    g = torch.Generator().manual_seed(2024)
    ctxs = torch.randn(steps, B, c, generator=g).cuda()
    lats = (ctxs[:, :, None, :] + 0.5 * torch.randn(steps, B, S, d, generator=g).cuda()).contiguous()
    pc = torch.randn(1024, c, generator=g).cuda()
    pz = (pc + 0.5 * torch.randn(1024, d, generator=g).cuda()).contiguous()
    exact = -(pz - pc) / (0.25 + 0.01)
    net.manual_seed(11)
    eng = net.ArdaeCondScoreEngine(fresh_module(CDAE, kind, d, h, nl, act, c), cfg, B, S)
    p = {k: v.cuda().requires_grad_(True) for k, v in init_params(CDAE.spec_of(kind, d, h, nl, c), 21).items()}
    opt = torch.optim.Adam(list(p.values()), lr=cfg.lr)
    torch.manual_seed(3)
    for i in range(steps):
        eng.step(lats[i], ctxs[i])
        sigma = net.dae_sigma(1.0, 0.1, 300, i)
        eps = torch.randn(B * S, d, device="cuda")
        xbar = (lats[i].view(B * S, d) + sigma * eps).requires_grad_(True)
        loss = torch.nn.functional.mse_loss(sigma * score(kind, p, act, xbar, None, ctxs[i], S, create_graph=True), -eps)
        opt.zero_grad()
        loss.backward()
        opt.step()
    cos = torch.nn.functional.cosine_similarity
    with torch.enable_grad():
        ref_score = score(kind, {k: v.detach() for k, v in p.items()}, act, pz, None, pc, 1).detach()
    got, ref = float(cos(eng.score(pz.view(1024, 1, d), pc).view(1024, d), exact).mean()), float(cos(ref_score, exact).mean())
    print(f"{kind}: mean cosine similarity with the analytic score: engine {got:.4f}, autograd restatement {ref:.4f}; last losses {eng.stats()['loss']:.4f} / {float(loss.detach()):.4f}")
    assert got > 0 and got > ref - 0.05
