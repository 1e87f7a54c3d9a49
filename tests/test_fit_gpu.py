"""Energy-function fitting on the device: the energy kernel, the generator network and its fused front end, torch-style Adam with the
device-side schedules, and ArdaeFitEngine against the trajectory / quality fixtures tools/gen_fit_golden.py wrote with the reference.

Bars: against float64, relative L2 <= 3 x the error of the fp32 reference computation + 2e-6 (the rule of tests/test_ardae_uncond_gpu.py);
elementwise <= 3 x the reference's own worst fp32 element, relative to max(1, |g|); optimiser arithmetic 2 ulp; engine losses 1e-4 relative."""
import os

import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import fit, layout
from score_restate import rel
from test_engine_gpu import assert_update_close
from test_fit import CASES, case_config, case_networks, load, sd_of

pytestmark = pytest.mark.gpu
ENERGIES = ("energy_func1", "energy_func2", "energy_func3", "energy_func4", "normal_energy_func", "regularization_func")
ACT_FN = {"relu": torch.relu, "tanh": torch.tanh}


def kind_of(name):
    return net.energy.KINDS["reg" if name == "regularization_func" else name]


def energy_points(fx, name):
    if name == "normal_energy_func":
        return fx["xn"], float(fx["normal_mu"]), float(fx["normal_logvar"])
    return fx["x"], 0.0, 0.0


# ---- 1. the energy kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ENERGIES)
def test_energy_kernel_against_the_float64_fixture(golden_dir, name):
    fx = load(golden_dir, "fit_energy")
    x, mu, lv = energy_points(fx, name)
    e64, g64, e32, g32 = (fx[f"{name}/{k}"].astype(np.float64) for k in ("e64", "g64", "e32", "g32"))
    e, g = net.energy.evaluate(kind_of(name), torch.tensor(x).cuda(), mu, lv)
    e, g = e.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all() and np.isfinite(e).all()
    l2 = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    worst = lambda a, b: float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))
    for what, dev, r32, r64 in (("gradient", g, g32, g64), ("energy", e, e32, e64)):
        print(f"{name} {what}: device relL2 {l2(dev, r64):.2e} (fp32 reference {l2(r32, r64):.2e}), worst element {worst(dev, r64):.2e} "
              f"(fp32 reference {worst(r32, r64):.2e})")
        assert l2(dev, r64) <= 3 * l2(r32, r64) + 2e-6, what
        assert worst(dev, r64) <= 3 * worst(r32, r64), what
    assert (g[g64 == 0] == 0).all(), "an exact zero of the float64 gradient is not one on the device"
    if name in ("energy_func3", "energy_func4"):      # (0, 7.5): both exponentials underflow in fp32, the log term's gradient is exactly zero
        far = int(np.flatnonzero((x[:, 0] == 0) & (x[:, 1] == 7.5))[0])
        assert g32[far, 0] == 0 and g[far, 0] == 0 and g[far, 1] == 3.0
    # either output may be NULL
    t = torch.tensor(x).cuda()
    only_e, none = net.energy.evaluate(kind_of(name), t, mu, lv, want_grad=False)
    only_g = torch.empty(t.shape, device="cuda")
    L.call("ardae_energy", kind_of(name), t, t.size(0), t.size(1), mu, lv, None, only_g)
    assert none is None and np.array_equal(only_e.cpu().numpy(), e.astype(np.float32)) and np.array_equal(only_g.cpu().numpy(), g.astype(np.float32))


@pytest.mark.parametrize("R", [1, 63, 4097])
@pytest.mark.parametrize("name", ["energy_func1", "energy_func2", "energy_func3", "energy_func4", "normal_energy_func"])
def test_fused_seed_and_mean_energy(golden_dir, name, R):
    fx = load(golden_dir, "fit_energy")
    x, mu, lv = energy_points(fx, name)
    x = x[:R] if len(x) >= R else np.concatenate([x, x[:R - len(x)] * 0.5])
    assert len(x) == R
    d, kind = x.shape[1], kind_of(name)
    xt = torch.tensor(x).cuda()
    score = torch.randn(R, d, generator=torch.Generator().manual_seed(R)).cuda()
    _, g = net.energy.evaluate(kind, xt, mu, lv)
    if len(fx[f"{name}/e64"]) >= R:
        e64 = fx[f"{name}/e64"][:R]
    else:       # the padded rows have no fixture entry: normal_energy_func restated in float64 (test_fit.py pins the form to the fixture)
        assert name == "normal_energy_func"
        e64 = (0.5 * (lv + (x.astype(np.float64) - mu) ** 2 / np.exp(lv) + np.log(2.0 * np.pi))).sum(1)
        assert np.max(np.abs(e64[:4096] - fx[f"{name}/e64"])) <= 1e-12
    partial = torch.empty(L.query("ardae_energy_partial_floats", R), device="cuda")
    state = torch.zeros(fit.FIT_STATE_WORDS, dtype=torch.int64, device="cuda")
    state.view(torch.float32)[8] = 0.8125
    out = []
    for alpha, st in ((0.37, None), (123.0, state), (0.37, None)):
        seed, mean = torch.full((R, d), float("nan"), device="cuda"), torch.zeros(1, device="cuda")
        L.call("ardae_energy_seed", kind, xt, score, R, d, mu, lv, alpha, st, seed, mean, partial)
        a = np.float32(0.8125 if st is not None else alpha)           # the state's alpha wins over the argument
        want = (a * g.cpu().numpy() + score.cpu().numpy()) / np.float32(R)      # three fp32 operations, each rounded
        assert np.array_equal(seed.cpu().numpy(), want)
        out.append((seed.clone(), mean.clone()))
        assert abs(float(mean) - e64.mean()) <= 1e-6 * abs(e64.mean()), (float(mean), e64.mean())
    assert torch.equal(out[0][0], out[2][0]) and torch.equal(out[0][1], out[2][1]) and torch.equal(out[0][1], out[1][1])      # a fixed order: the same bits


def test_energy_callables_are_differentiable_and_shaped_like_the_references(golden_dir):
    fx = load(golden_dir, "fit_energy")
    x = torch.tensor(fx["x"][:500]).cuda().requires_grad_(True)
    for k in (1, 2, 3, 4):
        e = getattr(net.energy, f"energy_func{k}")(x)
        assert e.shape == (500, 1)
        (g,) = torch.autograd.grad((e * 0.25).sum(), x)
        assert rel(g.cpu(), 0.25 * fx[f"energy_func{k}/g64"][:500]) <= 1e-6
    r = net.energy.regularization_func(x)
    assert r.shape == (500, 1) and rel(r.detach().cpu().reshape(-1), fx["regularization_func/e64"][:500]) <= 1e-6
    xn = torch.tensor(fx["xn"][:300]).cuda().requires_grad_(True)
    en = net.energy.normal_energy_func(xn, float(fx["normal_mu"]), float(fx["normal_logvar"]))
    assert en.shape == (300,) and rel(en.detach().cpu(), fx["normal_energy_func/e64"][:300]) <= 1e-6
    (gn,) = torch.autograd.grad(en.mean(), xn)
    assert rel(gn.cpu(), fx["normal_energy_func/g64"][:300] / 300.0) <= 1e-6
    with pytest.raises(AssertionError):
        net.energy.energy_func2(torch.zeros(4, 3, device="cuda"))


# ---- 2. the generator network ------------------------------------------------------------------------------------------------------------
def init_params(spec, seed):
    g = torch.Generator().manual_seed(seed)
    out, bound = {}, None
    for n, shp in spec:
        if n.endswith("weight"):
            bound = 1.0 / shp[1] ** 0.5
        out[n] = (torch.rand(*shp, generator=g) * 2 - 1) * bound
    return out


def restated(p, act, z, dx):
    """x = main(z) and d <dx, x> / d params in the dtype of p (the network restated: nn.Sequential of Linear / act)."""
    p = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    n = len(p) // 2
    hdn = z
    for i in range(n - 1):
        hdn = ACT_FN[act](hdn @ p[f"main.{2 * i}.weight"].t() + p[f"main.{2 * i}.bias"])
    x = hdn @ p[f"main.{2 * (n - 1)}.weight"].t() + p[f"main.{2 * (n - 1)}.bias"]
    return x.detach(), dict(zip(p, torch.autograd.grad((x * dx).sum(), list(p.values()))))


class GenHarness:
    def __init__(self, zd, h, nl, act, p):
        self.net = (zd, h, nl, 2, L.ACT[act])
        self.spec = layout.gen_spec(2, h, zd, nl)
        self.params = torch.cat([p[n].reshape(-1) for n, _ in self.spec]).cuda()
        assert self.params.numel() == L.query("ardae_gen_param_floats", *self.net)
        self.packed = torch.empty(L.query("ardae_gen_packed_floats", *self.net), device="cuda")
        L.call("ardae_gen_pack", *self.net, self.params, self.packed)

    def workspace(self, B):
        return torch.empty(L.query("ardae_gen_workspace_floats", *self.net, B), device="cuda")

    def run(self, z, dx):
        B = z.size(0)
        ws, x, grads = self.workspace(B), torch.empty(B, 2, device="cuda"), torch.full_like(self.params, float("nan"))
        L.call("ardae_gen_forward", *self.net, self.params, self.packed, z, B, ws, ws.numel(), x)
        L.call("ardae_gen_backward", *self.net, self.params, self.packed, z, dx, B, ws, ws.numel(), grads)
        out, off = {}, 0
        for n, shp in self.spec:
            k = int(np.prod(shp))
            out[n] = grads[off:off + k].view(shp).cpu()
            off += k
        return x.cpu(), out, ws


GEN_SHAPES = [(10, 64, 3), (3, 100, 2), (16, 256, 1)]


@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("zd,h,nl", GEN_SHAPES, ids=[f"z{s[0]}_h{s[1]}_L{s[2]}" for s in GEN_SHAPES])
@pytest.mark.parametrize("B", [1, 64, 100])
def test_generator_forward_and_gradients_against_float64(B, zd, h, nl, act):
    p = init_params(layout.gen_spec(2, h, zd, nl), 11 + zd)
    g = torch.Generator().manual_seed(B + h)
    z, dx = torch.randn(B, zd, generator=g), torch.randn(B, 2, generator=g) / B
    x64, g64 = restated({k: v.double() for k, v in p.items()}, act, z.double(), dx.double())
    x32, g32 = restated(p, act, z, dx)
    hn = GenHarness(zd, h, nl, act, p)
    x, grads, _ = hn.run(z.cuda(), dx.cuda())
    assert rel(x, x64) <= 3 * rel(x32, x64) + 2e-6, (rel(x, x64), rel(x32, x64))
    for n in g64:
        assert torch.isfinite(grads[n]).all(), n
        assert rel(grads[n], g64[n]) <= 3 * rel(g32[n], g64[n]) + 2e-6, (n, rel(grads[n], g64[n]), rel(g32[n], g64[n]))


@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("zd,h,nl", [(10, 64, 3), (16, 256, 1), (3, 128, 2), (10, 256, 3)])
@pytest.mark.parametrize("B", [1, 64, 100, 1024])
def test_fused_generator_front_end_equals_draw_plus_layer(B, zd, h, nl, act):
    hn = GenHarness(zd, h, nl, act, init_params(layout.gen_spec(2, h, zd, nl), 5))
    assert L.query("ardae_gen_draw_fused_ok", *hn.net) == 1
    state = torch.zeros(4, dtype=torch.int64, device="cuda")
    state[0] = 48                                              # a base offset in the step state
    seed, off = 0xABCDEF, (1 << 62) + 3
    z_ref = torch.empty(B, zd, device="cuda")
    L.call("ardae_philox_normal_at", z_ref, B * zd, seed, off, state, 0)
    ws_ref, x_ref = hn.workspace(B), torch.empty(B, 2, device="cuda")
    L.call("ardae_gen_forward", *hn.net, hn.params, hn.packed, z_ref, B, ws_ref, ws_ref.numel(), x_ref)
    z, ws, x = torch.full((B, zd), float("nan"), device="cuda"), hn.workspace(B), torch.empty(B, 2, device="cuda")
    L.call("ardae_gen_draw_forward", *hn.net, hn.params, hn.packed, B, seed, off, state, z, ws, ws.numel(), x)
    assert torch.equal(z, z_ref), "the fused draw is not ardae_philox_normal_at's"
    assert rel(ws[:B * h].cpu(), ws_ref[:B * h].cpu()) <= 1e-6
    assert rel(x.cpu(), x_ref.cpu()) <= 2e-6
    assert abs(float(z.mean())) < 5.0 / (B * zd) ** 0.5 and (B * zd < 64 or 0.5 < float(z.std()) < 1.5)


def test_module_route_gives_the_abi_gradients():
    """The notebook's generator cell on net.Generator + net.energy.energy_func4 + torch autograd: two backward calls through one
    forward; the sum of their gradients is ardae_gen_backward on the summed seed."""
    B, alpha = 96, 0.31
    gen = net.Generator(input_dim=2, hidden_dim=64, z_dim=10).cuda()
    assert gen.energy_func is net.energy.energy_func4
    z = torch.randn(B, 10, generator=torch.Generator().manual_seed(1)).cuda()
    s2 = torch.randn(B, 2, generator=torch.Generator().manual_seed(2)).cuda() / B
    x, loss = gen(z=z)
    (0 + alpha * loss).backward(retain_graph=True)
    x.backward(s2)
    e, g = net.energy.evaluate(net.energy.KINDS["energy_func4"], x.detach())
    assert abs(float(loss.detach()) - float(e.mean())) <= 1e-6 * abs(float(e.mean()))
    hn = GenHarness(10, 64, 3, "relu", {n: p.detach().cpu() for n, p in gen.named_parameters()})
    x_abi, grads, _ = hn.run(z, (alpha / B) * g + s2)
    assert torch.equal(x_abi, x.detach().cpu())
    for n, p in gen.named_parameters():
        assert rel(p.grad.cpu(), grads[n]) <= 1e-5, (n, rel(p.grad.cpu(), grads[n]))
    drawn, _ = gen(32)                       # own draw from the host Philox stream
    assert drawn.shape == (32, 2) and torch.isfinite(drawn).all()


# ---- 3. torch.optim.Adam with the schedules on the device --------------------------------------------------------------------------------
def test_adam_and_schedules_follow_torch():
    cfg = net.FitConfig(lr=1e-3, m_beta1=0.5, lr_step_size=3, lr_gamma=0.5, lr_min=3e-4, alpha_init=0.01, alpha_fin=1.0, alpha_annealing=5)
    n, g = 1003, torch.Generator().manual_seed(0)
    p0 = torch.randn(n, generator=g)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], lr=cfg.lr, betas=(cfg.m_beta1, 0.999))
    p, m, v = p0.clone().cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    state = torch.zeros(fit.FIT_STATE_WORDS, dtype=torch.int64, device="cuda")
    advance = lambda: L.call("ardae_fit_state_advance", state, 16, cfg.lr, cfg.m_beta1, 0.999, cfg.lr_step_size, cfg.lr_gamma, cfg.lr_min, cfg.alpha_init,
                             cfg.alpha_fin, cfg.alpha_annealing)
    advance()
    lrs = []
    for i in range(8):
        tail = state.view(torch.float32)[8:12].tolist()
        assert tail[0] == np.float32(fit.alpha_at(cfg, i)) and tail[1] == np.float32(fit.step_lr(cfg, i))
        assert int(state[0]) == 16 * (i + 1) and int(state[1]) == i + 1
        lrs.append(tail[1])
        grad = torch.randn(n, generator=g) * (10.0 ** torch.randint(-4, 2, (n,), generator=g).float())
        ref.grad = grad.clone()
        assert opt.param_groups[0]["lr"] == fit.step_lr(cfg, i)
        opt.step()
        opt.param_groups[0]["lr"] = fit.step_lr(cfg, i + 1)           # StepLR.step(), after the optimiser
        L.call("ardae_adam_torch_step_dev", p, grad.cuda(), m, v, n, cfg.m_beta1, 0.999, 1e-8, state)
        advance()
        assert state.view(torch.float32)[10:12].tolist() == tail[:2]   # the iteration just done keeps its pair
        want = ref.detach()
        assert bool(((p.cpu() - want).abs() <= 2.4e-7 * want.abs() + 1e-9).all()), i          # 2 ulp
        st = opt.state[ref]
        assert rel(m.cpu(), st["exp_avg"]) <= 1e-6 and rel(v.cpu(), st["exp_avg_sq"]) <= 1e-6
    assert len(set(lrs)) == 3 and lrs[-1] == np.float32(3e-4)          # two boundaries crossed, the floor reached


# ---- 4. the engine -----------------------------------------------------------------------------------------------------------------------
def engine_of(fx, graph=True, cfg=None, seed_modules=None):
    gen, dae = case_networks(fx)
    gen.load_state_dict(sd_of(fx, "sd_gen/")); dae.load_state_dict(sd_of(fx, "sd_dae/"))
    return net.ArdaeFitEngine(gen.cuda(), dae.cuda(), cfg or case_config(fx), int(fx["cfg/B"]), graph=graph)


@pytest.mark.parametrize("case", CASES)
def test_engine_follows_the_recorded_trajectory(golden_dir, case):
    """Teacher-forced: after every iteration the parameters are reset to the fixture's (the optimiser states stay the engine's own)."""
    fx, fx64 = load(golden_dir, "fit_traj_" + case), load(golden_dir, f"fit_traj_{case}_f64")
    eng = engine_of(fx)
    cuda = lambda a: torch.tensor(a).cuda().contiguous()
    for i in range(len(fx["lr"])):
        before = {"gen": {n: p.detach().clone() for n, p in eng.gen.named_parameters()}, "dae": {n: p.detach().clone() for n, p in eng.dae.named_parameters()}}
        eng.step(noise={"z": cuda(fx["z"][i]), "sigma": cuda(fx["sigma"][i]), "eps": cuda(fx["eps"][i])})
        st = eng.stats()
        print(f"{case} {i}: model loss {st['model_loss']:.7f} ({fx['model_loss'][i]:.7f}, fp64 {fx64['model_loss'][i]:.7f}), dae loss {st['dae_loss']:.7f} "
              f"({fx['dae_loss'][i]:.7f}), alpha {st['alpha']}, lr {st['lr']}")
        assert abs(st["model_loss"] - fx["model_loss"][i]) <= 1e-4 * abs(fx["model_loss"][i])
        assert abs(st["dae_loss"] - fx["dae_loss"][i]) <= 1e-4 * abs(fx["dae_loss"][i])
        assert st["alpha"] == np.float32(fx["alpha"][i]) and st["lr"] == np.float32(fx["lr"][i])
        for which, mod in (("gen", eng.gen), ("dae", eng.dae)):
            for n, p in mod.named_parameters():
                want = torch.tensor(fx[f"{i}/{which}/{n}"])
                if which == "dae" and n in eng.dae._no_grad_names:
                    assert torch.equal(p.detach().cpu(), want)
                else:
                    assert_update_close(p.detach().cpu(), before[which][n].cpu(), want, (case, i, which, n))
        eng.gen.load_state_dict(sd_of(fx, f"{i}/gen/")); eng.dae.load_state_dict(sd_of(fx, f"{i}/dae/"))
        eng.repack()
    assert eng.step_count == 6 and eng.score.step_count == 12


def snapshot(eng):
    return [eng.gen.flat_params().clone(), eng.dae.flat_params().clone(), eng.exp_avg.clone(), eng.exp_avg_sq.clone(), eng.state.clone(), eng.score.state.clone(),
            eng.x.clone(), eng.score.sigma.clone()] + [b.clone() for b in eng.score.opt.buffers()]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_replay_equals_eager_and_a_resumed_run_continues_bit_identically(golden_dir, case, fused):
    fx = load(golden_dir, "fit_traj_" + case)
    cfg = case_config(fx)
    cfg.lr_step_size, cfg.alpha_annealing = 3, 5              # both schedules move inside the 8 iterations
    runs = {}
    for mode in ("graph", "eager", "resumed"):
        net.manual_seed(4242)
        eng = engine_of(fx, graph=mode != "eager", cfg=cfg)
        if not fused:
            eng.fused_front = eng.score.fused_front = False
        scalars = []
        for i in range(8):
            if mode == "resumed" and i == 4:
                sd = eng.state_dict()
                assert list(sd["optimizer"]["state"][0]) == ["step", "exp_avg", "exp_avg_sq"] and float(sd["optimizer"]["state"][0]["step"]) == 4
                assert sd["scheduler"]["last_epoch"] == 4 and sd["optimizer"]["param_groups"][0]["lr"] == fit.step_lr(cfg, 4)
                net.manual_seed(1)                                 # the checkpoint, not the process, carries the RNG state
                eng = engine_of(fx, graph=True, cfg=cfg)
                if not fused:
                    eng.fused_front = eng.score.fused_front = False
                eng.load_state_dict(sd)
            eng.step()
            if mode == "graph" and i == 5:
                assert eng.sample(7).shape == (7, 2)               # host-stream draws: no training state is touched
            scalars.append(torch.cat([eng.model_loss, eng.score.loss, eng.state.view(torch.float32)[10:12]]).clone())
        torch.cuda.synchronize()
        assert (eng._graph is not None) == (mode != "eager")
        runs[mode] = (snapshot(eng), torch.stack(scalars))
    (s1, c1), (s2, c2), (s3, c3) = runs["graph"], runs["eager"], runs["resumed"]
    assert torch.equal(c1, c2) and all(torch.equal(a, b) for a, b in zip(s1, s2)), "replayed != eager"
    assert torch.equal(c1[4:], c3[4:]) and all(torch.equal(a, b) for a, b in zip(s1, s3)), "the resumed run drifted"
    assert torch.isfinite(c1).all() and len(set(c1[:, 0].tolist())) == 8                              # fresh draws every iteration
    assert c1[:, 3].tolist() == [float(np.float32(fit.step_lr(cfg, i))) for i in range(8)] and len(set(c1[:, 3].tolist())) == 3
    assert c1[:, 2].tolist() == [float(np.float32(fit.alpha_at(cfg, i))) for i in range(8)]
    assert int(s1[4][0]) == 16 * 9 and int(s1[4][1]) == 9 and int(s1[5][1]) == 17                     # the blocks describe the coming iteration


def test_engine_refuses_bad_noise_and_networks(golden_dir):
    fx = load(golden_dir, "fit_traj_e4_res")
    eng = engine_of(fx)
    B, U, zd, N = eng.B, eng.U, eng.zd, eng.B * 4
    good = lambda: {"z": torch.zeros(U + 1, B, zd, device="cuda"), "sigma": torch.zeros(U, N, device="cuda"), "eps": torch.zeros(U, N, 2, device="cuda")}
    before = snapshot(eng)
    for key, bad in (("z", torch.zeros(U, B, zd, device="cuda")), ("z", torch.zeros(U + 1, B, zd + 1, device="cuda")), ("sigma", torch.zeros(U, N + 1, device="cuda")),
                     ("eps", torch.zeros(U, N, 3, device="cuda")), ("eps", torch.zeros(U, N, 2)), ("sigma", torch.zeros(U, N, device="cuda").double()),
                     ("z", torch.zeros(U + 1, B, 2 * zd, device="cuda")[:, :, ::2]), ("sigma", [0.0] * N),
                     # the right number of values in another arrangement is refused too, not reinterpreted
                     ("z", torch.zeros(U + 1, zd, B, device="cuda")), ("eps", torch.zeros(U, 2, N, device="cuda")), ("sigma", torch.zeros(U, N, 1, device="cuda"))):
        n = good()
        n[key] = bad
        with pytest.raises(ValueError, match=key + " must be"):
            eng.step(noise=n)
    with pytest.raises(ValueError, match="keys"):
        eng.step(noise={"z": good()["z"]})
    with pytest.raises(ValueError, match="positive"):
        eng.sample(0)
    assert eng.step_count == 0 and all(torch.equal(a, b) for a, b in zip(before, snapshot(eng))), "a refused call reached the device"
    gen, dae = case_networks(fx)
    with pytest.raises(TypeError):
        net.ArdaeFitEngine(gen.cuda(), net.MLPGradCARDAE(input_dim=2, context_dim=2, h_dim=16, nonlinearity="softplus").cuda(), net.FitConfig(), 8)
    with pytest.raises(ValueError, match="input_dim"):
        net.ArdaeFitEngine(gen, net.MLPResARDAE(input_dim=3, h_dim=16, nonlinearity="softplus").cuda(), net.FitConfig(energy="normal_energy_func"), 8)
    with pytest.raises(ValueError, match="2 dimensions"):
        net.ArdaeFitEngine(net.Generator(input_dim=3, hidden_dim=16).cuda(), net.MLPResARDAE(input_dim=3, h_dim=16, nonlinearity="softplus").cuda(), net.FitConfig(), 8)


@pytest.mark.parametrize("fused", [True, False])
def test_engine_draws_with_the_documented_philox_offsets(golden_dir, fused):
    """What the launches actually draw: the generator's last sample of iteration i is ardae_philox_normal_at at 2^62 + 16 (i + 1) + U, the
    embedded AR-DAE update k draws sigma / eps at 16 k + {0, 1} - the offsets ArdaeFitEngine.philox_offsets lists (and test_fit.py shows disjoint)."""
    fx = load(golden_dir, "fit_traj_e4_res")
    net.manual_seed(991)
    eng = engine_of(fx, graph=False)
    eng.fused_front = eng.score.fused_front = fused
    U, B, zd, N, d = eng.U, eng.B, eng.zd, eng.score.N, eng.d

    def draw(n, offset):
        out = torch.empty(n, device="cuda")
        L.call("ardae_philox_normal_at", out, n, 991, offset, None, 0)
        return out
    for i in range(3):
        eng.step()
        off = net.ArdaeFitEngine.philox_offsets(i, U)
        assert off["z"][U] == (1 << 62) + 16 * (i + 1) + U and off["dae"][U - 1] == (16 * (i * U + U), 16 * (i * U + U) + 1)
        assert torch.equal(eng.z, draw(B * zd, off["z"][U]).view(B, zd))
        assert torch.equal(eng.score.eps, draw(N * d, off["dae"][U - 1][1]).view(N, d))
        assert torch.equal(eng.score.sigma, float(eng.cfg.delta) * draw(N, off["dae"][U - 1][0]))
        for other in off["z"][:U]:
            assert not torch.equal(eng.z, draw(B * zd, other).view(B, zd))


def test_load_state_dict_of_a_checkpoint_assembled_from_torch_objects(golden_dir):
    """Without the "engine" entry the device blocks are rebuilt from the schedule's last_epoch and the optimisers' step counts."""
    fx = load(golden_dir, "fit_traj_e1_grad")
    cfg = case_config(fx)
    eng = engine_of(fx, cfg=cfg)
    for _ in range(4):
        eng.step()
    sd = eng.state_dict()
    del sd["engine"]
    new = engine_of(fx, cfg=cfg)
    new.load_state_dict(sd)
    assert (new.step_count, new.score.step_count, new.score.opt.steps) == (4, 8, 8)
    assert new.state[:2].tolist() == [16 * 5, 5] and new.score.state[:2].tolist() == [16 * 9, 9]         # both describe the coming step
    assert new.state.view(torch.float32)[8:10].tolist() == [float(np.float32(fit.alpha_at(cfg, 4))), float(np.float32(fit.step_lr(cfg, 4)))]
    assert torch.equal(new.state[2], eng.state[2])                                                        # Adam's coefficients for t = 5
    assert torch.equal(new.gen.flat_params(), eng.gen.flat_params()) and torch.equal(new.exp_avg_sq, eng.exp_avg_sq)
    assert all(torch.equal(a, b) for a, b in zip(new.score.opt.buffers(), eng.score.opt.buffers()))
    new.step()
    st = new.stats()
    assert st["lr"] == np.float32(fit.step_lr(cfg, 4)) and st["alpha"] == np.float32(fit.alpha_at(cfg, 4)) and np.isfinite(st["model_loss"])


# ---- 5. quality --------------------------------------------------------------------------------------------------------------------------
def test_fit_quality_against_the_reference_seeds(golden_dir):
    """4 device seeds of the fixture's short fit against the reference's 8: mean energy and per-axis standard deviation of 4096 final
    samples, |device mean - reference mean| <= 3 x the combined standard error (the form of test_training_quality_against_the_reference_seeds)."""
    q = load(golden_dir, "fit_quality")
    cfg, steps, points = case_config(q), int(q["cfg/steps"]), int(q["cfg/points"])
    ref, untrained = q["trained"], q["untrained"]
    dev = []
    for seed in range(4):
        torch.manual_seed(5000 + seed)          # module init
        net.manual_seed(5000 + seed)            # the Philox streams
        gen, dae = case_networks(q)
        eng = net.ArdaeFitEngine(gen.cuda(), dae.cuda(), cfg, int(q["cfg/B"]))
        for _ in range(steps):
            eng.step()
        x = eng.sample(points)
        e, _ = net.energy.evaluate(eng.kind, x, want_grad=False)
        dev.append([float(e.mean())] + x.std(0).tolist())
    dev = np.array(dev)
    for j, what in enumerate(("mean energy", "std of axis 0", "std of axis 1")):
        gap = abs(dev[:, j].mean() - ref[:, j].mean())
        bar = 3 * np.sqrt(ref[:, j].var(ddof=1) / len(ref) + dev[:, j].var(ddof=1) / len(dev))
        print(f"{what}: device {dev[:, j].mean():.4f} +- {dev[:, j].std(ddof=1):.4f}, reference {ref[:, j].mean():.4f} +- {ref[:, j].std(ddof=1):.4f}, "
              f"untrained {untrained[:, j].mean():.4f}; gap {gap:.4f} <= {bar:.4f}")
        assert gap <= bar, what
