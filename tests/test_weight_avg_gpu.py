"""--m-weight-avg polyak | swa on the device (ivae_ardae.py:158-164,559-565,644-673,931-950): the `ardae_weight_avg` kernel against
float64 and torch fp32 restatements, the engine's buffer against the recorded trajectory (eager, replayed, two ranks), the in-place
swap for evaluation, checkpoints in both layouts, and the drop-in wrappers net.Polyak / net.SWA.  Rules: optim.py, "Weight averaging"."""
import ctypes
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

import ardae_amd as net
from ardae_amd import _lib as L
from oracle import ardae_oracle as O

pytestmark = pytest.mark.gpu

MC = O.ModelCfg("mnist", 48, 12, 64, 8, 2, "softplus")
CC = O.CdaeCfg("grad", 8, 8, 64, 3)
B, NZ = 16, 32
KIND = {"swa": 0, "polyak": 1}


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _build(dev="cuda"):
    model = net.MNISTIPVAE(input_dim=MC.input_dim, noise_dim=MC.noise_dim, h_dim=MC.h_dim, num_hidden_layers=MC.n_layers,
                           nonlinearity=MC.nonlin, enc_type="concat", z_dim=MC.z_dim)
    cdae = net.MLPGradCARDAE(input_dim=CC.input_dim, context_dim=CC.context_dim, std=1., h_dim=CC.h_dim, num_hidden_layers=CC.n_layers,
                             nonlinearity=CC.nonlin, noise_type="gaussian", enc_ctx=True, enc_input=True)
    model.load_state_dict(O.init_params(O.model_param_spec(MC), 0, O.model_init_special(MC)))
    cdae.load_state_dict(O.init_params(O.cdae_param_spec(CC), 1))
    return model.to(dev), cdae.to(dev)


def _batches(n, seed=21):
    g = torch.Generator().manual_seed(seed)
    return [(torch.bernoulli(torch.full((B, MC.input_dim), 0.3), generator=g).cuda(),
             torch.bernoulli(torch.full((B, MC.input_dim), 0.3), generator=g).cuda()) for _ in range(n)]


def _engine(kind, start, decay=0.9, graph=True, seed=99, **kw):
    model, cdae = _build()
    net.manual_seed(seed)
    cfg = net.TrainConfig(nz_cdae=NZ, m_lr=1e-3, d_lr=1e-3, m_weight_avg=kind, m_weight_avg_start=start, m_weight_avg_decay=decay, **kw)
    return model, cdae, net.ArdaeEngine(model, cdae, cfg, batch_size=B, graph=graph)


def _avg64(traj, kind, start, decay):
    """float64 restatement of the rules over the recorded raw weights traj[t - 1] (t = 1, 2, ...)."""
    avg = None
    for t, p in enumerate(traj, 1):
        if t <= start:
            continue
        k, p = t - (start + 1), p.double()
        if k == 0:
            avg = p.clone()
        else:
            avg += (p - avg) * (1.0 / (k + 1) if kind == "swa" else 1.0 - decay)
    return avg


# ---------------------------------------------------------------------------------------------------------------------------------------
def _launch(avg, p, kind, decay, origin, state=None, t=0):
    L.check(L.lib().ardae_weight_avg(L.ptr(avg), L.ptr(p), avg.numel(), KIND[kind], decay, origin,
                                     None if state is None else ctypes.c_void_p(state.data_ptr()), t, L.stream_ptr()), "ardae_weight_avg")


@pytest.mark.parametrize("kind", ["swa", "polyak"])
@pytest.mark.parametrize("n", [1, 3, 4099, 839472])
@pytest.mark.parametrize("offs", [(0, 0), (1, 1), (3, 3), (0, 1), (2, 0)])
def test_kernel_against_restatements(kind, n, offs):
    """t from the device block across origin - 1, origin and origin + 1 .. origin + 5; avg / p at the given float offsets from a
    16-byte boundary (equal offsets: float4 body with a scalar head; different ones: the scalar path)."""
    decay, origin = 0.97, 7
    g = torch.Generator(device="cuda").manual_seed(n + 10 * offs[0] + offs[1])
    abuf = torch.zeros(n + 8, device="cuda")
    pbuf = torch.zeros(n + 8, device="cuda")
    avg, p = abuf[offs[0]:offs[0] + n], pbuf[offs[1]:offs[1] + n]
    avg.copy_(torch.randn(n, device="cuda", generator=g))
    guard_a, guard_p = abuf.clone(), pbuf.clone()
    state = torch.zeros(4, dtype=torch.int64, device="cuda")
    ref32, ref64 = avg.clone(), avg.double()
    for t in range(origin - 1, origin + 6):
        p.copy_(torch.randn(n, device="cuda", generator=g) * 0.5 + 1.0)
        guard_p = pbuf.clone()
        state[1] = t
        before = avg.clone()
        _launch(avg, p, kind, decay, origin, state=state)
        torch.cuda.synchronize()
        if t < origin:
            assert torch.equal(avg, before)                      # nothing written before the first averaging step
            continue
        k = t - origin
        if k == 0:
            assert torch.equal(avg, p)                           # the first averaging step stores p itself
            ref32, ref64 = p.clone(), p.double()
        else:
            w = float(torch.tensor(1.0 / (k + 1) if kind == "swa" else 1.0 - decay, dtype=torch.float32))
            ref32.add_((p - ref32) * w)
            ref64 += (p.double() - ref64) * (1.0 / (k + 1) if kind == "swa" else 1.0 - decay)
            ulp = torch.nextafter(ref32.abs(), torch.full_like(ref32, float("inf"))) - ref32.abs()
            assert bool(((avg - ref32).abs() <= ulp).all()), (t, float((avg - ref32).abs().max()))
            assert rel_l2(avg, ref64) < 1e-6
        assert torch.equal(pbuf, guard_p)                        # p is read only
    # nothing outside [offs, offs + n) of either buffer was touched
    assert torch.equal(abuf[:offs[0]], guard_a[:offs[0]]) and torch.equal(abuf[offs[0] + n:], guard_a[offs[0] + n:])
    # the host-t form gives the same numbers as the device-t form
    a2 = before.clone()
    _launch(a2, p, kind, decay, origin, t=origin + 5)
    torch.cuda.synchronize()
    assert torch.equal(a2, avg)


# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["polyak", "swa"])
def test_engine_buffer_follows_the_trajectory(kind):
    start, steps, decay = 10, 30, 0.9
    model, _, eng = _engine(kind, start, decay)
    traj = []
    for t, (x1, x2) in enumerate(_batches(steps), 1):
        eng.step(x1, x2)
        traj.append(model.flat_params().detach().cpu().clone())
        if t == start:
            assert not bool(eng.avg.any()) and eng.averaged_params() is None      # no averaging up to and including t = start
        if t == start + 1:
            assert torch.equal(eng.avg, model.flat_params())
    assert eng.plan_summary() is not None                       # the averaging ran inside replayed graphs
    assert rel_l2(eng.avg, _avg64(traj, kind, start, decay)) < 1e-6
    assert rel_l2(eng.avg, traj[-1]) > 1e-4                     # ... and is not just the last weights


def test_graph_replay_equals_eager():
    out = []
    for graph in (True, False):
        model, cdae, eng = _engine("polyak", 5, 0.95, graph=graph)
        for x1, x2 in _batches(20):
            eng.step(x1, x2)
        torch.cuda.synchronize()
        assert (eng.plan_summary() is not None) == graph
        out.append((model.flat_params().cpu().clone(), cdae.flat_params().cpu().clone(), eng.avg.cpu().clone()))
    assert all(torch.equal(a, b) for a, b in zip(*out))


def test_phase_calls_average_too():
    """The eager phase calls (cdae_phase + vae_phase) run the same update as step()."""
    model, _, eng = _engine("swa", 2)
    traj = []
    for x1, x2 in _batches(6):
        eng.cdae_phase(x1)
        eng.vae_phase(x2)
        traj.append(model.flat_params().cpu().clone())
    assert rel_l2(eng.avg, _avg64(traj, "swa", 2, 0.0)) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------------------------
def _iwae(model, x, k=32, seed=3):
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn(x.size(0), k, MC.noise_dim, generator=g).cuda()
    prop = torch.randn(x.size(0), k, MC.z_dim, generator=g).cuda()
    return float(model.logprob(x, sample_size=k, enc_noise=enc, prop_noise=prop))


def test_swap_has_no_side_effects():
    bs = _batches(14)
    model, _, eng = _engine("polyak", 3, 0.9)
    twin_model, _, twin = _engine("polyak", 3, 0.9)
    for x1, x2 in bs[:8]:
        eng.step(x1, x2)
        twin.step(x1, x2)
    raw, avg = model.flat_params().clone(), eng.avg.clone()
    x_eval = bs[0][0]
    ll_raw = _iwae(model, x_eval)
    eng.use_averaged()
    assert torch.equal(model.flat_params(), avg)
    ll = _iwae(model, x_eval)
    fresh, _ = _build()
    with torch.no_grad():
        fresh.flat_params().copy_(avg)
    assert ll == pytest.approx(_iwae(fresh, x_eval), rel=1e-6, abs=0) and ll != ll_raw
    with pytest.raises(RuntimeError):
        eng.step(*bs[8])
    with pytest.raises(RuntimeError):
        eng.model_checkpoint()
    with pytest.raises(RuntimeError):
        eng.vae_phase(bs[8][1])
    eng.use_trained()
    assert torch.equal(model.flat_params(), raw) and torch.equal(eng.avg, avg)
    assert _iwae(model, x_eval) == ll_raw                     # the module sees the raw weights again
    for x1, x2 in bs[8:]:
        eng.step(x1, x2)
        twin.step(x1, x2)
    torch.cuda.synchronize()
    assert torch.equal(model.flat_params(), twin_model.flat_params()) and torch.equal(eng.avg, twin.avg)
    # the context manager, and the swap before the first averaging step (no average yet: the raw weights stay)
    with eng.averaged_weights() as m:
        assert m is model and torch.equal(model.flat_params(), twin.avg)
    assert torch.equal(model.flat_params(), twin_model.flat_params())
    m2, _, e2 = _engine("swa", 100)
    e2.step(*bs[0])
    before = m2.flat_params().clone()
    e2.use_averaged()
    assert torch.equal(m2.flat_params(), before)
    e2.use_trained()
    e2.step(*bs[1])


# ---------------------------------------------------------------------------------------------------------------------------------------
def _save_load(obj, path):
    torch.save(obj, path)
    return torch.load(path, weights_only=True)


def _opt_bufs(eng):
    return [t.clone() for t in eng.opt_m.buffers()]


@pytest.mark.parametrize("kind", ["polyak", "swa"])
def test_checkpoint_resume_is_bit_identical(kind, tmp_path):
    bs = _batches(35)
    model_a, cdae_a, a = _engine(kind, 10)
    for x1, x2 in bs:
        a.step(x1, x2)
    model_b, _, b = _engine(kind, 10)
    for x1, x2 in bs[:25]:
        b.step(x1, x2)
    mck, cck = _save_load(b.model_checkpoint(), tmp_path / "m.pt"), _save_load(b.cdae_checkpoint(), tmp_path / "c.pt")
    skey, bkey = net.optim.weight_avg_keys(kind)
    assert sorted(mck["optimizer"]) == sorted(["opt_state", skey, "param_groups"])
    assert mck["optimizer"]["param_groups"][0]["n_avg"] == 15 and mck["optimizer"]["param_groups"][0]["step_counter"] == 25
    model_c, cdae_c, c = _engine(kind, 10, seed=5)
    c.load_checkpoints(mck, cck)
    for x1, x2 in bs[25:]:
        c.step(x1, x2)
    torch.cuda.synchronize()
    assert torch.equal(model_c.flat_params(), model_a.flat_params()) and torch.equal(cdae_c.flat_params(), cdae_a.flat_params())
    assert all(torch.equal(u, v) for u, v in zip(_opt_bufs(c), _opt_bufs(a)))
    assert torch.equal(c.avg, a.avg)
    # averaging off: the wrapped file loads, the buffer is dropped, training continues exactly
    model_d, cdae_d, d = _engine("none", 10, seed=5)
    assert d.avg is None
    d.load_checkpoints(mck, cck)
    for x1, x2 in bs[25:]:
        d.step(x1, x2)
    assert torch.equal(model_d.flat_params(), model_a.flat_params())
    assert "opt_state" not in d.model_checkpoint()["optimizer"]
    # a plain file loaded past the start: a fresh average from the resume step on
    plain = dict(mck, optimizer={"state": mck["optimizer"]["opt_state"], "param_groups": mck["optimizer"]["param_groups"]})
    model_e, _, e = _engine(kind, 10, seed=5)
    e.load_checkpoints(plain, cck)
    e.step(*bs[25])
    assert torch.equal(e.avg, model_e.flat_params())
    e.step(*bs[26])
    assert e.model_checkpoint()["optimizer"]["param_groups"][0]["n_avg"] == 2
    # a kind mismatch is refused
    _, _, f = _engine("swa" if kind == "polyak" else "polyak", 10)
    with pytest.raises(ValueError):
        f.load_checkpoints(mck, cck)


def test_checkpoints_move_between_engine_and_wrappers(tmp_path):
    bs = _batches(25)
    model, cdae, eng = _engine("polyak", 10)
    for x1, x2 in bs:
        eng.step(x1, x2)
    mck, cck = _save_load(eng.model_checkpoint(), tmp_path / "m.pt"), _save_load(eng.cdae_checkpoint(), tmp_path / "c.pt")
    # engine -> net.Polyak(net.Adam(...))
    m2, _ = _build()
    m2.load_state_dict(mck["state_dict"])
    w = net.Polyak(net.Adam(m2.parameters(), lr=1e-3, betas=(0.5, 0.999)), polyak_start=10, polyak_decay=0.9)
    w.load_state_dict(mck["optimizer"])
    assert (w.param_groups[0]["n_avg"], w.param_groups[0]["step_counter"]) == (15, 25)
    flat_buf = torch.cat([w.state[p]["polyak_buffer"].reshape(-1) for p in m2.parameters()])
    assert torch.equal(flat_buf, eng.avg)
    assert torch.equal(torch.cat([w.optimizer.state[p]["exp_avg"].reshape(-1) for p in m2.parameters()]), eng.opt_m.a)
    # ... and back: net.Polyak's state_dict into a fresh engine
    sd = _save_load(w.state_dict(), tmp_path / "w.pt")
    model3, _, e3 = _engine("polyak", 10, seed=5)
    e3.load_checkpoints({"state_dict": m2.state_dict(), "optimizer": sd}, cck)
    assert e3.step_count == 25 and torch.equal(e3.avg, eng.avg) and torch.equal(e3.opt_m.a, eng.opt_m.a)
    assert e3.model_checkpoint()["optimizer"]["param_groups"][0]["n_avg"] == 15
    # the wrapper continues the same average from the loaded state (one more averaging step on given weights)
    with torch.no_grad():
        for p in m2.parameters():
            p.grad = torch.zeros_like(p)
    w.step()
    assert w.param_groups[0]["n_avg"] == 16
    flat_after = torch.cat([w.state[p]["polyak_buffer"].reshape(-1) for p in m2.parameters()])
    want = eng.avg + (m2.flat_params() - eng.avg) * float(torch.tensor(1.0 - 0.9, dtype=torch.float32))
    assert torch.equal(flat_after, want)


# ---------------------------------------------------------------------------------------------------------------------------------------
def _dropin_step(model, cdae, mopt, copt, xc, xv, noise, nz):
    """The reference loop body (ivae_ardae.py:713-846) on the module surface, as test_engine_gpu.test_module_surface_drop_in_loop."""
    std_scale, delta, beta = 1e4, 0.1, 1.0
    Bn = xc.size(0)
    model.train(); cdae.train()
    copt.zero_grad()
    context = model.encode(xc, std=0).detach()
    latent_mean = model.encode(xc, std=0).detach()
    latent = model.forward_hidden(xc, nz=nz, noise=noise["sampler"]).detach()
    latent_sub_mean = std_scale * (latent - latent_mean)
    std = delta * torch.mean(torch.std(latent_sub_mean, dim=1, keepdim=True), dim=2, keepdim=True)
    _, cdae_loss = cdae(latent_sub_mean, context, std=std * noise["sigma"], scale=std_scale, eps=noise["eps"])
    cdae_loss.backward()
    copt.step()
    model.train(); cdae.eval()
    mopt.zero_grad()
    _, _, latent, model_loss, _, _ = model(xv, beta=beta, eta=0., lmbd=0., nz=1, noise=noise["vae"])
    model_loss.backward(retain_graph=True)
    context = model.encode(xv, std=0).detach()
    latent_mean = model.encode(xv, std=0).detach()
    latent_sub_mean = std_scale * (latent - latent_mean).detach()
    grad = cdae.glogprob(latent_sub_mean, context, std=torch.zeros(Bn, 1, 1, device=xv.device), scale=std_scale).detach()
    (std_scale * (latent - latent_mean)).backward(beta * grad / float(Bn))
    mopt.step()


@pytest.mark.parametrize("kind", ["polyak", "swa"])
def test_drop_in_wrappers_match_the_engine(kind):
    start, steps, decay = 2, 8, 0.9
    tc = O.TrainCfg(nz_cdae=NZ)
    gen = torch.Generator().manual_seed(17)
    noises = [{k: v.cuda().contiguous() for k, v in O.draw_step_noise(MC, tc, B, gen).items()} for _ in range(steps)]
    bs = _batches(steps)
    model, cdae = _build()
    adam = net.Adam(model.parameters(), lr=1e-4, betas=(0.5, 0.999))
    mopt = net.Polyak(adam, polyak_start=start, polyak_freq=1, polyak_decay=decay) if kind == "polyak" else net.SWA(adam, swa_start=start, swa_freq=1)
    copt = net.RMSprop(cdae.parameters(), lr=1e-4, momentum=0.5)
    m_e, c_e = _build()
    eng = net.ArdaeEngine(m_e, c_e, net.TrainConfig(nz_cdae=NZ, m_weight_avg=kind, m_weight_avg_start=start, m_weight_avg_decay=decay), batch_size=B)
    traj = []
    for t, ((x1, x2), nz) in enumerate(zip(bs, noises), 1):
        _dropin_step(model, cdae, mopt, copt, x1, x2, nz, NZ)
        eng.step(x1, x2, noise=nz)
        traj.append(model.flat_params().cpu().clone())
        if t == 5:      # evaluate the averaged weights as evaluate_iws does (ivae_ardae.py:646-647,671-672)
            raw = model.flat_params().clone()
            mopt.use_buf()
            buf_flat = torch.cat([mopt.state[p][f"{kind}_buffer"].reshape(-1) for p in model.parameters()])
            assert torch.equal(buf_flat, raw)                 # the swap parks the raw weights in the buffers
            ll = _iwae(model, x1)
            with pytest.raises(RuntimeError):
                mopt.step()
            mopt.use_sgd()
            assert torch.equal(model.flat_params(), raw)
            fresh, _ = _build()
            with torch.no_grad():
                fresh.flat_params().copy_(torch.cat([mopt.state[p][f"{kind}_buffer"].reshape(-1) for p in model.parameters()]))
            assert ll == pytest.approx(_iwae(fresh, x1), rel=1e-6, abs=0)
    buf = torch.cat([mopt.state[p][f"{kind}_buffer"].reshape(-1) for p in model.parameters()])
    assert rel_l2(buf, _avg64(traj, kind, start, decay)) < 1e-6
    # the two trainers' raw weights agree to fp32 reduction order; the averages must not add to that
    d_raw = rel_l2(model.flat_params(), m_e.flat_params())
    d_avg = rel_l2(buf, eng.avg)
    print(f"{kind}: raw weights drop-in vs engine {d_raw:.3e}, averages {d_avg:.3e}")
    assert d_avg <= 1e-6 + 2 * d_raw


# ---------------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    from ardae_amd import dist
    lo, hi = dist.shard_rows(B)
    model, cdae = _build()
    net.manual_seed(99)
    cfg = net.TrainConfig(nz_cdae=NZ, m_lr=1e-3, d_lr=1e-3, m_weight_avg="polyak", m_weight_avg_start=2, m_weight_avg_decay=0.9)
    eng = net.ArdaeEngine(model, cdae, cfg, batch_size=hi - lo)
    traj = []
    for x1, x2 in _batches(8):
        eng.step(x1[lo:hi].contiguous(), x2[lo:hi].contiguous())
        traj.append(model.flat_params().cpu().clone())
    torch.save({"avg": eng.avg.cpu().clone(), "traj": torch.stack(traj)}, out + f".{rank}")
    torch.distributed.destroy_process_group()


def test_two_ranks_on_one_gpu(tmp_path):
    out = str(tmp_path / "wavg_dp.pt")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = (torch.load(out + f".{r}", weights_only=True) for r in (0, 1))
    assert torch.equal(r0["avg"], r1["avg"]) and torch.equal(r0["traj"], r1["traj"])
    assert rel_l2(r0["avg"], _avg64(list(r0["traj"]), "polyak", 2, 0.9)) < 1e-6
    # against the single process on the whole batch: the averages track as the weights do (sum order of the half batches)
    model, _, eng = _engine("polyak", 2, 0.9)
    p0 = model.flat_params().cpu().clone()
    for x1, x2 in _batches(8):
        eng.step(x1, x2)
    upd, want = (r0["avg"] - p0).double(), (eng.avg.cpu() - p0).double()
    assert float((upd - want).norm() / want.norm()) < 0.1


# ---------------------------------------------------------------------------------------------------------------------------------------
def test_ties_to_the_quality_gate_ema():
    """The quality gate (test_training_quality_gpu.py) averages in the test with ema.lerp_(flat, 1 - decay), starting from the initial
    weights; the engine's Polyak with start 0 starts from the first step's weights.  With the test-side average started the same way,
    the two agree at every step from the second on."""
    from oracle.gen_quality_golden import MC as M2, CC as C2, B as B2, NZ as NZ2, batches
    decay, steps = 0.99, 300
    model = net.MNISTIPVAE(input_dim=M2.input_dim, noise_dim=M2.noise_dim, h_dim=M2.h_dim, num_hidden_layers=M2.n_layers, nonlinearity=M2.nonlin,
                           enc_type="concat", z_dim=M2.z_dim)
    cdae = net.MLPGradCARDAE(input_dim=C2.input_dim, context_dim=C2.context_dim, std=1., h_dim=C2.h_dim, num_hidden_layers=C2.n_layers,
                             nonlinearity=C2.nonlin, noise_type="gaussian", enc_ctx=True, enc_input=True)
    model.load_state_dict(O.init_params(O.model_param_spec(M2), 0, O.model_init_special(M2)))
    cdae.load_state_dict(O.init_params(O.cdae_param_spec(C2), 1))
    model, cdae = model.to("cuda"), cdae.to("cuda")
    net.manual_seed(31337)
    eng = net.ArdaeEngine(model, cdae, net.TrainConfig(nz_cdae=NZ2, m_lr=3e-4, d_lr=3e-4, m_weight_avg="polyak", m_weight_avg_start=0,
                                                       m_weight_avg_decay=decay), batch_size=B2)
    worst, ema = 0.0, None
    for t, (x1, x2) in enumerate(batches(steps), 1):
        eng.step(x1.cuda(), x2.cuda())
        if t == 1:
            ema = model.flat_params().clone()
            assert torch.equal(eng.avg, ema)
            continue
        ema.lerp_(model.flat_params(), 1.0 - decay)
        worst = max(worst, float((eng.avg - ema).double().norm() / ema.double().norm()))
    print(f"engine Polyak vs test-side lerp_ EMA over {steps} steps: worst relative L2 {worst:.3e}")
    assert worst < 1e-6
    assert rel_l2(eng.avg, model.flat_params()) > 1e-4
