"""Unconditional AR-DAE score networks on the device: C ABI kinds 2 / 3, the fused front end, the modules and ArdaeScoreEngine.

Bars: loss 2e-5 relative, every gradient tensor and glogprob 1e-4 relative L2 against the reference's fp32 fixtures - the bars
tests/test_cdae_gpu.py states for the conditional kinds.  The float64 oracle is the restatement in tests/test_ardae_uncond.py, which that
file pins to the reference's fp64 fixtures to 1e-12."""
import os

import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import layout
from oracle import ardae_oracle as O
from test_ardae_uncond import KIND_ID, load, rel, score, state_dict_of
from test_cdae_gpu import CdaeHarness, oracle64_grads, split_flat

pytestmark = pytest.mark.gpu
LOSS_TOL, TENSOR_TOL = 2e-5, 1e-4
FIXTURE_IDS = [f"{k}_{c}" for k in ("grad", "res") for c in ("n60_d3_elu", "n64_d2_relu1", "n64_d2_softplus", "n64_d2_swish", "n96_d8_tanh")]


def fixture(golden_dir, fid):
    return load(os.path.join(golden_dir, f"ardae_uncond_{fid}.npz"))


def meta(fx):
    N, d, h, nl = (int(v) for v in fx["shape"])
    return str(fx["kind"]), str(fx["act"]), N, d, h, nl


def flat_of(p, spec):
    return torch.cat([p[n].reshape(-1).float() for n, _ in spec])


def init_params(spec, seed):
    """nn.Linear's family: U(+-1/sqrt(fan_in)) for weight and bias."""
    g = torch.Generator().manual_seed(seed)
    out, bound = {}, None
    for n, shp in spec:
        if n.endswith("weight"):
            bound = 1.0 / shp[1] ** 0.5
        out[n] = (torch.rand(*shp, generator=g) * 2 - 1) * bound
    return out


class Harness:
    """The C ABI for one unconditional network (kind 2 / 3)."""

    def __init__(self, kind, d, h, nl, act, flat_params):
        self.kind, self.d_in, self.h = kind, d, h
        self.spec = layout.dae_spec(kind, d, h, nl)
        self.d = L.CdaeDesc(KIND_ID[kind], d, 0, h, nl, L.ACT[act])
        assert L.query("ardae_cdae_param_floats", self.d) == flat_params.numel()
        self.params = flat_params.cuda()
        self.packed = torch.empty(L.query("ardae_cdae_packed_floats", self.d), device="cuda")
        L.call("ardae_cdae_pack", self.d, self.params, self.packed)

    def loss_grads(self, xbar, sigma, eps, B=None, S=1):
        N = xbar.size(0)
        B = N if B is None else B
        assert B * S == N
        self.ws = torch.empty(L.query("ardae_cdae_workspace_floats", self.d, B, S, 1), device="cuda")
        loss, grads = torch.zeros(1, device="cuda"), torch.full_like(self.params, float("nan"))
        sc = torch.empty(N, self.d_in, device="cuda")
        xbar, sigma, eps = (t.contiguous().cuda() for t in (xbar, sigma.reshape(-1), eps))
        L.call("ardae_cdae_loss_grads", self.d, self.params, self.packed, xbar, sigma, eps, None, B, S, self.ws, self.ws.numel(), loss, grads, sc)
        torch.cuda.synchronize()
        return loss.cpu(), split_flat(grads.cpu(), self.spec), sc.cpu()

    def glogprob(self, x, sigma):
        N = x.size(0)
        ws = torch.empty(L.query("ardae_cdae_workspace_floats", self.d, N, 1, 0), device="cuda")
        out = torch.empty(N, self.d_in, device="cuda")
        x, sigma = x.contiguous().cuda(), sigma.reshape(-1).contiguous().cuda()
        L.call("ardae_cdae_score", self.d, self.params, self.packed, x, sigma, None, N, 1, ws, ws.numel(), out)
        torch.cuda.synchronize()
        return out.cpu()

    def fused(self, x, B, ns, delta, seed, first_row=0, state=None):
        """-> loss, grads, xbar, sigma, eps, h_1 of ardae_dae_perturb_loss_grads"""
        N = B * ns
        ws = torch.empty(L.query("ardae_cdae_workspace_floats", self.d, N, 1, 1), device="cuda")
        loss, grads = torch.zeros(1, device="cuda"), torch.full_like(self.params, float("nan"))
        xbar, sigma, eps = torch.empty(N, self.d_in, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, self.d_in, device="cuda")
        L.call("ardae_dae_perturb_loss_grads", self.d, self.params, self.packed, x, B, ns, delta, seed, 3, 4, state, first_row, xbar, sigma, eps, ws,
               ws.numel(), loss, grads)
        torch.cuda.synchronize()
        return loss.cpu(), split_flat(grads.cpu(), self.spec), xbar, sigma, eps, ws[:N * self.h].clone()

    def unfused(self, x, B, ns, delta, seed, first_row=0, state=None):
        N = B * ns
        n, eps = torch.empty(N, device="cuda"), torch.empty(N, self.d_in, device="cuda")
        L.call("ardae_philox_normal_at", n, N, seed, 3, state, first_row)
        L.call("ardae_philox_normal_at", eps, N * self.d_in, seed, 4, state, first_row * self.d_in)
        sigma = delta * n                                   # one fp32 multiply
        xbar = torch.empty(N, self.d_in, device="cuda")
        L.call("ardae_dae_perturb", x, sigma, eps, B, ns, self.d_in, xbar)
        loss, grads, _ = self.loss_grads(xbar, sigma, eps)
        return loss, grads, xbar, sigma, eps, self.ws[:N * self.h].clone()


def assert_matches_reference(got, fx, prefix, what):
    for n, g in got.items():
        if f"{prefix}/{n}/none" in fx:
            assert torch.isnan(g).all(), f"{what}: {n} must stay untouched (the reference's .grad is None)"
        else:
            assert not torch.isnan(g).any(), (what, n)
            e = rel(g, fx[f"{prefix}/{n}"])
            assert e <= TENSOR_TOL, f"{what}: {n} relL2 {e:.2e}"


# ---- 5. C ABI against every fixture ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FIXTURE_IDS)
def test_abi_matches_the_reference_fixtures(golden_dir, fid):
    fx = fixture(golden_dir, fid)
    kind, act, N, d, h, nl = meta(fx)
    x, std, eps = (torch.tensor(fx[k]) for k in ("x", "std", "eps"))
    hn = Harness(kind, d, h, nl, act, flat_of(state_dict_of(fx), layout.dae_spec(kind, d, h, nl)))
    loss, grads, sc = hn.loss_grads(x + std * eps, std, eps)
    print(f"{fid}: loss {float(loss):.7f} (reference {float(fx['loss']):.7f})")
    assert abs(float(loss) - float(fx["loss"])) <= LOSS_TOL * abs(float(fx["loss"]))
    assert_matches_reference(grads, fx, "g", fid)
    assert (kind == "grad") == any(torch.isnan(g).any() for g in grads.values())       # neglogprob.fc.bias, and nothing else
    assert rel(hn.glogprob(x, torch.zeros(N)), fx["glog0"]) <= TENSOR_TOL
    assert rel(hn.glogprob(x, std), fx["glog"]) <= TENSOR_TOL
    # N = B S in any factorisation: the same bits
    if N % 4 == 0:
        loss2, grads2, sc2 = hn.loss_grads(x + std * eps, std, eps, N // 4, 4)
        assert torch.equal(loss, loss2) and torch.equal(sc, sc2) and all(torch.equal(torch.nan_to_num(grads[n]), torch.nan_to_num(grads2[n])) for n in grads)


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
    spec = layout.dae_spec(kind, d, h, nl)
    p = init_params(spec, 3)
    xbar = torch.addcmul(x, sigma, eps)

    def oracle(dtype):                          # the restatement's loss on the SAME fp32 xbar: mse(sigma g(xbar, sigma), -eps)
        pp = {k: v.to(dtype).requires_grad_(True) for k, v in p.items()}
        xb = xbar.to(dtype).requires_grad_(True)
        loss = torch.nn.functional.mse_loss(sigma.to(dtype) * score(kind, pp, act, xb, sigma.to(dtype), create_graph=True), -eps.to(dtype))
        return loss.detach(), dict(zip(pp, torch.autograd.grad(loss, list(pp.values()), allow_unused=True)))
    loss64, g64 = oracle(torch.float64)
    loss32, g32 = oracle(torch.float32)
    loss, grads, _ = Harness(kind, d, h, nl, act, flat_of(p, spec)).loss_grads(xbar, sigma, eps)
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
    spec = layout.dae_spec(kind, d, h, nl)
    hn = Harness(kind, d, h, nl, act, flat_of(init_params(spec, 9), spec))
    assert L.query("ardae_dae_perturb_fused_ok", hn.d, ns) == 1
    x = torch.randn(B, d, generator=torch.Generator().manual_seed(B)).cuda()
    delta, seed = 0.7, 1234
    state = torch.zeros(4, dtype=torch.int64, device="cuda")
    L.call("ardae_step_state_advance", state, 16 * 5, 1e-3, 0.5, 0.999)
    for st in (None, state):
        lf, gf, xb_f, sg_f, ep_f, h1_f = hn.fused(x, B, ns, delta, seed, 0, st)
        lu, gu, xb_u, sg_u, ep_u, h1_u = hn.unfused(x, B, ns, delta, seed, 0, st)
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
    assert not torch.equal(sg_f, hn.fused(x, B, ns, delta, seed)[3])              # the state's base offset moved the draws
    # rows 4 k ... of the larger draw: the samples from b0 on, first_row = b0 ns (a multiple of 4)
    b0 = next(b for b in range(1, B) if (b * ns) % 4 == 0)
    _, _, xb_all, sg_all, ep_all, _ = hn.fused(x, B, ns, delta, seed)
    _, _, xb_t, sg_t, ep_t, _ = hn.fused(x[b0:].contiguous(), B - b0, ns, delta, seed, b0 * ns)
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
    kind, act, N, d, h, nl = meta(fx)
    m = (net.MLPGradARDAE if kind == "grad" else net.MLPResARDAE)(input_dim=d, h_dim=h, num_hidden_layers=nl, nonlinearity=act)
    m.load_state_dict(state_dict_of(fx))
    return m.to(device)


@pytest.mark.parametrize("fid", FIXTURE_IDS)
def test_module_forward_backward(golden_dir, fid):
    fx = fixture(golden_dir, fid)
    kind, act, N, d, h, nl = meta(fx)
    x, std, eps = (torch.tensor(fx[k]).cuda() for k in ("x", "std", "eps"))
    m = module_of(fx)
    none, loss = m(x, std, eps=eps)
    assert none is None and loss.dim() == 0
    loss.backward()
    assert abs(float(loss.detach()) - float(fx["loss"])) <= LOSS_TOL * abs(float(fx["loss"]))
    hn = Harness(kind, d, h, nl, act, m.flat_params().detach().cpu())
    xbar = torch.empty_like(x)
    L.call("ardae_dae_perturb", x, std.reshape(-1).contiguous(), eps, N, 1, d, xbar)
    abi_loss, abi_grads, _ = hn.loss_grads(xbar, std, eps)
    assert float(loss.detach()) == float(abi_loss)
    for n, p in m.named_parameters():
        if n == "neglogprob.fc.bias":
            assert p.grad is None
        else:
            assert torch.equal(p.grad.cpu(), abi_grads[n]), n
            assert rel(p.grad.cpu(), fx["g/" + n]) <= TENSOR_TOL
    assert rel(m.glogprob(x).cpu(), fx["glog0"]) <= TENSOR_TOL and rel(m.glogprob(x, std).cpu(), fx["glog"]) <= TENSOR_TOL
    # std=None: zeros, so the loss is mean(eps^2) whatever the network says
    _, loss0 = m(x, eps=eps)
    assert abs(float(loss0) - float((eps ** 2).mean())) <= 1e-6 * float((eps ** 2).mean())
    _, drawn = m(x, std)                                    # the module's own Philox draw
    assert torch.isfinite(drawn) and float(drawn.detach()) != float(loss.detach())


@pytest.mark.parametrize("opt_name", ["torch_rmsprop", "net_rmsprop", "torch_sgd"])
@pytest.mark.parametrize("fid", ["grad_n64_d2_softplus", "res_n96_d8_tanh", "grad_n60_d3_elu", "res_n64_d2_relu1"])
def test_training_cell_follows_the_recorded_trajectory(golden_dir, fid, opt_name):
    """The training cell of notebooks/ardae_toy.ipynb, teacher-forced: parameters reset to the fixture's before each step."""
    fx = fixture(golden_dir, fid)
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
def fresh_module(kind, d, h, nl, act, seed=21):
    m = (net.MLPGradARDAE if kind == "grad" else net.MLPResARDAE)(input_dim=d, h_dim=h, num_hidden_layers=nl, nonlinearity=act)
    m.load_state_dict(init_params(layout.dae_spec(kind, d, h, nl), seed))
    return m.cuda()


@pytest.mark.parametrize("optimizer", ["rmsprop", "adam", "sgd", "amsgrad"])
@pytest.mark.parametrize("kind,B,ns,d,h,nl,act", [("grad", 256, 10, 2, 128, 3, "softplus"), ("res", 64, 10, 2, 64, 3, "softplus"), ("grad", 30, 10, 3, 100, 2, "elu")])
def test_engine_replay_equals_eager(kind, B, ns, d, h, nl, act, optimizer):
    cfg = net.ScoreConfig(delta=1.0, nsigma=ns, lr=1e-3, optimizer=optimizer)
    xs = [torch.randn(B, d, generator=torch.Generator().manual_seed(s)).cuda() for s in range(8)]
    runs = []
    for graph in (True, False):
        net.manual_seed(77)
        eng = net.ArdaeScoreEngine(fresh_module(kind, d, h, nl, act), cfg, B, graph=graph)
        losses = []
        for x in xs:
            eng.step(x)
            losses.append(eng.loss.clone())
        torch.cuda.synchronize()
        assert (eng._graph is not None) == graph
        runs.append((eng.dae.flat_params().clone(), [b.clone() for b in eng.opt.buffers()], torch.cat(losses), eng.state.clone(), eng.sigma.clone()))
    (p1, o1, l1, s1, g1), (p2, o2, l2, s2, g2) = runs
    assert torch.equal(p1, p2) and torch.equal(l1, l2) and torch.equal(s1, s2) and torch.equal(g1, g2)
    assert len(o1) == len(o2) and all(torch.equal(a, b) for a, b in zip(o1, o2))
    assert torch.isfinite(l1).all() and len(set(l1.tolist())) == 8          # fresh noise every step
    assert int(s1[0]) == 16 * 9 and int(s1[1]) == 9                          # the block describes the coming step


@pytest.mark.parametrize("kind", ["grad", "res"])
def test_engine_with_injected_noise_equals_the_module_path(kind):
    B, ns, d, h, nl, act = 64, 10, 2, 128, 3, "softplus"
    g = torch.Generator().manual_seed(3)
    x, sigma, eps = torch.randn(B, d, generator=g).cuda(), torch.randn(B * ns, generator=g).cuda(), torch.randn(B * ns, d, generator=g).cuda()
    m = fresh_module(kind, d, h, nl, act)
    rows = x.unsqueeze(1).expand(B, ns, d).contiguous().view(B * ns, d)       # the notebooks' broadcast
    _, loss = m(rows, sigma[:, None], eps=eps)
    loss.backward()
    eng = net.ArdaeScoreEngine(fresh_module(kind, d, h, nl, act), net.ScoreConfig(nsigma=ns, optimizer="sgd", lr=1e-2), B)
    before = eng.dae.flat_params().clone()
    eng.step(x, noise={"sigma": sigma, "eps": eps})
    st = eng.stats()
    assert abs(st["loss"] - float(loss.detach())) <= LOSS_TOL * abs(float(loss.detach()))
    assert abs(st["sigma_abs_mean"] - float(sigma.abs().mean())) <= 1e-6
    grads = split_flat(eng.grads.cpu(), layout.dae_spec(kind, d, h, nl))
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
    eng = net.ArdaeScoreEngine(fresh_module("grad", 2, 64, 3, "softplus"), net.ScoreConfig(nsigma=10), 32)
    with pytest.raises(ValueError, match="batch_size=32"):
        eng.step(torch.zeros(31, 2, device="cuda"))
    with pytest.raises(ValueError, match="batch_size=32"):
        eng.step(torch.zeros(32, 3, device="cuda"))
    with pytest.raises(ValueError, match="contiguous"):
        eng.step(torch.zeros(32, 4, device="cuda")[:, ::2])
    with pytest.raises(ValueError, match="expected a tensor on cuda"):
        eng.step(torch.zeros(32, 2))
    with pytest.raises(ValueError, match="float32"):
        eng.step(torch.zeros(32, 2, device="cuda").double())
    with pytest.raises(ValueError, match="sigma must be"):
        eng.step(torch.zeros(32, 2, device="cuda"), noise={"sigma": torch.zeros(32, device="cuda"), "eps": torch.zeros(320, 2, device="cuda")})
    with pytest.raises(TypeError):
        net.ArdaeScoreEngine(net.MLPGradCARDAE(input_dim=2, context_dim=2, h_dim=16, nonlinearity="softplus").cuda(), net.ScoreConfig(), 32)
    with pytest.raises(NotImplementedError):
        net.ArdaeScoreEngine(fresh_module("grad", 2, 64, 3, "softplus"), net.ScoreConfig(optimizer="lbfgs"), 32)


def test_engine_refuses_noise_on_another_device():
    """Injected noise is validated like a batch: a tensor on the host or on another GPU is refused before anything is launched."""
    B, ns, d = 30, 4, 3
    eng = net.ArdaeScoreEngine(fresh_module("grad", d, 64, 2, "elu"), net.ScoreConfig(nsigma=ns), B)
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
    xs = [torch.randn(B, d, generator=torch.Generator().manual_seed(s)).cuda() for s in range(8)]
    runs, sd = [], None
    for resumed in (False, True):
        net.manual_seed(77)
        eng = net.ArdaeScoreEngine(fresh_module(kind, d, h, nl, act), cfg, B)
        assert eng.fused_front
        losses = []
        for i, x in enumerate(xs):
            if resumed and i == 4:
                sd = eng.state_dict()
                net.manual_seed(1)                                 # the checkpoint, not the process, carries the RNG state
                eng = net.ArdaeScoreEngine(fresh_module(kind, d, h, nl, act, seed=5), cfg, B, graph=True)
                eng.load_state_dict(sd)
                assert eng._graph is None and (eng.step_count, eng.opt.steps) == (4, 4)
            eng.step(x)
            losses.append(eng.loss.clone())
        torch.cuda.synchronize()
        assert eng._graph is not None
        runs.append([eng.dae.flat_params().clone(), eng.state.clone(), eng.sigma.clone(), torch.cat(losses)[4:]] + [b.clone() for b in eng.opt.buffers()])
    assert len(runs[0]) == len(runs[1]) == 4 + len(eng.opt.state_names())
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "the resumed run drifted"
    assert torch.isfinite(runs[0][3]).all() and len(set(runs[0][3].tolist())) == 4
    # a checkpoint assembled from torch objects has no "engine" entry: the block is rebuilt for the coming step, n = 4 steps done
    assert list(sd) == ["dae", "optimizer", "engine"] and [int(st["step"]) for st in sd["optimizer"]["state"].values()] == [4] * len(sd["optimizer"]["state"])
    del sd["engine"]
    new = net.ArdaeScoreEngine(fresh_module(kind, d, h, nl, act, seed=5), cfg, B)
    new.load_state_dict(sd)
    assert new.step_count == 4 and new.state[:2].tolist() == [16 * 5, 5]
    new.step(xs[4])
    assert np.isfinite(new.stats()["loss"]) and new.state[:2].tolist() == [16 * 6, 6]


# ---- 10. quality: device seeds against the reference's seeds ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["grad", "res"])
def test_training_quality_against_the_reference_seeds(golden_dir, kind):
    """The training cell of notebooks/ardae_toy.ipynb on x ~ N(0, I_2) with the notebook's optimiser (torch.optim.Adam over the module's
    parameters); every constant comes from the fixture tools/gen_ardae_golden.py wrote with the reference classes."""
    q = load(os.path.join(golden_dir, "ardae_uncond_quality.npz"))
    B, ns, steps, tail, delta, lr = int(q["B"]), int(q["nsigma"]), int(q["steps"]), int(q["tail"]), float(q["delta"]), float(q["lr"])
    xt = torch.tensor(q["x_t"]).cuda()
    ref_loss, ref_err = q[f"{kind}/loss"], q[f"{kind}/score_err"]
    dev_loss, dev_err = [], []
    for seed in (int(s) for s in q["seeds"]):
        torch.manual_seed(2000 + seed)
        net.manual_seed(2000 + seed)
        m = (net.MLPGradARDAE if kind == "grad" else net.MLPResARDAE)(input_dim=2, h_dim=int(q["h"]), num_hidden_layers=int(q["L"]), nonlinearity=str(q["act"])).cuda()
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
