"""Plain DAE score networks on the device: C ABI kinds 6 / 7, the perturbation, the sigma schedule, the modules and ArdaeScoreEngine
with a DaeConfig (notebooks/dae_toy.ipynb).

Bars: loss 2e-5 relative, every gradient tensor and glogprob 1e-4 relative L2 against the reference's fp32 fixtures - the bars
tests/test_cdae_gpu.py and tests/test_ardae_uncond_gpu.py state.  The float64 oracle is the restatement in tests/test_dae_plain.py, which
that file pins to the reference's fp64 fixtures to 1e-12."""
import os

import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import layout
from test_ardae_uncond import load, rel, state_dict_of
from test_ardae_uncond import score as ar_score
from test_ardae_uncond_gpu import Harness as ArHarness
from test_ardae_uncond_gpu import assert_matches_reference, flat_of, init_params, meta
from test_cdae_gpu import split_flat
from test_dae_plain import KIND_ID, score, std_of

pytestmark = pytest.mark.gpu
LOSS_TOL, TENSOR_TOL = 2e-5, 1e-4
FIXTURE_IDS = [f"{k}_{c}" for k in ("grad", "res") for c in ("n60_d3_elu", "n64_d2_relu1", "n64_d2_softplus", "n64_d2_swish", "n96_d8_tanh")]
STRIDE = 16


def fixture(golden_dir, fid):
    return load(os.path.join(golden_dir, f"dae_plain_{fid}.npz"))


def sigma_rows(std, N):
    """The per-row [N] array the ABI takes for the reference's float or [N, 1] std."""
    return std.reshape(-1) if torch.is_tensor(std) else torch.full((N,), float(std))


def guarded(rows, cols=None):
    """A NaN-filled buffer of rows + 1 rows: the first `rows` are the output, the last one must stay NaN."""
    full = torch.full((rows + 1,) if cols is None else (rows + 1, cols), float("nan"), device="cuda")
    return full, full[:rows]


def dae_block(t, smax, smin, ann, lr=5e-3, beta1=0.9):
    """A DAE state block that describes step t (t >= 1): written for t - 1, advanced once."""
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    st[0], st[1] = STRIDE * (t - 1), t - 1
    L.call("ardae_dae_state_advance", st, STRIDE, lr, beta1, 0.999, smax, smin, ann)
    return st


class Harness(ArHarness):
    """The C ABI for one plain DAE (kind 6 / 7)."""

    def __init__(self, kind, d, h, nl, act, flat_params):
        self.kind, self.d_in, self.h = kind, d, h
        self.spec = layout.dae_plain_spec(kind, d, h, nl)
        self.d = L.CdaeDesc(KIND_ID[kind], d, 0, h, nl, L.ACT[act])
        assert L.query("ardae_cdae_param_floats", self.d) == flat_params.numel()
        self.params = flat_params.cuda()
        self.packed = torch.empty(L.query("ardae_cdae_packed_floats", self.d), device="cuda")
        L.call("ardae_cdae_pack", self.d, self.params, self.packed)

    def score(self, x, sigma=None):
        N = x.size(0)
        ws = torch.empty(L.query("ardae_cdae_workspace_floats", self.d, N, 1, 0), device="cuda")
        out = torch.empty(N, self.d_in, device="cuda")
        L.call("ardae_cdae_score", self.d, self.params, self.packed, x.contiguous().cuda(), None if sigma is None else sigma.reshape(-1).contiguous().cuda(), None,
               N, 1, ws, ws.numel(), out)
        torch.cuda.synchronize()
        return out.cpu()

    def front(self, x, B, ns, sigma, dae_state, seed, first_row=0, state=None):
        """-> loss, grads, xbar, sigma_out, eps, h_1 of the update's three launches; the three outputs carry a NaN guard row"""
        N = B * ns
        (xb_all, xbar), (sg_all, sg), (ep_all, eps) = guarded(N, self.d_in), guarded(N), guarded(N, self.d_in)
        L.call("ardae_philox_normal_at", eps, N * self.d_in, seed, 4, state, first_row * self.d_in)
        L.call("ardae_dae_noise_perturb", x, eps, B, ns, self.d_in, sigma, dae_state, xbar, sg)
        loss, grads, _ = self.loss_grads(xbar, sg, eps)
        for full in (xb_all, sg_all, ep_all):
            assert torch.isnan(full[N:]).all() and not torch.isnan(full[:N]).any()
        return loss, grads, xbar, sg, eps, self.ws[:N * self.h].clone()


def with_zero_sigma_column(kind, p, d, h, nl):
    """The AR-DAE network (kind 2 / 3) that computes the plain network's function: its parameters with a zero sigma column."""
    first = ("neglogprob." if kind == "grad" else "main.") + "layers.0.weight"
    q = dict(p)
    q[first] = torch.cat([p[first], torch.zeros(h, 1)], 1)
    return q, first


# ---- 1. C ABI against every fixture ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FIXTURE_IDS)
def test_abi_matches_the_reference_fixtures(golden_dir, fid):
    fx = fixture(golden_dir, fid)
    kind, act, N, d, h, nl = meta(fx)
    x, eps, std = torch.tensor(fx["x"]), torch.tensor(fx["eps"]), std_of(fx)
    s = sigma_rows(std, N)
    hn = Harness(kind, d, h, nl, act, flat_of(state_dict_of(fx), layout.dae_plain_spec(kind, d, h, nl)))
    xbar = x + std * eps                                        # add_gaussian_noise as the reference evaluates it
    loss, grads, sc = hn.loss_grads(xbar, s, eps)
    print(f"{fid}: loss {float(loss):.7f} (reference {float(fx['loss']):.7f})")
    assert abs(float(loss) - float(fx["loss"])) <= LOSS_TOL * abs(float(fx["loss"]))
    assert_matches_reference(grads, fx, "g", fid)
    assert [n for n, g in grads.items() if torch.isnan(g).any()] == (["neglogprob.fc.bias"] if kind == "grad" else [])       # and nothing else
    # score: the same bits whatever sigma is passed
    glog = hn.score(x)
    assert rel(glog, fx["glog"]) <= TENSOR_TOL
    assert torch.equal(glog, hn.score(x, s)) and torch.equal(glog, hn.score(x, torch.zeros(N))) and torch.equal(glog, hn.score(x, torch.full((N,), float("nan"))))
    # N = B S in any factorisation: the same bits
    if N % 4 == 0:
        loss2, grads2, sc2 = hn.loss_grads(xbar, s, eps, N // 4, 4)
        assert torch.equal(loss, loss2) and torch.equal(sc, sc2) and all(torch.equal(torch.nan_to_num(grads[n]), torch.nan_to_num(grads2[n])) for n in grads)


# ---- 2. the AR-DAE kinds with a zero sigma column are the same function: existing code as the oracle -------------------------------
ORACLE_SHAPES = [(60, 3, 100, 2, "elu"), (64, 2, 64, 3, "softplus"), (300, 8, 256, 3, "softplus"), (1000, 1, 64, 4, "tanh")]


@pytest.mark.parametrize("kind", ["grad", "res"])
@pytest.mark.parametrize("N,d,h,nl,act", ORACLE_SHAPES, ids=[f"n{s[0]}_d{s[1]}_h{s[2]}" for s in ORACLE_SHAPES])
def test_plain_kinds_equal_the_ardae_kinds_with_a_zero_sigma_column(kind, N, d, h, nl, act):
    g = torch.Generator().manual_seed(N + d)
    x, sigma, eps = torch.randn(N, d, generator=g), 0.3 * torch.randn(N, generator=g), torch.randn(N, d, generator=g)
    spec = layout.dae_plain_spec(kind, d, h, nl)
    p = init_params(spec, 4)
    q, first = with_zero_sigma_column(kind, p, d, h, nl)
    xbar = torch.addcmul(x, sigma[:, None], eps)
    hn = Harness(kind, d, h, nl, act, flat_of(p, spec))
    loss, grads, sc = hn.loss_grads(xbar, sigma, eps)
    ar = ArHarness(kind, d, h, nl, act, flat_of(q, layout.dae_spec(kind, d, h, nl)))      # fma(sigma, 0, v) = v
    loss_o, grads_o, sc_o = ar.loss_grads(xbar, sigma, eps)
    grads_o[first] = grads_o[first][:, :d]                                                  # all tensors but the sigma column
    assert abs(float(loss) - float(loss_o)) <= LOSS_TOL * abs(float(loss_o))
    same, total = int((sc == sc_o).sum()), sc.numel()
    assert rel(sc, sc_o) <= TENSOR_TOL
    for n in grads:
        if torch.isnan(grads_o[n]).all():
            assert torch.isnan(grads[n]).all() and n == "neglogprob.fc.bias"
            continue
        assert not torch.isnan(grads[n]).any(), n
        assert rel(grads[n], grads_o[n]) <= TENSOR_TOL, (n, rel(grads[n], grads_o[n]))
        same, total = same + int((grads[n] == grads_o[n]).sum()), total + grads[n].numel()
    assert rel(hn.score(x), ar.glogprob(x, sigma)) <= TENSOR_TOL
    print(f"{kind} N={N} d={d} h={h} L={nl} {act}: {100 * same / total:.3f} % of the score and gradient elements bit-identical, loss {float(loss):.7f} / {float(loss_o):.7f}")


# ---- 3. against float64 at sizes a user runs, with the AR-DAE sibling as the yardstick ---------------------------------------------
USER_SHAPES = [(2560, 2, 128, 3, "softplus"), (300, 3, 100, 2, "elu"), (1000, 1, 64, 4, "tanh")]


def sibling_error(kind, d, h, nl, act, xbar, sigma, eps):
    """E_sibling: the AR-DAE network of the same widths (kind 2 / 3) through ardae_cdae_loss_grads against float64, worst relative L2
    over its gradient tensors."""
    spec = layout.dae_spec(kind, d, h, nl)
    p = init_params(spec, 11)
    pp = {k: v.double().requires_grad_(True) for k, v in p.items()}
    xb = xbar.double().requires_grad_(True)
    loss = torch.nn.functional.mse_loss(sigma.double() * ar_score(kind, pp, act, xb, sigma.double(), create_graph=True), -eps.double())
    g64 = dict(zip(pp, torch.autograd.grad(loss, list(pp.values()), allow_unused=True)))
    _, grads, _ = ArHarness(kind, d, h, nl, act, flat_of(p, spec)).loss_grads(xbar, sigma, eps)
    return max(rel(grads[n], g64[n]) for n in grads if g64[n] is not None)


@pytest.mark.parametrize("kind", ["grad", "res"])
@pytest.mark.parametrize("N,d,h,nl,act", USER_SHAPES, ids=[f"n{s[0]}_d{s[1]}_h{s[2]}" for s in USER_SHAPES])
def test_gradients_against_float64_at_user_sizes(kind, N, d, h, nl, act):
    """e <= max(2 E_sibling, 3 e_ref32 + 2e-6) per gradient tensor (e_ref32: the fp32 restatement's own distance to float64)."""
    g = torch.Generator().manual_seed(N + d)
    x, sigma, eps = torch.randn(N, d, generator=g), 0.1 * torch.randn(N, 1, generator=g), torch.randn(N, d, generator=g)
    spec = layout.dae_plain_spec(kind, d, h, nl)
    p = init_params(spec, 3)
    xbar = torch.addcmul(x, sigma, eps)

    def oracle(dtype):                          # the restatement's loss on the SAME fp32 xbar: mse(sigma g(xbar), -eps)
        pp = {k: v.to(dtype).requires_grad_(True) for k, v in p.items()}
        xb = xbar.to(dtype).requires_grad_(True)
        loss = torch.nn.functional.mse_loss(sigma.to(dtype) * score(kind, pp, act, xb, create_graph=True), -eps.to(dtype))
        return loss.detach(), dict(zip(pp, torch.autograd.grad(loss, list(pp.values()), allow_unused=True)))
    loss64, g64 = oracle(torch.float64)
    loss32, g32 = oracle(torch.float32)
    loss, grads, _ = Harness(kind, d, h, nl, act, flat_of(p, spec)).loss_grads(xbar, sigma, eps)
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
    spec = layout.dae_plain_spec(kind, d, h, nl)
    hn = Harness(kind, d, h, nl, act, flat_of(init_params(spec, 9), spec))
    x = torch.randn(B, d, generator=torch.Generator().manual_seed(B)).cuda()
    seed, N = 1234, B * ns
    block = dae_block(3, 1.0, 0.1, 4)                        # sigma of i = 2, Philox base offset 3 * STRIDE
    s = float(np.float32(net.dae_sigma(1.0, 0.1, 4, 2)))
    outs = {}
    for form, sig, dst in (("value", s, None), ("block", 0.0, block)):
        for st in (None, block):
            loss, grads, xbar, sg, eps, h1 = hn.front(x, B, ns, sig, dst, seed, 0, st)
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
def module_of(fx, device="cuda"):
    kind, act, N, d, h, nl = meta(fx)
    m = (net.MLPGradDAE if kind == "grad" else net.MLPResDAE)(input_dim=d, h_dim=h, num_hidden_layers=nl, nonlinearity=act)
    m.load_state_dict(state_dict_of(fx))
    return m.to(device)


@pytest.mark.parametrize("fid", FIXTURE_IDS)
def test_module_forward_backward(golden_dir, fid):
    fx = fixture(golden_dir, fid)
    kind, act, N, d, h, nl = meta(fx)
    x, eps, std = torch.tensor(fx["x"]).cuda(), torch.tensor(fx["eps"]).cuda(), std_of(fx)
    std = std.cuda() if torch.is_tensor(std) else std
    m = module_of(fx)
    none, loss = m(x, std, eps=eps)
    assert none is None and loss.dim() == 0
    loss.backward()
    assert abs(float(loss.detach()) - float(fx["loss"])) <= LOSS_TOL * abs(float(fx["loss"]))
    hn = Harness(kind, d, h, nl, act, m.flat_params().detach().cpu())
    s = sigma_rows(std, N).cuda()
    xbar = torch.empty_like(x)
    L.call("ardae_dae_perturb", x, s, eps, N, 1, d, xbar)
    abi_loss, abi_grads, _ = hn.loss_grads(xbar, s, eps)
    assert float(loss.detach()) == float(abi_loss)
    for n, p in m.named_parameters():
        if n == "neglogprob.fc.bias":
            assert p.grad is None
        else:
            assert torch.equal(p.grad.cpu(), abi_grads[n]), n
            assert rel(p.grad.cpu(), fx["g/" + n]) <= TENSOR_TOL
    glog = m.glogprob(x)
    assert rel(glog.cpu(), fx["glog"]) <= TENSOR_TOL and torch.equal(glog, m.glogprob(x, 0.7)) and torch.equal(glog, m.glogprob(x, torch.ones(N, 1, device="cuda")))
    # std=None: self.std
    m.std = 0.37
    assert float(m(x, eps=eps)[1].detach()) == float(m(x, 0.37, eps=eps)[1].detach()) != float(loss.detach())
    assert float(m(x, torch.tensor(0.37, device="cuda"), eps=eps)[1].detach()) == float(m(x, torch.full((N, 1), 0.37, device="cuda"), eps=eps)[1].detach()) == float(m(x, eps=eps)[1].detach())
    # eps=None: the module's own Philox draw, a fresh one per call
    a, b = float(m(x, std)[1].detach()), float(m(x, std)[1].detach())
    assert np.isfinite(a) and np.isfinite(b) and a != b and a != float(loss.detach())


# ---- 8. engine ---------------------------------------------------------------------------------------------------------------------
def fresh_module(kind, d, h, nl, act, seed=21):
    m = (net.MLPGradDAE if kind == "grad" else net.MLPResDAE)(input_dim=d, h_dim=h, num_hidden_layers=nl, nonlinearity=act)
    m.load_state_dict(init_params(layout.dae_plain_spec(kind, d, h, nl), seed))
    return m.cuda()


def sigma32(cfg, i):
    return float(np.float32(net.dae_sigma(cfg.sigma_max, cfg.sigma_min, cfg.sigma_annealing, i)))


@pytest.mark.parametrize("kind,B,ns,d,h,nl,act,optimizer", [("grad", 30, 4, 3, 64, 2, "elu", "adam_torch"), ("res", 16, 4, 2, 64, 3, "softplus", "adam_torch"),
                                                             ("grad", 30, 10, 3, 100, 2, "elu", "adam_torch"), ("res", 256, 10, 2, 128, 3, "softplus", "rmsprop")])
def test_engine_replay_equals_eager(kind, B, ns, d, h, nl, act, optimizer):
    cfg = net.DaeConfig(sigma_max=1.0, sigma_min=0.1, sigma_annealing=4, nsigma=ns, optimizer=optimizer, momentum=0.5)
    xs = [torch.randn(B, d, generator=torch.Generator().manual_seed(s)).cuda() for s in range(6)]
    runs = []
    for graph in (True, False):
        net.manual_seed(77)
        eng = net.ArdaeScoreEngine(fresh_module(kind, d, h, nl, act), cfg, B, graph=graph)
        assert not eng.fused_front
        trace = []
        for i, x in enumerate(xs):
            eng.step(x)
            trace += [eng.dae.flat_params().clone(), eng.loss.clone(), eng.sigma.clone()] + [b.clone() for b in eng.opt.buffers()]
            assert eng.stats()["sigma"] == sigma32(cfg, i) and torch.equal(eng.sigma, torch.full((B * ns,), sigma32(cfg, i), device="cuda"))
        torch.cuda.synchronize()
        assert (eng._graph is not None) == graph
        runs.append(trace + [eng.state.clone()])
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(a, b) for a, b in zip(*runs)), "replayed != eager"
    losses = torch.cat(runs[0][1::3 + len(eng.opt.buffers())][:6])
    assert torch.isfinite(losses).all() and len(set(losses.tolist())) == 6
    s = runs[0][-1]
    assert int(s[0]) == STRIDE * 7 and int(s[1]) == 7                          # the block describes the coming step
    with pytest.raises(ValueError, match="computes sigma on the device"):
        eng.step(xs[0], sigma=0.5)
    assert eng.step_count == 6


@pytest.mark.parametrize("kind", ["grad", "res"])
def test_engine_follows_the_recorded_trajectory(golden_dir, kind):
    """The notebook's loop on the fixture's x / eps: every parameter after every step against the reference's fp32 run, and no further
    from its float64 run than max(2 x the fp32 reference's own distance, 2e-6)."""
    fx = load(os.path.join(golden_dir, f"dae_plain_traj_{kind}.npz"))
    c = {k[4:]: v for k, v in fx.items() if k.startswith("cfg/")}
    B, ns, d, h, nl, act, steps = int(c["B"]), int(c["nsigma"]), int(c["d"]), int(c["h"]), int(c["L"]), str(c["act"]), int(c["steps"])
    cfg = net.DaeConfig(sigma_max=float(c["sigma_max"]), sigma_min=float(c["sigma_min"]), sigma_annealing=int(c["sigma_annealing"]), nsigma=ns, lr=float(c["lr"]))
    m = (net.MLPGradDAE if kind == "grad" else net.MLPResDAE)(input_dim=d, h_dim=h, num_hidden_layers=nl, nonlinearity=act)
    m.load_state_dict(state_dict_of(fx))
    eng = net.ArdaeScoreEngine(m.cuda(), cfg, B)
    bad = []
    for s in range(steps):
        eng.step(torch.tensor(fx[f"{s}/x"]).cuda(), noise={"eps": torch.tensor(fx[f"{s}/eps"]).cuda()})
        st = eng.stats()
        assert st["sigma"] == float(np.float32(float(fx[f"{s}/sigma"])))
        assert abs(st["loss"] - float(fx[f"{s}/loss"])) <= LOSS_TOL * abs(float(fx[f"{s}/loss"])), (s, st["loss"])
        for n, p in eng.dae.named_parameters():
            p32, p64 = fx[f"{s}/p/{n}"], fx[f"{s}/p_f64/{n}"]
            e32, e64, ref64 = rel(p.detach().cpu(), p32), rel(p.detach().cpu(), p64), rel(p32, p64)
            print(f"{kind} step {s} {n}: to fp32 reference {e32:.2e}, to float64 {e64:.2e} (fp32 reference to float64 {ref64:.2e})")
            if e32 > TENSOR_TOL or e64 > max(2 * ref64, 2e-6):
                bad.append((s, n, e32, e64, ref64))
    assert not bad, bad


@pytest.mark.parametrize("kind", ["grad", "res"])
def test_engine_equals_the_drop_in_module_route(kind):
    """The same six steps through ArdaeScoreEngine and through the module + torch.optim.Adam with a host-computed sigma."""
    B, ns, d, h, nl, act = 30, 4, 3, 64, 2, "elu"
    cfg = net.DaeConfig(sigma_max=1.0, sigma_min=0.1, sigma_annealing=4, nsigma=ns)
    g = torch.Generator().manual_seed(5)
    eng = net.ArdaeScoreEngine(fresh_module(kind, d, h, nl, act), cfg, B)
    m = fresh_module(kind, d, h, nl, act)
    opt = torch.optim.Adam(m.parameters(), lr=cfg.lr)
    for i in range(6):
        x, eps = (0.5 * torch.randn(B, d, generator=g)).cuda(), torch.randn(B * ns, d, generator=g).cuda()
        eng.step(x, noise={"eps": eps})
        opt.zero_grad()
        _, loss = m(x.unsqueeze(1).expand(B, ns, d).contiguous().view(B * ns, d), net.dae_sigma(1.0, 0.1, 4, i), eps=eps)
        loss.backward()
        opt.step()
        assert abs(eng.stats()["loss"] - float(loss.detach())) <= LOSS_TOL * abs(float(loss.detach())), i
        for (n, p), (_, q) in zip(eng.dae.named_parameters(), m.named_parameters()):
            assert rel(p.detach().cpu(), q.detach().cpu()) <= TENSOR_TOL, (i, n, rel(p.detach().cpu(), q.detach().cpu()))
    # the two routes' checkpoints are interchangeable: torch.optim.Adam's state loads into the engine
    eng.load_state_dict({"dae": m.state_dict(), "optimizer": opt.state_dict()})
    assert eng.step_count == 6 and eng.state[:2].tolist() == [STRIDE * 7, 7]
    assert eng.state[3:].view(torch.float32)[0].item() == sigma32(cfg, 6)
    pts = torch.randn(100, d, generator=g).cuda()
    assert torch.equal(eng.score(pts), m.glogprob(pts)) and torch.equal(eng.score(pts), eng.score(pts, torch.rand(100, generator=g).cuda()))


@pytest.mark.parametrize("kind,optimizer", [("grad", "adam_torch"), ("res", "adam_torch"), ("grad", "amsgrad")])
def test_dae_engine_resumes_bit_identically_across_the_end_of_the_ramp(kind, optimizer):
    """state_dict() after step 2 into a fresh engine under another library seed: steps 3 - 8 (the ramp of 4 steps ends among them; eager,
    eager, captured, replayed there) leave what the uninterrupted run leaves."""
    B, ns, d, h, nl, act = 30, 4, 3, 64, 2, "elu"
    cfg = net.DaeConfig(sigma_max=1.0, sigma_min=0.1, sigma_annealing=4, nsigma=ns, optimizer=optimizer, beta1=0.5)
    xs = [torch.randn(B, d, generator=torch.Generator().manual_seed(s)).cuda() for s in range(8)]
    runs, sd = [], None
    for resumed in (False, True):
        net.manual_seed(77)
        eng = net.ArdaeScoreEngine(fresh_module(kind, d, h, nl, act), cfg, B)
        losses = []
        for i, x in enumerate(xs):
            if resumed and i == 2:
                sd = eng.state_dict()
                net.manual_seed(1)                                 # the checkpoint, not the process, carries the RNG state
                eng = net.ArdaeScoreEngine(fresh_module(kind, d, h, nl, act, seed=5), cfg, B, graph=True)
                eng.load_state_dict(sd)
                assert eng._graph is None and (eng.step_count, eng.opt.steps) == (2, 2)
            eng.step(x)
            assert eng.stats()["sigma"] == sigma32(cfg, i)
            losses.append(eng.loss.clone())
        torch.cuda.synchronize()
        assert eng._graph is not None
        runs.append([eng.dae.flat_params().clone(), eng.state.clone(), eng.sigma.clone(), torch.cat(losses)[2:]] + [b.clone() for b in eng.opt.buffers()])
    assert len(runs[0]) == len(runs[1]) == 4 + len(eng.opt.state_names())
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "the resumed run drifted"
    assert torch.isfinite(runs[0][3]).all() and len(set(runs[0][3].tolist())) == 6
    # a checkpoint written under another schedule resumes at THIS engine's value: bytes 24..27 are recomputed from t
    other = net.DaeConfig(sigma_max=5.0, sigma_min=0.05, sigma_annealing=4000, nsigma=ns, optimizer=optimizer, beta1=0.5)
    new = net.ArdaeScoreEngine(fresh_module(kind, d, h, nl, act, seed=5), other, B)
    new.load_state_dict(sd)
    assert torch.equal(new.state[:3].cpu(), sd["engine"]["step_state"][:3]) and new.state[3:].view(torch.float32)[0].item() == sigma32(other, 2)
    new.step(xs[2])
    assert new.stats()["sigma"] == sigma32(other, 2) and torch.equal(new.sigma, torch.full((B * ns,), sigma32(other, 2), device="cuda"))


def test_engine_refuses_mismatched_configs_and_bad_batches():
    with pytest.raises(TypeError, match="(?s)MLPGradDAE.*DaeConfig.*ScoreConfig"):
        net.ArdaeScoreEngine(fresh_module("grad", 2, 64, 3, "softplus"), net.ScoreConfig(), 32)
    from test_ardae_uncond_gpu import fresh_module as fresh_ardae
    with pytest.raises(TypeError, match="(?s)MLPResARDAE.*ScoreConfig.*DaeConfig"):
        net.ArdaeScoreEngine(fresh_ardae("res", 2, 64, 3, "softplus"), net.DaeConfig(), 32)
    eng = net.ArdaeScoreEngine(fresh_module("grad", 2, 64, 3, "softplus"), net.DaeConfig(), 32)
    with pytest.raises(ValueError, match="batch_size=32"):
        eng.step(torch.zeros(31, 2, device="cuda"))
    with pytest.raises(ValueError, match="eps must be"):
        eng.step(torch.zeros(32, 2, device="cuda"), noise={"eps": torch.zeros(32, 2, device="cuda")})
    with pytest.raises(ValueError, match="eps must be"):
        eng.step(torch.zeros(32, 2, device="cuda"), noise={"eps": torch.zeros(320, 2)})
    assert eng.step_count == 0 and eng.input_buffer().shape == (32, 2)
    with pytest.raises(ValueError, match="inject them through noise"):
        net.ArdaeScoreEngine(fresh_ardae("grad", 2, 64, 3, "softplus"), net.ScoreConfig(), 32).step(torch.zeros(32, 2, device="cuda"), sigma=0.5)


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
    eng = net.ArdaeScoreEngine(fresh_module(kind, d, h, nl, act), cfg, B)
    m = fresh_module(kind, d, h, nl, act)
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
