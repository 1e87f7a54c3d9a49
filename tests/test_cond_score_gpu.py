"""Plain conditional DAE score networks on the device (C ABI kinds 10 / 11, the two one-noise-level perturbation kernels, the modules) and
ArdaeCondScoreEngine for both conditional families.

Bars: loss 2e-5 relative, every gradient tensor and glogprob 1e-4 relative L2 against the reference's fp32 fixtures - the bars
tests/test_cdae_gpu.py and tests/test_dae_plain_gpu.py state.  The float64 oracle is the restatement in tests/test_cond_score.py, which that
file pins to the reference's fp64 fixtures to 1e-12."""
import os

import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import layout
from oracle import ardae_oracle as O
from test_ardae_uncond import load, rel, state_dict_of
from test_ardae_uncond_gpu import assert_matches_reference, flat_of, init_params
from test_cdae_gpu import split_flat
from test_cond_score import CLS, KIND_ID, build, dims, inputs_of, score, std_of

pytestmark = pytest.mark.gpu
LOSS_TOL, TENSOR_TOL = 2e-5, 1e-4
FIXTURE_IDS = [f"{k}_{c}" for k in ("grad", "res") for c in ("b4_s16_d2_softplus", "b5_s12_d3_elu", "b6_s16_d8_tanh", "b8_s8_d2_relu1", "b4_s16_d2_swish")]
STRIDE = 16


def fixture(golden_dir, fid):
    return load(os.path.join(golden_dir, f"cdae_plain_{fid}.npz"))


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


class Harness:
    """The C ABI for one conditional network: plain (kind 10 / 11) or, plain=False, its AR-DAE sibling (kind 0 / 1)."""

    def __init__(self, kind, d, c, h, nl, act, flat_params, plain=True):
        self.kind, self.d_in, self.c, self.h = kind, d, c, h
        self.spec = (layout.cdae_plain_spec if plain else layout.cdae_spec)(kind, d, c, h, nl)
        self.d = L.CdaeDesc(KIND_ID[kind] - (0 if plain else 10), d, c, h, nl, L.ACT[act])
        assert L.query("ardae_cdae_param_floats", self.d) == flat_params.numel()
        self.params = flat_params.cuda()
        self.packed = torch.empty(L.query("ardae_cdae_packed_floats", self.d), device="cuda")
        L.call("ardae_cdae_pack", self.d, self.params, self.packed)

    def loss_grads(self, xbar, sigma, eps, ctx, B, S):
        assert B * S == xbar.size(0)
        ws = torch.empty(L.query("ardae_cdae_workspace_floats", self.d, B, S, 1), device="cuda")
        loss, grads = torch.zeros(1, device="cuda"), torch.full_like(self.params, float("nan"))
        sc = torch.empty(B * S, self.d_in, device="cuda")
        xbar, sigma, eps, ctx = (t.contiguous().cuda() for t in (xbar, sigma.reshape(-1), eps, ctx.reshape(B, self.c)))
        L.call("ardae_cdae_loss_grads", self.d, self.params, self.packed, xbar, sigma, eps, ctx, B, S, ws, ws.numel(), loss, grads, sc)
        torch.cuda.synchronize()
        return loss.cpu(), split_flat(grads.cpu(), self.spec), sc.cpu()

    def score(self, x, ctx, B, S, sigma=None):
        ws = torch.empty(L.query("ardae_cdae_workspace_floats", self.d, B, S, 0), device="cuda")
        out = torch.empty(B * S, self.d_in, device="cuda")
        x, ctx = x.contiguous().cuda(), ctx.reshape(B, self.c).contiguous().cuda()
        L.call("ardae_cdae_score", self.d, self.params, self.packed, x, None if sigma is None else sigma.reshape(-1).contiguous().cuda(), ctx, B, S, ws,
               ws.numel(), out)
        torch.cuda.synchronize()
        return out.cpu()


def first_energy_weight(kind):
    return ("neglogprob." if kind == "grad" else "dae.") + "layers.0.weight"


# ---- 1. C ABI against every fixture ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FIXTURE_IDS)
def test_abi_matches_the_reference_fixtures(golden_dir, fid):
    fx = fixture(golden_dir, fid)
    (B, S, d, c, h, nl), kind, act = dims(fx), str(fx["kind"]), str(fx["act"])
    N = B * S
    x, ctx, eps = inputs_of(fx, torch.float32)
    std = std_of(fx)
    s = sigma_rows(std, N)
    hn = Harness(kind, d, c, h, nl, act, flat_of(state_dict_of(fx), layout.cdae_plain_spec(kind, d, c, h, nl)))
    xbar = x + std * eps                                        # add_gaussian_noise as the reference evaluates it
    loss, grads, sc = hn.loss_grads(xbar, s, eps, ctx, B, S)
    print(f"{fid}: loss {float(loss):.7f} (reference {float(fx['loss']):.7f})")
    assert abs(float(loss) - float(fx["loss"])) <= LOSS_TOL * abs(float(fx["loss"]))
    assert_matches_reference(grads, fx, "g", fid)
    assert [n for n, g in grads.items() if torch.isnan(g).any()] == (["neglogprob.fc.bias"] if kind == "grad" else [])       # the prefill survives there only
    # score: the same bits whatever sigma is passed
    glog = hn.score(x, ctx, B, S)
    assert rel(glog, fx["glog"].reshape(N, d)) <= TENSOR_TOL
    assert torch.equal(glog, hn.score(x, ctx, B, S, s)) and torch.equal(glog, hn.score(x, ctx, B, S, torch.zeros(N)))
    assert torch.equal(glog, hn.score(x, ctx, B, S, torch.full((N,), float("nan"))))


# ---- 2. the AR-DAE kinds with a zero sigma column are the same function: existing code as the oracle -------------------------------
ORACLE_SHAPES = [(1, 1, 2, 2, 64, 1, "tanh"), (5, 20, 3, 5, 100, 2, "elu"), (4, 16, 2, 2, 64, 3, "softplus"), (8, 40, 8, 24, 256, 3, "softplus"),
                 (64, 1, 32, 32, 256, 3, "softplus")]


@pytest.mark.parametrize("kind", ["grad", "res"])
@pytest.mark.parametrize("B,S,d,c,h,nl,act", ORACLE_SHAPES, ids=[f"b{s[0]}_s{s[1]}_d{s[2]}_h{s[4]}" for s in ORACLE_SHAPES])
def test_plain_kinds_equal_the_ardae_kinds_with_a_zero_sigma_column(kind, B, S, d, c, h, nl, act):
    N = B * S
    g = torch.Generator().manual_seed(N + d)
    x, sigma, eps, ctx = torch.randn(N, d, generator=g), 0.3 * torch.randn(N, generator=g), torch.randn(N, d, generator=g), torch.randn(B, c, generator=g)
    spec = layout.cdae_plain_spec(kind, d, c, h, nl)
    p = init_params(spec, 4)
    first = first_energy_weight(kind)
    q = dict(p)
    q[first] = torch.cat([p[first], torch.zeros(h, 1)], 1)                                  # fma(sigma, 0, v) = v
    xbar = torch.addcmul(x, sigma[:, None], eps)
    hn = Harness(kind, d, c, h, nl, act, flat_of(p, spec))
    ar = Harness(kind, d, c, h, nl, act, flat_of(q, layout.cdae_spec(kind, d, c, h, nl)), plain=False)
    loss, grads, sc = hn.loss_grads(xbar, sigma, eps, ctx, B, S)
    loss_o, grads_o, sc_o = ar.loss_grads(xbar, sigma, eps, ctx, B, S)
    grads_o[first] = grads_o[first][:, :2 * h]                                              # all tensors but the sigma column
    assert abs(float(loss) - float(loss_o)) <= LOSS_TOL * abs(float(loss_o))
    assert rel(sc, sc_o) <= TENSOR_TOL
    same, total = int((sc == sc_o).sum()), sc.numel()
    for n in grads:
        if torch.isnan(grads_o[n]).all():
            assert torch.isnan(grads[n]).all() and n == "neglogprob.fc.bias"
            continue
        assert not torch.isnan(grads[n]).any(), n
        assert rel(grads[n], grads_o[n]) <= TENSOR_TOL, (n, rel(grads[n], grads_o[n]))
        same, total = same + int((grads[n] == grads_o[n]).sum()), total + grads[n].numel()
    assert rel(hn.score(x, ctx, B, S), ar.score(x, ctx, B, S, sigma)) <= TENSOR_TOL          # (N == B: kind 10 walks kind 0's one-launch chain)
    print(f"{kind} B={B} S={S} d={d} h={h} L={nl} {act}: {100 * same / total:.3f} % of the score and gradient elements bit-identical, loss {float(loss):.7f} / {float(loss_o):.7f}")


# ---- 3. against float64, with the AR-DAE sibling as the yardstick ------------------------------------------------------------------
F64_SHAPES = [(16, 64, 32, 32, 256, 3, "softplus"), (10, 30, 3, 5, 100, 2, "elu")]


def oracle_grads(kind, p, act, xbar, sigma, eps, ctx, S, dtype, with_sigma_input):
    """The restatement's loss on the SAME fp32 xbar, mse(sigma g(xbar), -eps), and its gradients, in `dtype`"""
    pp = {k: v.to(dtype).requires_grad_(True) for k, v in p.items()}
    xb = xbar.to(dtype).requires_grad_(True)
    sg = sigma.to(dtype).reshape(-1, 1)
    g = score(kind, pp, act, xb, ctx.to(dtype), S, create_graph=True, sigma=sg if with_sigma_input else None)
    loss = torch.nn.functional.mse_loss(sg * g, -eps.to(dtype))
    return loss.detach(), dict(zip(pp, torch.autograd.grad(loss, list(pp.values()), allow_unused=True)))


@pytest.mark.parametrize("kind", ["grad", "res"])
@pytest.mark.parametrize("B,S,d,c,h,nl,act", F64_SHAPES, ids=[f"b{s[0]}_s{s[1]}_d{s[2]}_h{s[4]}" for s in F64_SHAPES])
def test_gradients_against_float64(kind, B, S, d, c, h, nl, act):
    """e <= max(2 E_sibling, 3 e_ref32 + 2e-6) per gradient tensor (e_ref32: the fp32 restatement's own distance to float64; E_sibling: the
    kind 0 / 1 network of the same widths through the same entry point against float64, worst tensor)."""
    N = B * S
    g = torch.Generator().manual_seed(N + d)
    x, sigma, eps, ctx = torch.randn(N, d, generator=g), 0.1 * torch.randn(N, generator=g), torch.randn(N, d, generator=g), torch.randn(B, c, generator=g)
    xbar = torch.addcmul(x, sigma[:, None], eps)
    spec, spec_sib = layout.cdae_plain_spec(kind, d, c, h, nl), layout.cdae_spec(kind, d, c, h, nl)
    p, p_sib = init_params(spec, 3), init_params(spec_sib, 11)
    _, g64_sib = oracle_grads(kind, p_sib, act, xbar, sigma, eps, ctx, S, torch.float64, True)
    _, grads_sib, _ = Harness(kind, d, c, h, nl, act, flat_of(p_sib, spec_sib), plain=False).loss_grads(xbar, sigma, eps, ctx, B, S)
    E_sib = max(rel(grads_sib[n], g64_sib[n]) for n in grads_sib if g64_sib[n] is not None)
    loss64, g64 = oracle_grads(kind, p, act, xbar, sigma, eps, ctx, S, torch.float64, False)
    _, g32 = oracle_grads(kind, p, act, xbar, sigma, eps, ctx, S, torch.float32, False)
    loss, grads, _ = Harness(kind, d, c, h, nl, act, flat_of(p, spec)).loss_grads(xbar, sigma, eps, ctx, B, S)
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
    fx = fixture(golden_dir, fid)
    (B, S, d, c, h, nl), kind, act = dims(fx), str(fx["kind"]), str(fx["act"])
    N = B * S
    x, ctx, eps = torch.tensor(fx["x"]).cuda(), torch.tensor(fx["ctx"]).cuda(), torch.tensor(fx["eps"]).cuda()
    std = std_of(fx)
    std = std.cuda() if torch.is_tensor(std) else std
    m = build(fx)
    m.load_state_dict(state_dict_of(fx))
    m = m.cuda()
    none, loss = m(x, ctx, std, eps=eps)
    assert none is None and loss.dim() == 0
    loss.backward()
    assert abs(float(loss.detach()) - float(fx["loss"])) <= LOSS_TOL * abs(float(fx["loss"]))
    for n, p in m.named_parameters():
        if n == "neglogprob.fc.bias":
            assert p.grad is None
        else:
            assert rel(p.grad.cpu(), fx["g/" + n]) <= TENSOR_TOL, n
    glog = m.glogprob(x, ctx)
    assert glog.shape == (B, S, d) and rel(glog.cpu(), fx["glog"]) <= TENSOR_TOL
    assert torch.equal(glog, m.glogprob(x, ctx, 0.7)) and torch.equal(glog, m.glogprob(x, ctx, torch.ones(N, 1, device="cuda")))
    # std=None: self.std; a number and the tensors that broadcast to [B*S, 1] are the same call
    m.std = 0.37
    a = float(m(x, ctx, eps=eps)[1].detach())
    assert a == float(m(x, ctx, 0.37, eps=eps)[1].detach()) != float(loss.detach())
    assert a == float(m(x, ctx, torch.tensor(0.37, device="cuda"), eps=eps)[1].detach()) == float(m(x, ctx, torch.full((N, 1), 0.37, device="cuda"), eps=eps)[1].detach())
    # eps=None: the module's own Philox draw, a fresh one per call
    a, b = float(m(x, ctx, std)[1].detach()), float(m(x, ctx, std)[1].detach())
    assert np.isfinite(a) and np.isfinite(b) and a != b and a != float(loss.detach())


# ---- 6. the AR-DAE kinds: ArdaeEngine's cDAE phase behind its sampler --------------------------------------------------------------
def fresh_module(kind, d, c, h, nl, act, plain, seed=21):
    cls = getattr(net, CLS[kind]) if plain else (net.MLPGradCARDAE if kind == "grad" else net.MLPResCARDAE)
    m = cls(input_dim=d, context_dim=c, h_dim=h, num_hidden_layers=nl, nonlinearity=act)
    m.load_state_dict(init_params((layout.cdae_plain_spec if plain else layout.cdae_spec)(kind, d, c, h, nl), seed))
    return m.cuda()


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
    twin = (net.MLPGradCARDAE if kind == "grad" else net.MLPResCARDAE)(input_dim=8, context_dim=8, h_dim=64, num_hidden_layers=3, nonlinearity=cc.nonlin)
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
        eng = net.ArdaeCondScoreEngine(fresh_module(kind, z, c, h, nl, act, False), cfg, B, S, std_scale=100.0, graph=False)
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
def sigma32(cfg, i):
    return float(np.float32(net.dae_sigma(cfg.sigma_max, cfg.sigma_min, cfg.sigma_annealing, i)))


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
    data = batches(B, S, z, c, 6)
    runs = []
    for graph in (True, False):
        net.manual_seed(77)
        eng = net.ArdaeCondScoreEngine(fresh_module(kind, z, c, h, nl, act, plain), cfg, B, S, std_scale=2.0, graph=graph)
        assert eng.plain == plain and eng.fused_first == (not plain and z == 32) and eng.draw_form == plain
        trace = []
        for i, (lat, ctx, mean) in enumerate(data):
            eng.step(lat, ctx.view(B, 1, c), mean.view(B, 1, z) if i % 2 else mean)
            trace += [eng.cdae.flat_params().clone(), eng.loss.clone(), eng.sigma.clone(), eng.xbar.clone()] + [b.clone() for b in eng.opt.buffers()]
            if plain:
                assert eng.stats()["sigma"] == sigma32(cfg, i) and torch.equal(eng.sigma, torch.full((B * S * ns,), sigma32(cfg, i), device="cuda"))
        torch.cuda.synchronize()
        assert (eng._graph is not None) == graph
        runs.append(trace + [eng.state.clone()])
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(a, b) for a, b in zip(*runs)), "replayed != eager"
    losses = torch.cat(runs[0][1::4 + len(eng.opt.buffers())][:6])
    assert torch.isfinite(losses).all() and len(set(losses.tolist())) == 6
    s = runs[0][-1]
    assert int(s[0]) == STRIDE * 7 and int(s[1]) == 7                          # the block describes the coming step
    lat_b, mean_b, ctx_b = eng.input_buffers()
    assert lat_b.shape == (B, S, z) and mean_b.shape == (B, z) and ctx_b.shape == (B, c)
    assert torch.equal(lat_b, data[-1][0]) and torch.equal(ctx_b, data[-1][1]) and torch.equal(mean_b, data[-1][2])
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
        eng = net.ArdaeCondScoreEngine(fresh_module(kind, z, c, h, nl, act, True), cfg, B, S, std_scale=2.0, draw_form=draw_form)
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
    """The update on the fixture's samples / eps: every parameter after every step against the reference's fp32 run, and no further from its
    float64 run than max(2 x the fp32 reference's own distance, 2e-6)."""
    fx = load(os.path.join(golden_dir, f"cdae_plain_traj_{kind}.npz"))
    c = {k[4:]: v for k, v in fx.items() if k.startswith("cfg/")}
    B, S, ns, d, cd, h, nl, act, steps = int(c["B"]), int(c["S"]), int(c["nsigma"]), int(c["d"]), int(c["c"]), int(c["h"]), int(c["L"]), str(c["act"]), int(c["steps"])
    cfg = net.DaeConfig(sigma_max=float(c["sigma_max"]), sigma_min=float(c["sigma_min"]), sigma_annealing=int(c["sigma_annealing"]), nsigma=ns, lr=float(c["lr"]))
    m = getattr(net, CLS[kind])(input_dim=d, context_dim=cd, h_dim=h, num_hidden_layers=nl, nonlinearity=act)
    m.load_state_dict(state_dict_of(fx))
    eng = net.ArdaeCondScoreEngine(m.cuda(), cfg, B, S, std_scale=float(c["std_scale"]))
    bad = []
    for s in range(steps):
        lat, mean, ctx, eps = (torch.tensor(fx[f"{s}/{k}"]).cuda() for k in ("latent", "mean", "ctx", "eps"))
        eng.step(lat, ctx, mean, noise={"eps": eps})
        st = eng.stats()
        assert st["sigma"] == float(np.float32(float(fx[f"{s}/sigma"])))
        assert abs(st["loss"] - float(fx[f"{s}/loss"])) <= LOSS_TOL * abs(float(fx[f"{s}/loss"])), (s, st["loss"])
        for n, p in eng.cdae.named_parameters():
            p32, p64 = fx[f"{s}/p/{n}"], fx[f"{s}/p_f64/{n}"]
            e32, e64, ref64 = rel(p.detach().cpu(), p32), rel(p.detach().cpu(), p64), rel(p32, p64)
            print(f"{kind} step {s} {n}: to fp32 reference {e32:.2e}, to float64 {e64:.2e} (fp32 reference to float64 {ref64:.2e})")
            if e32 > TENSOR_TOL or e64 > max(2 * ref64, 2e-6):
                bad.append((s, n, e32, e64, ref64))
    assert not bad, bad


@pytest.mark.parametrize("plain,kind", [(True, "grad"), (True, "res"), (False, "grad"), (False, "res")])
def test_engine_equals_the_drop_in_module_route(plain, kind):
    """The same six steps through the engine and through the module + torch.optim with host-computed noise levels."""
    B, S, ns, z, c, h, nl, act, scale = 6, 8, 2, 3, 5, 64, 2, "elu", 2.0
    N = B * S * ns
    if plain:
        cfg = net.DaeConfig(sigma_max=1.0, sigma_min=0.1, sigma_annealing=4, nsigma=ns)
    else:
        cfg = net.ScoreConfig(delta=0.1, nsigma=ns, lr=1e-3, optimizer="rmsprop", momentum=0.5)
    eng = net.ArdaeCondScoreEngine(fresh_module(kind, z, c, h, nl, act, plain), cfg, B, S, std_scale=scale)
    m = fresh_module(kind, z, c, h, nl, act, plain)
    opt = torch.optim.Adam(m.parameters(), lr=cfg.lr) if plain else torch.optim.RMSprop(m.parameters(), lr=cfg.lr, momentum=0.5)
    g = torch.Generator().manual_seed(5)
    for i, (lat, ctx, mean) in enumerate(batches(B, S, z, c, 6, seed=1)):
        xi, eps = torch.randn(N, generator=g).cuda(), torch.randn(N, z, generator=g).cuda()
        eng.step(lat, ctx, mean, noise={"eps": eps} if plain else {"sigma": xi, "eps": eps})
        u = scale * (lat - mean[:, None, :])
        rows = u.unsqueeze(2).expand(B, S, ns, z).reshape(B, S * ns, z)
        opt.zero_grad()
        if plain:
            _, loss = m(rows, ctx.view(B, 1, c), net.dae_sigma(1.0, 0.1, 4, i), eps=eps)
        else:       # ivae_ardae.py:753-767: std = delta * mean_d std_S(u), one draw per row
            std = cfg.delta * u.std(dim=1, keepdim=True).mean(dim=2, keepdim=True).expand(B, S * ns, 1) * xi.view(B, S * ns, 1)
            _, loss = m(rows, ctx.view(B, 1, c), std, eps=eps)
        loss.backward()
        opt.step()
        assert abs(eng.stats()["loss"] - float(loss.detach())) <= LOSS_TOL * abs(float(loss.detach())), i
        for (n, p), (_, q) in zip(eng.cdae.named_parameters(), m.named_parameters()):
            assert rel(p.detach().cpu(), q.detach().cpu()) <= TENSOR_TOL, (i, n, rel(p.detach().cpu(), q.detach().cpu()))
    # the two routes' checkpoints are interchangeable: torch.optim's state loads into the engine
    eng.load_state_dict({"cdae": m.state_dict(), "optimizer": opt.state_dict()})
    assert eng.step_count == 6 and eng.state[:2].tolist() == [STRIDE * 7, 7]
    if plain:
        assert eng.state[3:].view(torch.float32)[0].item() == sigma32(cfg, 6)


@pytest.mark.parametrize("plain,kind,optimizer", [(True, "grad", "adam_torch"), (True, "res", "amsgrad"), (False, "grad", "rmsprop")])
def test_engine_resumes_bit_identically_across_the_end_of_the_ramp(plain, kind, optimizer):
    """state_dict() after step 2 into a fresh engine under another library seed: steps 3 - 8 (the ramp of 4 steps ends among them; eager,
    eager, captured, replayed there) leave what the uninterrupted run leaves."""
    B, S, ns, z, c, h, nl, act = 6, 8, 2, 3, 5, 64, 2, "elu"
    cfg = make_cfg(plain, ns, optimizer)
    data = batches(B, S, z, c, 8)
    runs, sd = [], None
    for resumed in (False, True):
        net.manual_seed(77)
        eng = net.ArdaeCondScoreEngine(fresh_module(kind, z, c, h, nl, act, plain), cfg, B, S)
        losses = []
        for i, (lat, ctx, mean) in enumerate(data):
            if resumed and i == 2:
                sd = eng.state_dict()
                net.manual_seed(1)                                 # the checkpoint, not the process, carries the RNG state
                eng = net.ArdaeCondScoreEngine(fresh_module(kind, z, c, h, nl, act, plain, seed=5), cfg, B, S)
                eng.load_state_dict(sd)
                assert eng._graph is None and (eng.step_count, eng.opt.steps) == (2, 2)
            eng.step(lat, ctx, mean)
            if plain:
                assert eng.stats()["sigma"] == sigma32(cfg, i)
            losses.append(eng.loss.clone())
        torch.cuda.synchronize()
        assert eng._graph is not None
        runs.append([eng.cdae.flat_params().clone(), eng.state.clone(), eng.sigma.clone(), torch.cat(losses)[2:]] + [b.clone() for b in eng.opt.buffers()])
    assert len(runs[0]) == len(runs[1]) == 4 + len(eng.opt.state_names())
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "the resumed run drifted"
    assert torch.isfinite(runs[0][3]).all() and len(set(runs[0][3].tolist())) == 6
    if plain:      # a checkpoint written under another schedule resumes at THIS engine's value: bytes 24..27 are recomputed from t
        other = net.DaeConfig(sigma_max=5.0, sigma_min=0.05, sigma_annealing=4000, nsigma=ns, optimizer=optimizer, momentum=0.5)
        new = net.ArdaeCondScoreEngine(fresh_module(kind, z, c, h, nl, act, plain, seed=5), other, B, S)
        new.load_state_dict(sd)
        assert torch.equal(new.state[:3].cpu(), sd["engine"]["step_state"][:3]) and new.state[3:].view(torch.float32)[0].item() == sigma32(other, 2)


def test_engine_refusals_leave_the_step_count_at_zero():
    z, c = 2, 3
    with pytest.raises(TypeError, match="(?s)MLPGradCDAE.*DaeConfig.*ScoreConfig"):
        net.ArdaeCondScoreEngine(fresh_module("grad", z, c, 64, 3, "softplus", True), net.ScoreConfig(), 4, 8)
    with pytest.raises(TypeError, match="(?s)MLPResCARDAE.*ScoreConfig.*DaeConfig"):
        net.ArdaeCondScoreEngine(fresh_module("res", z, c, 64, 3, "softplus", False), net.DaeConfig(), 4, 8)
    from test_engine_gpu import build as build_pair
    model, _ = build_pair(O.ModelCfg("mnist", 24, 10, 64, 2, 2, "softplus"), O.CdaeCfg("grad", 2, 2, 64, 3))
    with pytest.raises(TypeError, match="ArdaeCondScoreEngine"):       # the VAE loop's engine has no slot for a noise level beside beta
        net.ArdaeEngine(model.cuda(), fresh_module("grad", 2, 2, 64, 3, "softplus", True), net.TrainConfig(nz_cdae=8), batch_size=4)
    lat, ctx, mean = torch.zeros(4, 8, z, device="cuda"), torch.zeros(4, c, device="cuda"), torch.zeros(4, z, device="cuda")
    for plain, cfg in ((True, net.DaeConfig(nsigma=2)), (False, net.ScoreConfig(nsigma=2))):
        eng = net.ArdaeCondScoreEngine(fresh_module("grad", z, c, 64, 3, "softplus", plain), cfg, 4, 8)
        with pytest.raises(ValueError, match="batch_size=4"):
            eng.step(lat[:3], ctx, mean)                                       # a ragged batch
        with pytest.raises(ValueError, match="batch_size=4"):
            eng.step(lat, ctx[:3], mean)
        with pytest.raises(ValueError, match="batch_size=4"):
            eng.step(lat, ctx, torch.zeros(4, z + 1, device="cuda"))
        with pytest.raises(ValueError, match="batch_size=4"):
            eng.step(torch.zeros(4, 7, z, device="cuda"), ctx, mean)
        with pytest.raises(ValueError, match="step\\(latent\\)"):
            eng.step(lat.cpu(), ctx, mean)
        good = {"sigma": torch.zeros(64, device="cuda"), "eps": torch.zeros(64, z, device="cuda")}
        with pytest.raises(ValueError, match="eps must be"):
            eng.step(lat, ctx, mean, noise=dict(good, eps=torch.zeros(32, z, device="cuda")))      # nsigma forgotten
        with pytest.raises(ValueError, match="eps must be"):
            eng.step(lat, ctx, mean, noise=dict(good, eps=torch.zeros(64, z)))
        if not plain:
            with pytest.raises(ValueError, match="sigma must be"):
                eng.step(lat, ctx, mean, noise=dict(good, sigma=torch.zeros(32, device="cuda")))
        with pytest.raises(ValueError, match="computes sigma on the device" if plain else "inject them through noise"):
            eng.step(lat, ctx, mean, sigma=0.5)
        with pytest.raises(ValueError, match="score\\(ctx\\)"):
            eng.score(lat, ctx[:3])
        assert eng.step_count == 0 and eng.opt.steps == 0 and eng.state[:2].tolist() == [STRIDE, 1]
    with pytest.raises(ValueError, match="sample_size >= 2"):
        net.ArdaeCondScoreEngine(fresh_module("grad", z, c, 64, 3, "softplus", False), net.ScoreConfig(), 4, 1)


# ---- 8. quality, kept small --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["grad", "res"])
def test_learned_conditional_score_points_at_the_context(kind):
    """z | c ~ N(c, 0.25 I_2), sigma 1.0 -> 0.1 over 300 of 400 steps: the learned score(z, c) against the analytic score of the
    sigma-smoothed conditional, -(z - c) / (0.25 + 0.01), by cosine similarity on 1024 fresh pairs - and against the PyTorch autograd
    restatement (tests/test_cond_score.py) trained with torch.optim.Adam on the same data."""
    B, S, d, c, h, nl, act, steps = 64, 8, 2, 2, 64, 3, "softplus", 400
    cfg = net.DaeConfig(sigma_max=1.0, sigma_min=0.1, sigma_annealing=300, nsigma=1)
    g = torch.Generator().manual_seed(2024)
    ctxs = torch.randn(steps, B, c, generator=g).cuda()
    lats = (ctxs[:, :, None, :] + 0.5 * torch.randn(steps, B, S, d, generator=g).cuda()).contiguous()
    pc = torch.randn(1024, c, generator=g).cuda()
    pz = (pc + 0.5 * torch.randn(1024, d, generator=g).cuda()).contiguous()
    exact = -(pz - pc) / (0.25 + 0.01)
    net.manual_seed(11)
    eng = net.ArdaeCondScoreEngine(fresh_module(kind, d, c, h, nl, act, True), cfg, B, S)
    p = {k: v.cuda().requires_grad_(True) for k, v in init_params(layout.cdae_plain_spec(kind, d, c, h, nl), 21).items()}
    opt = torch.optim.Adam(list(p.values()), lr=cfg.lr)
    torch.manual_seed(3)
    for i in range(steps):
        eng.step(lats[i], ctxs[i])
        sigma = net.dae_sigma(1.0, 0.1, 300, i)
        eps = torch.randn(B * S, d, device="cuda")
        xbar = (lats[i].view(B * S, d) + sigma * eps).requires_grad_(True)
        loss = torch.nn.functional.mse_loss(sigma * score(kind, p, act, xbar, ctxs[i], S, create_graph=True), -eps)
        opt.zero_grad()
        loss.backward()
        opt.step()
    cos = torch.nn.functional.cosine_similarity
    with torch.enable_grad():
        ref_score = score(kind, {k: v.detach() for k, v in p.items()}, act, pz, pc, 1).detach()
    got, ref = float(cos(eng.score(pz.view(1024, 1, d), pc).view(1024, d), exact).mean()), float(cos(ref_score, exact).mean())
    print(f"{kind}: mean cosine similarity with the analytic score: engine {got:.4f}, autograd restatement {ref:.4f}; last losses {eng.stats()['loss']:.4f} / {float(loss.detach()):.4f}")
    assert got > 0 and got > ref - 0.05
