"""Conditional AR-DAE without an input encoder on the device (C ABI kinds 16 / 17, the fused front end with the sigma column and the per-image
bias, the modules with enc_input=False) in ArdaeCondScoreEngine and in ArdaeEngine.

Bars: loss 2e-5 relative, every gradient tensor and glogprob 1e-4 relative L2 (tests/score_restate.py).  The float64 oracle is the restatement in
tests/noenc_restate.py, which tests/test_cardae_noenc.py pins to the reference's fp64 fixtures to 1e-12."""
import os

import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import layout
from oracle import ardae_oracle as O
from noenc_restate import FIXTURE_IDS, NOENC, grads_on_xbar, score
from score_gpu_checks import (STRIDE, Harness, check_abi_against_fixture, check_drop_in_route, check_refusals,
                              check_replay_equals_eager, check_resume, fixture_case, flat_of, fresh_module, guarded, init_params, sigma_rows)
from score_restate import ARDAE, CARDAE, CDAE, LOSS_TOL, TENSOR_TOL, Family, cast, load, rel, state_dict_of
from score_restate import grads_on_xbar as sibling_grads_on_xbar

pytestmark = pytest.mark.gpu
# kind 13 (the conditional DAE without an input encoder and without a sigma column) as a record the harness takes
K13 = Family(None, lambda kind, d, c, h, nl: layout.recon_cdae_spec(d, c, h, nl, False), {}, {"res": 13}, net.DaeConfig, True, True)


# ---- 1. C ABI against every fixture ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FIXTURE_IDS)
def test_abi_matches_the_reference_fixtures(golden_dir, fid):
    check_abi_against_fixture(NOENC, golden_dir, fid)       # loss, gradients (neglogprob.fc.bias untouched), glogprob at both noise levels
    # nothing is written past N rows
    fx, kind, act, (B, S), (d, h, nl, c), x, ctx, eps, std = fixture_case(NOENC, golden_dir, fid)
    N = B * S
    hn = Harness(NOENC, kind, d, h, nl, act, flat_of(state_dict_of(fx), NOENC.spec_of(kind, d, h, nl, c)), c)
    s, xbar, cx = sigma_rows(std, N).cuda().contiguous(), (x + std * eps).cuda(), ctx.cuda()
    for need_grads in (1, 0):
        ws = torch.empty(L.query("ardae_cdae_workspace_floats", hn.d, B, S, need_grads), device="cuda")
        full, out = guarded(N, d)
        if need_grads:
            loss, grads = torch.zeros(1, device="cuda"), torch.zeros_like(hn.params)
            L.call("ardae_cdae_loss_grads", hn.d, hn.params, hn.packed, xbar, s, eps.cuda(), cx, B, S, ws, ws.numel(), loss, grads, out)
        else:
            L.call("ardae_cdae_score", hn.d, hn.params, hn.packed, xbar, s, cx, B, S, ws, ws.numel(), out)
        torch.cuda.synchronize()
        assert torch.isnan(full[N:]).all() and not torch.isnan(out).any()


# ---- 2. existing code as the oracle ------------------------------------------------------------------------------------------------
ORACLE_SHAPES = [(1, 1, 2, 2, 64, 1, "tanh"), (5, 20, 3, 5, 100, 2, "elu"), (8, 40, 8, 24, 256, 3, "softplus"), (64, 1, 32, 32, 256, 3, "softplus")]
ORACLE_IDS = [f"b{s[0]}_s{s[1]}_d{s[2]}_h{s[4]}" for s in ORACLE_SHAPES]


def oracle_inputs(B, S, d, c):
    N = B * S
    g = torch.Generator().manual_seed(N + d)
    x, sigma, eps = torch.randn(N, d, generator=g), 0.3 * torch.randn(N, generator=g), torch.randn(N, d, generator=g)
    return x, sigma, eps, torch.randn(B, c, generator=g), torch.addcmul(x, sigma[:, None], eps)


def assert_same_function(got, want, shared, what):
    """(loss, grads, score) of two harnesses: loss and score within the bars, and every tensor of `shared` ({name here: (name there, columns)})"""
    (loss, grads, sc), (loss_o, grads_o, sc_o) = got, want
    assert abs(float(loss) - float(loss_o)) <= LOSS_TOL * abs(float(loss_o)), what
    assert rel(sc, sc_o) <= TENSOR_TOL, (what, rel(sc, sc_o))
    for n, (m, cols) in shared.items():
        a, b = grads[n], grads_o[m]
        if torch.isnan(b).all():
            assert torch.isnan(a).all() and n == "neglogprob.fc.bias"
            continue
        a = a if cols is None else a[:, cols]
        assert not torch.isnan(a).any() and rel(a, b) <= TENSOR_TOL, (what, n, rel(a, b))


@pytest.mark.parametrize("B,S,d,c,h,nl,act", ORACLE_SHAPES, ids=ORACLE_IDS)
def test_res_kind_with_a_zero_sigma_column_is_kind_13(B, S, d, c, h, nl, act):
    x, sigma, eps, ctx, xbar = oracle_inputs(B, S, d, c)
    spec13 = K13.spec_of("res", d, h, nl, c)
    p = init_params(spec13, 4)
    q = dict(p)
    q["dae.layers.0.weight"] = torch.cat([p["dae.layers.0.weight"], torch.zeros(h, 1)], 1)
    old = Harness(K13, "res", d, h, nl, act, flat_of(p, spec13), c)
    new = Harness(NOENC, "res", d, h, nl, act, flat_of(q, NOENC.spec_of("res", d, h, nl, c)), c)
    shared = {n: (n, slice(0, d + h) if n == "dae.layers.0.weight" else None) for n in p}
    assert_same_function(new.loss_grads(xbar, sigma, eps, ctx, B, S), old.loss_grads(xbar, sigma, eps, ctx, B, S), shared, "kind 17 / 13")
    assert rel(new.score(x, sigma, ctx, B, S), old.score(x, None, ctx, B, S)) <= TENSOR_TOL


@pytest.mark.parametrize("kind", ["grad", "res"])
@pytest.mark.parametrize("B,S,d,c,h,nl,act", ORACLE_SHAPES, ids=ORACLE_IDS)
def test_without_a_context_weight_the_kinds_are_the_unconditional_ones(kind, B, S, d, c, h, nl, act):
    """W1c = 0: the context does not reach the energy MLP, which is then kind 2 / 3's on the same rows."""
    x, sigma, eps, ctx, xbar = oracle_inputs(B, S, d, c)
    N = B * S
    spec = NOENC.spec_of(kind, d, h, nl, c)
    q = init_params(spec, 6)
    last, last_u = NOENC.last[kind], ARDAE.last[kind]
    first = last + "layers.0.weight"
    q[first][:, d:d + h] = 0
    p = {last_u + n[len(last):]: v for n, v in q.items() if n.startswith(last)}
    p[last_u + "layers.0.weight"] = torch.cat([q[first][:, :d], q[first][:, d + h:]], 1)
    new = Harness(NOENC, kind, d, h, nl, act, flat_of(q, spec), c)
    old = Harness(ARDAE, kind, d, h, nl, act, flat_of(p, ARDAE.spec_of(kind, d, h, nl)))
    cols = torch.tensor(list(range(d)) + [d + h])
    shared = {n: (last_u + n[len(last):], cols if n == first else None) for n in q if n.startswith(last)}
    got = new.loss_grads(xbar, sigma, eps, ctx, B, S)
    assert_same_function(got, old.loss_grads(xbar, sigma, eps), shared, f"kind {NOENC.kind_id[kind]} / {ARDAE.kind_id[kind]}")
    assert rel(new.score(x, sigma, ctx, B, S), old.score(x, sigma)) <= TENSOR_TOL
    for n, g in got[1].items():       # the context encoder's gradients vanish with W1c; W1c's own do not
        if n.startswith("ctx_encode."):
            assert not torch.isnan(g).any() and float(g.abs().max()) == 0.0, n
    assert float(got[1][first][:, d:d + h].abs().max()) > 0


# ---- 3. against float64, with the kind 0 / 1 sibling as the yardstick --------------------------------------------------------------
F64_SHAPES = [(16, 64, 32, 32, 256, 3, "softplus"), (10, 30, 3, 5, 100, 2, "elu")]


@pytest.mark.parametrize("kind", ["grad", "res"])
@pytest.mark.parametrize("B,S,d,c,h,nl,act", F64_SHAPES, ids=[f"b{s[0]}_s{s[1]}_d{s[2]}_h{s[4]}" for s in F64_SHAPES])
def test_gradients_against_float64(kind, B, S, d, c, h, nl, act):
    """e <= max(2 E_sibling, 3 e_ref32 + 2e-6) per gradient tensor (e_ref32: the fp32 restatement's own distance to float64; E_sibling: the
    kind 0 / 1 network of the same widths through the same entry point against float64, worst tensor)."""
    N = B * S
    g = torch.Generator().manual_seed(N + d)
    x, sigma, eps, ctx = torch.randn(N, d, generator=g), 0.1 * torch.randn(N, generator=g), torch.randn(N, d, generator=g), torch.randn(B, c, generator=g)
    xbar = torch.addcmul(x, sigma[:, None], eps)
    spec, spec_sib = NOENC.spec_of(kind, d, h, nl, c), CARDAE.spec_of(kind, d, h, nl, c)
    p, p_sib = init_params(spec, 3), init_params(spec_sib, 11)

    def oracle(fn, pp, dtype, *extra):
        pp, xb, sg, ep, cx = cast(dtype, pp, xbar, sigma.reshape(-1, 1), eps, ctx)
        return fn(kind, pp, act, xb, sg, ep, *extra, cx, S)
    _, g64_sib = oracle(sibling_grads_on_xbar, p_sib, torch.float64, True)
    _, grads_sib, _ = Harness(CARDAE, kind, d, h, nl, act, flat_of(p_sib, spec_sib), c).loss_grads(xbar, sigma, eps, ctx, B, S)
    E_sib = max(rel(grads_sib[n], g64_sib[n]) for n in grads_sib if g64_sib[n] is not None)
    loss64, g64 = oracle(grads_on_xbar, p, torch.float64)
    _, g32 = oracle(grads_on_xbar, p, torch.float32)
    loss, grads, _ = Harness(NOENC, kind, d, h, nl, act, flat_of(p, spec), c).loss_grads(xbar, sigma, eps, ctx, B, S)
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


# ---- 4. the front end --------------------------------------------------------------------------------------------------------------
# (B, S, z, c, h, L, act), eligible for the fused forms.  The second shape has 512 values per image, below the draw kernel's 1024: there the step has
# its separate launches only, whatever is asked for; the fourth is the same network with one image of 1024 values, split over four workgroups.
FRONT_SHAPES = [((4, 32, 32, 8, 64, 2, "softplus"), True), ((1, 64, 8, 3, 64, 1, "relu"), False), ((3, 256, 32, 32, 256, 3, "softplus"), True),
                ((1, 128, 8, 3, 64, 1, "relu"), True)]


@pytest.mark.parametrize("kind", ["grad", "res"])
@pytest.mark.parametrize("shape,eligible", FRONT_SHAPES, ids=[f"b{s[0]}_s{s[1]}_z{s[2]}_h{s[4]}_L{s[5]}" for s, _ in FRONT_SHAPES])
def test_own_draw_forms_equal_the_unfused_launches(kind, shape, eligible):
    """One own-draw step in its three forms (draws + first energy layer in the perturbation kernel; draws in it; two draws and the perturbation): the
    same xbar / sigma / eps / std_b bit for bit - the draws are remade at the step's offsets - and loss and parameters within the tolerances."""
    B, S, z, c, h, nl, act = shape
    g = torch.Generator().manual_seed(3)
    mean = torch.randn(B, z, generator=g).cuda()
    latent = (mean[:, None, :] + 0.01 * torch.randn(B, S, z, generator=g).cuda()).contiguous()
    ctx = torch.randn(B, c, generator=g).cuda()
    cfg = net.ScoreConfig(delta=0.1, nsigma=1, lr=1e-4)
    desc = L.CdaeDesc(NOENC.kind_id[kind], z, c, h, nl, L.ACT[act])
    assert bool(L.query("ardae_cdae_perturb_fused_ok", desc, S, 1)) == eligible == bool(L.query("ardae_latent_perturb_draw_ok", S, 1, z))
    runs = {}
    for form in ("first_layer", "draw", "unfused"):
        net.manual_seed(55)
        eng = net.ArdaeCondScoreEngine(fresh_module(NOENC, kind, z, h, nl, act, c), cfg, B, S, std_scale=100.0, graph=False, fused_first=True)
        assert eng.fused_first == eligible and eng.fused_draw == eligible
        eng.fused_first, eng.fused_draw = eligible and form == "first_layer", eligible and form != "unfused"
        eng.step(latent, ctx, mean)
        runs[form] = [t.clone() for t in (eng.xbar, eng.sigma, eng.eps, eng.std_b, eng.loss, eng.cdae.flat_params())]
    torch.cuda.synchronize()
    xi, eps = torch.empty(B * S, device="cuda"), torch.empty(B * S, z, device="cuda")
    L.call("ardae_philox_normal_at", xi, B * S, 55, STRIDE + 0, None, 0)             # in-step offsets RNG_STRIDE * step + {0: xi, 1: eps}, step 1
    L.call("ardae_philox_normal_at", eps, B * S * z, 55, STRIDE + 1, None, 0)
    assert torch.equal(runs["unfused"][2], eps)
    assert torch.equal(runs["unfused"][1], runs["unfused"][3].repeat_interleave(S) * xi)
    assert torch.isfinite(runs["unfused"][4]).all() and float(runs["unfused"][3].min()) > 0
    for form in ("first_layer", "draw"):
        assert all(torch.equal(a, b) for a, b in zip(runs[form][:4], runs["unfused"][:4])), form
        e_loss, e_par = abs(float(runs[form][4]) - float(runs["unfused"][4])) / abs(float(runs["unfused"][4])), rel(runs[form][5].cpu(), runs["unfused"][5].cpu())
        print(f"{kind} {shape} {form}: loss {float(runs[form][4]):.7f} / {float(runs['unfused'][4]):.7f} ({e_loss:.1e}), parameters {e_par:.1e}")
        assert e_loss <= LOSS_TOL and e_par <= TENSOR_TOL


# ---- 5. modules --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FIXTURE_IDS)
def test_module_forward_backward(golden_dir, fid):
    """The drop-in module on one fixture: loss and .grad against the reference and - the same ABI call on the same xbar - against the harness bit
    for bit; glogprob at both noise levels; the defaults of std and eps.  (ConditionalARDAE.forward perturbs with torch.addcmul, so the body that
    score_gpu_checks.check_module_forward_backward shares among the families that perturb with ardae_dae_perturb is restated here.)"""
    fx, kind, act, (B, S), (d, h, nl, c), x, ctx, eps, std = fixture_case(NOENC, golden_dir, fid)
    N = B * S
    x, eps, std = x.cuda(), eps.cuda(), std.cuda()
    m = NOENC.module(kind, d, h, nl, act, c)
    m.load_state_dict(state_dict_of(fx))
    m = m.cuda()
    args = (torch.tensor(fx["x"]).cuda(), torch.tensor(fx["ctx"]).cuda())
    assert args[0].shape == (B, S, d) and args[1].shape == (B, 1, c)
    call = lambda *a, **kw: m(*args, *a, **kw)[1]
    none, loss = m(*args, std.view(B, S, 1), eps=eps)
    assert none is None and loss.dim() == 0
    loss.backward()
    assert abs(float(loss.detach()) - float(fx["loss"])) <= LOSS_TOL * abs(float(fx["loss"]))
    hn = Harness(NOENC, kind, d, h, nl, act, m.flat_params().detach().cpu(), c)
    s = sigma_rows(std, N)
    abi_loss, abi_grads, _ = hn.loss_grads(torch.addcmul(x, s[:, None], eps), s, eps, ctx, B, S)
    assert float(loss.detach()) == float(abi_loss)
    for n, p in m.named_parameters():
        if n == "neglogprob.fc.bias":
            assert p.grad is None
        else:
            assert torch.equal(p.grad.cpu(), abi_grads[n]), n
            assert rel(p.grad.cpu(), fx["g/" + n]) <= TENSOR_TOL, n
    glog = m.glogprob(*args)
    assert glog.shape == (B, S, d)
    assert rel(glog.cpu(), fx["glog0"]) <= TENSOR_TOL and rel(m.glogprob(*args, std).cpu(), fx["glog"]) <= TENSOR_TOL
    # std=None: zeros, so the loss is mean(eps^2) whatever the network says
    loss0 = call(eps=eps)
    assert abs(float(loss0.detach()) - float((eps ** 2).mean())) <= 1e-6 * float((eps ** 2).mean())
    a, b = float(call(std).detach()), float(call(std).detach())                  # the module's own Philox draw, a fresh one per call
    assert torch.isfinite(torch.tensor([a, b])).all() and a != b and a != float(loss.detach())


def batches(B, S, z, c, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        mean = torch.randn(B, z, generator=g)
        out.append(((mean[:, None, :] + 0.5 * torch.randn(B, S, z, generator=g)).cuda(), torch.randn(B, c, generator=g).cuda(), mean.cuda()))
    return out


@pytest.mark.parametrize("kind", ["grad", "res"])
def test_engine_equals_the_drop_in_module_route(kind):
    """The same six steps through the engine and through the module + torch.optim with host-computed noise levels."""
    B, S, ns, z, c, h, nl, act = 6, 8, 2, 3, 5, 64, 2, "elu"
    data = iter(batches(B, S, z, c, 6, seed=1))
    check_drop_in_route(NOENC, kind, z, h, nl, act, c, B, (S,), ns, lambda g: next(data), scale=2.0)


# ---- 6. ArdaeCondScoreEngine -------------------------------------------------------------------------------------------------------
def make_cfg(ns, optimizer):
    return net.ScoreConfig(delta=0.1, nsigma=ns, lr=1e-3, optimizer=optimizer, momentum=0.5)


ENGINE_CASES = [("grad", 4, 32, 1, 32, 8, 64, 2, "softplus", "adam_torch", True), ("grad", 6, 8, 2, 3, 5, 64, 2, "elu", "adam_torch", False),
                ("res", 4, 32, 1, 32, 8, 64, 2, "softplus", "rmsprop", True), ("res", 6, 8, 2, 3, 5, 64, 3, "softplus", "rmsprop", None)]


@pytest.mark.parametrize("kind,B,S,ns,z,c,h,nl,act,optimizer,fused_first", ENGINE_CASES, ids=[f"{e[0]}_ns{e[3]}_{e[9]}" for e in ENGINE_CASES])
def test_engine_replay_equals_eager(kind, B, S, ns, z, c, h, nl, act, optimizer, fused_first):
    cfg = make_cfg(ns, optimizer)
    raw = batches(B, S, z, c, 6)
    data = [(lat, ctx.view(B, 1, c), mean.view(B, 1, z) if i % 2 else mean) for i, (lat, ctx, mean) in enumerate(raw)]
    flags = dict(fused_first=bool(fused_first), fused_draw=z == 32, draw_form=False)
    eng = check_replay_equals_eager(NOENC, lambda: fresh_module(NOENC, kind, z, h, nl, act, c), cfg, B, (S,), data, flags, std_scale=2.0, fused_first=fused_first)
    assert int(eng.cdae._desc.kind) == NOENC.kind_id[kind]
    # score(): glogprob(std_scale (latent - mean), ctx, sigma = 0) with the engine's weights, for any B', S'
    lat, ctx, mean = batches(3, 5, z, c, 1, seed=9)[0]
    got = eng.score(lat, ctx.view(3, 1, c), mean)
    want = eng.cdae.glogprob(2.0 * (lat - mean[:, None, :]), ctx.view(3, 1, c), torch.zeros(3, 5, 1, device="cuda"))
    assert got.shape == (3, 5, z) and torch.equal(got, want)
    assert torch.equal(eng.score(lat, ctx), eng.score(lat, ctx, torch.zeros(3, 1, z, device="cuda")))
    st = eng.stats()
    assert st["std_min"] <= st["std_mean"] <= st["std_max"] and st["std_min"] > 0 and st["loss"] == float(eng.loss)
    assert list(eng.state_dict()) == ["cdae", "optimizer", "engine"]


@pytest.mark.parametrize("kind", ["grad", "res"])
def test_engine_follows_the_recorded_trajectory(golden_dir, kind):
    """The update on the fixture's samples / xi / eps: every parameter after every step against the reference's fp32 run, and no further from its
    float64 run than max(2 x the fp32 reference's own distance, 2e-6) - the criterion of score_gpu_checks.check_recorded_trajectory."""
    fx = load(os.path.join(golden_dir, f"cardae_noenc_traj_{kind}.npz"))
    c = {k[4:]: v for k, v in fx.items() if k.startswith("cfg/")}
    B, S, ns, d, h, nl, act, steps = int(c["B"]), int(c["S"]), int(c["nsigma"]), int(c["d"]), int(c["h"]), int(c["L"]), str(c["act"]), int(c["steps"])
    cfg = net.ScoreConfig(delta=float(c["delta"]), nsigma=ns, lr=float(c["lr"]), optimizer="adam_torch", beta1=0.9)
    m = NOENC.module(kind, d, h, nl, act, int(c["c"]))
    m.load_state_dict(state_dict_of(fx))
    eng = net.ArdaeCondScoreEngine(m.cuda(), cfg, B, S, std_scale=float(c["std_scale"]))
    bad = []
    for s in range(steps):
        eng.step(*(torch.tensor(fx[f"{s}/{k}"]).cuda() for k in ("latent", "ctx", "mean")),
                 noise={"sigma": torch.tensor(fx[f"{s}/xi"]).cuda(), "eps": torch.tensor(fx[f"{s}/eps"]).cuda()})
        st = eng.stats()
        assert abs(st["loss"] - float(fx[f"{s}/loss"])) <= LOSS_TOL * abs(float(fx[f"{s}/loss"])), (s, st["loss"])
        for n, p in eng.cdae.named_parameters():
            p32, p64 = fx[f"{s}/p/{n}"], fx[f"{s}/p_f64/{n}"]
            e32, e64, ref64 = rel(p.detach().cpu(), p32), rel(p.detach().cpu(), p64), rel(p32, p64)
            print(f"{kind} step {s} {n}: to fp32 reference {e32:.2e}, to float64 {e64:.2e} (fp32 reference to float64 {ref64:.2e})")
            if e32 > TENSOR_TOL or e64 > max(2 * ref64, 2e-6):
                bad.append((s, n, e32, e64, ref64))
    assert not bad, bad


@pytest.mark.parametrize("kind,optimizer", [("grad", "adam_torch"), ("res", "rmsprop")])
def test_engine_resumes_bit_identically(kind, optimizer):
    B, S, ns, z, c, h, nl, act = 6, 8, 2, 3, 5, 64, 2, "elu"
    check_resume(NOENC, lambda seed: fresh_module(NOENC, kind, z, h, nl, act, c, seed=seed), make_cfg(ns, optimizer), None, B, (S,), batches(B, S, z, c, 8), 2, {})


def test_engine_refusals_leave_the_step_count_at_zero():
    z, c = 2, 3
    lat, ctx, mean = torch.zeros(4, 8, z, device="cuda"), torch.zeros(4, c, device="cuda"), torch.zeros(4, z, device="cuda")
    eng = check_refusals(NOENC, lambda: fresh_module(NOENC, "grad", z, 64, 3, "softplus", c), lambda: fresh_module(CDAE, "grad", z, 64, 3, "softplus", c), 4, (8,),
                         (lat, ctx, mean), lat[:3])
    with pytest.raises(ValueError, match="batch_size=4"):
        eng.step(lat, ctx[:3], mean)
    with pytest.raises(ValueError, match="score\\(ctx\\)"):
        eng.score(lat, ctx[:3])
    assert eng.step_count == 0 and eng.opt.steps == 0 and eng.state[:2].tolist() == [STRIDE, 1]
    with pytest.raises(ValueError, match="sample_size >= 2"):
        net.ArdaeCondScoreEngine(fresh_module(NOENC, "res", z, 64, 3, "softplus", c), net.ScoreConfig(), 4, 1)


# ---- 7. ArdaeEngine ----------------------------------------------------------------------------------------------------------------
MC = O.ModelCfg("mnist", 24, 10, 64, 8, 2, "softplus")


def vae_pair(kind, seed=1):
    from test_engine_gpu import build as build_pair
    model, _ = build_pair(MC, O.CdaeCfg(kind, 8, 8, 64, 3))
    model.load_state_dict(O.init_params(O.model_param_spec(MC), 0, O.model_init_special(MC)))
    cdae = NOENC.module(kind, 8, 64, 3, "softplus", 8, std=1.)
    cdae.load_state_dict(init_params(NOENC.spec_of(kind, 8, 64, 3, 8), seed))
    return model.cuda(), cdae.cuda()


def images(n, B=4, seed=9):
    g = torch.Generator().manual_seed(seed)
    return [torch.bernoulli(torch.full((B, 24), 0.3), generator=g).cuda() for _ in range(n)]


@pytest.mark.parametrize("kind,nstd", [("grad", 1), ("res", 3)])
def test_cdae_phase_of_the_vae_engine_is_the_score_engine_step(kind, nstd):
    """The same ABI calls at the same shapes: with injected noise, a step on the latent / z0 / context that a tiny ArdaeEngine's cdae_phase
    used leaves the same x_bar, sigma, std_b, loss, parameters and optimiser buffers, bit for bit."""
    B, nz = 4, 16
    N = B * nz * nstd
    tcfg = net.TrainConfig(nz_cdae=nz, nstd_cdae=nstd)
    model, cdae = vae_pair(kind)
    twin = NOENC.module(kind, 8, 64, 3, "softplus", 8)
    twin.load_state_dict(cdae.state_dict())
    eng = net.ArdaeEngine(model, cdae, tcfg, batch_size=B)
    assert int(eng.cdae._desc.kind) == NOENC.kind_id[kind] and eng.n_c == cdae.flat_params().numel() - (kind == "grad")
    g = torch.Generator().manual_seed(9)
    x = images(1)[0]
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


@pytest.mark.parametrize("kind", ["grad", "res"])
def test_vae_engine_steps_replay_resume_and_score(kind, tmp_path):
    """Six steps with graph=True equal six with graph=False; after a step eng.g is cdae.glogprob on eng.u / eng.ctx_v at sigma 0; a checkpoint
    written after step 2 resumes on the same bits.  All bit for bit."""
    B, nz = 4, 16
    xs = images(12)
    runs, ckpt = [], None
    for graph in (True, False):
        net.manual_seed(123)
        model, cdae = vae_pair(kind)
        eng = net.ArdaeEngine(model, cdae, net.TrainConfig(nz_cdae=nz), batch_size=B, graph=graph)
        trace = []
        for i in range(6):
            eng.step(xs[2 * i], xs[2 * i + 1])
            trace += [model.flat_params().clone(), cdae.flat_params().clone(), eng.loss_c.clone(), eng.g.clone()]
            if graph and i == 1:
                ckpt = (eng.model_checkpoint(), eng.cdae_checkpoint())
                torch.save(ckpt[1], tmp_path / "cdae.pth.tar")
                names = [n for n, _ in NOENC.spec_of(kind, 8, 64, 3, 8)]
                assert list(ckpt[1]["state_dict"]) == names and set(ckpt[1]["optimizer"]["state"]) == set(range(len(names) - (kind == "grad")))
        torch.cuda.synchronize()
        nzm = eng.u.numel() // (B * 8)
        want = cdae.glogprob(eng.u.view(B, nzm, 8), eng.ctx_v.view(B, 1, 8), torch.zeros(B, nzm, 1, device="cuda"))
        assert torch.equal(eng.g.view(B, nzm, 8), want) and torch.isfinite(eng.g).all()
        runs.append(trace)
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "replayed != eager"
    assert len({float(t) for t in runs[0][2::4]}) == 6
    net.manual_seed(1)
    model, cdae = vae_pair(kind, seed=5)
    eng = net.ArdaeEngine(model, cdae, net.TrainConfig(nz_cdae=nz), batch_size=B)
    eng.load_checkpoints(ckpt[0], torch.load(tmp_path / "cdae.pth.tar", weights_only=True))
    assert eng.step_count == 2
    for i in range(2, 6):
        eng.step(xs[2 * i], xs[2 * i + 1])
    assert torch.equal(model.flat_params(), runs[0][-4]) and torch.equal(cdae.flat_params(), runs[0][-3])


def test_vae_engine_still_refuses_a_plain_cdae():
    model, _ = vae_pair("grad")
    with pytest.raises(TypeError, match="ArdaeCondScoreEngine"):
        net.ArdaeEngine(model, fresh_module(CDAE, "grad", 8, 64, 3, "softplus", 8), net.TrainConfig(nz_cdae=16), batch_size=4)


# ---- 8. quality, kept small --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["grad", "res"])
def test_learned_conditional_score_points_at_the_context(kind):
    """z | c ~ N(c, 0.25 I_2), the AR-DAE update with sigma = delta * mean_d std_S(z) * xi for 400 steps: the learned score(z, c) at sigma 0 against
    the analytic score -(z - c) / 0.25 by cosine similarity on 1024 fresh pairs - and against the PyTorch autograd restatement
    (tests/noenc_restate.py) of the same network trained with torch.optim.Adam on the same data and the same draws.  (At 400 steps the
    restatement's own result moves by 0.05 - 0.1 between seeds of the noise draws - sigma = 0 is the edge of the noise levels an AR-DAE sees - so
    both routes take the same xi and eps: injected into the engine, which then runs the step's launches eagerly.)"""
    B, S, d, c, h, nl, act, steps = 64, 8, 2, 2, 64, 3, "softplus", 400
    cfg = net.ScoreConfig(delta=0.5, nsigma=1, lr=1e-3, optimizer="adam_torch", beta1=0.9)
    g = torch.Generator().manual_seed(2024)
    ctxs = torch.randn(steps, B, c, generator=g).cuda()
    lats = (ctxs[:, :, None, :] + 0.5 * torch.randn(steps, B, S, d, generator=g).cuda()).contiguous()
    pc = torch.randn(1024, c, generator=g).cuda()
    pz = (pc + 0.5 * torch.randn(1024, d, generator=g).cuda()).contiguous()
    exact = -(pz - pc) / 0.25
    net.manual_seed(11)
    eng = net.ArdaeCondScoreEngine(fresh_module(NOENC, kind, d, h, nl, act, c), cfg, B, S)
    p = {k: v.cuda().requires_grad_(True) for k, v in init_params(NOENC.spec_of(kind, d, h, nl, c), 21).items()}
    opt = torch.optim.Adam(list(p.values()), lr=cfg.lr)
    torch.manual_seed(3)
    for i in range(steps):
        xi, eps = torch.randn(B, S, 1, device="cuda"), torch.randn(B * S, d, device="cuda")
        eng.step(lats[i], ctxs[i], noise={"sigma": xi.reshape(-1), "eps": eps})
        sigma = (cfg.delta * lats[i].std(dim=1, keepdim=True).mean(dim=2, keepdim=True).expand(B, S, 1) * xi).reshape(B * S, 1)
        xbar = (lats[i].view(B * S, d) + sigma * eps).requires_grad_(True)
        loss = torch.nn.functional.mse_loss(sigma * score(kind, p, act, xbar, sigma, ctxs[i], S, create_graph=True), -eps)
        opt.zero_grad()
        loss.backward()
        opt.step()
    cos = torch.nn.functional.cosine_similarity
    zero = torch.zeros(1024, 1, device="cuda")
    with torch.enable_grad():
        ref_score = score(kind, {k: v.detach() for k, v in p.items()}, act, pz, zero, pc, 1).detach()
    got, ref = float(cos(eng.score(pz.view(1024, 1, d), pc).view(1024, d), exact).mean()), float(cos(ref_score, exact).mean())
    print(f"{kind}: mean cosine similarity with the analytic score: engine {got:.4f}, autograd restatement {ref:.4f}; last losses {eng.stats()['loss']:.4f} / {float(loss.detach()):.4f}")
    assert got > 0 and got > ref - 0.05
