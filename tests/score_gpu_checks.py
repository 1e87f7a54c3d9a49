"""What the GPU tests of the score-network families outside the VAE loop (tests/test_ardae_uncond_gpu.py, test_dae_plain_gpu.py,
test_cond_score_gpu.py) share, written once: ONE harness over the C ABI's pack / loss_grads / score for any of the eight kinds, the front ends
of the unconditional updates as functions of it, parameter and buffer helpers, and the bodies of the tests every family has - the ABI against the
reference's fixtures, the zero-sigma-column equivalence, module forward / backward, replay == eager, the recorded trajectory, the drop-in module
route, resume, refusals - as functions of a `Family` record (tests/score_restate.py).  Not a test module: nothing here is collected.

Engines are built as `family.engine(module, cfg, B, *S)`: S is () for the unconditional engines and (sample_size,) for the conditional one.
A body holds what is the same test in every family it runs for; where the families' copies asserted different things about the same step it
asserts all of them.  What one family alone has stays in that family's file.

Bars: loss 2e-5 relative, every gradient tensor and glogprob 1e-4 relative L2 against the reference's fp32 fixtures."""
import os
import weakref

import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from score_restate import AR_SIBLING, LOSS_TOL, TENSOR_TOL, dims, load, meta, rel, state_dict_of, std_of

STRIDE = 16


def flat_of(p, spec):
    return torch.cat([p[n].reshape(-1).float() for n, _ in spec])


def split_flat(v, spec):
    out, off = {}, 0
    for n, shp in spec:
        k = int(np.prod(shp))
        out[n] = v[off:off + k].view(*shp)
        off += k
    return out


def init_params(spec, seed):
    """nn.Linear's family: U(+-1/sqrt(fan_in)) for weight and bias."""
    g = torch.Generator().manual_seed(seed)
    out, bound = {}, None
    for n, shp in spec:
        if n.endswith("weight"):
            bound = 1.0 / shp[1] ** 0.5
        out[n] = (torch.rand(*shp, generator=g) * 2 - 1) * bound
    return out


def fresh_module(family, kind, d, h, nl, act, c=0, seed=21):
    m = family.module(kind, d, h, nl, act, c)
    m.load_state_dict(init_params(family.spec_of(kind, d, h, nl, c), seed))
    return m.cuda()


def sigma_rows(std, N):
    """The per-row [N] array the ABI takes for the reference's float or [N, 1] std."""
    return std.reshape(-1) if torch.is_tensor(std) else torch.full((N,), float(std))


def sigma32(cfg, i):
    return float(np.float32(net.dae_sigma(cfg.sigma_max, cfg.sigma_min, cfg.sigma_annealing, i)))


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
    """The C ABI for one score network of `family`: ctx=None and c=0 for the unconditional kinds, where B defaults to the row count."""

    def __init__(self, family, kind, d, h, nl, act, flat_params, c=0):
        self.kind, self.d_in, self.c, self.h = kind, d, c, h
        self.spec = family.spec_of(kind, d, h, nl, c)
        self.d = L.CdaeDesc(family.kind_id[kind], d, c, h, nl, L.ACT[act])
        assert L.query("ardae_cdae_param_floats", self.d) == flat_params.numel()
        self.params = flat_params.cuda()
        self.packed = torch.empty(L.query("ardae_cdae_packed_floats", self.d), device="cuda")
        L.call("ardae_cdae_pack", self.d, self.params, self.packed)

    def _ctx(self, ctx, B):
        return None if ctx is None else ctx.reshape(B, self.c).contiguous().cuda()

    def loss_grads(self, xbar, sigma, eps, ctx=None, B=None, S=1):
        """-> loss, {name: gradient, NaN where the call wrote nothing}, the score; the workspace stays in self.ws"""
        N = xbar.size(0)
        B = N if B is None else B
        assert B * S == N
        self.ws = torch.empty(L.query("ardae_cdae_workspace_floats", self.d, B, S, 1), device="cuda")
        loss, grads = torch.zeros(1, device="cuda"), torch.full_like(self.params, float("nan"))
        sc = torch.empty(N, self.d_in, device="cuda")
        xbar, sigma, eps = (t.contiguous().cuda() for t in (xbar, sigma.reshape(-1), eps))
        L.call("ardae_cdae_loss_grads", self.d, self.params, self.packed, xbar, sigma, eps, self._ctx(ctx, B), B, S, self.ws, self.ws.numel(), loss, grads, sc)
        torch.cuda.synchronize()
        return loss.cpu(), split_flat(grads.cpu(), self.spec), sc.cpu()

    def score(self, x, sigma=None, ctx=None, B=None, S=1):
        N = x.size(0)
        B = N if B is None else B
        assert B * S == N
        ws = torch.empty(L.query("ardae_cdae_workspace_floats", self.d, B, S, 0), device="cuda")
        out = torch.empty(N, self.d_in, device="cuda")
        L.call("ardae_cdae_score", self.d, self.params, self.packed, x.contiguous().cuda(), None if sigma is None else sigma.reshape(-1).contiguous().cuda(),
               self._ctx(ctx, B), B, S, ws, ws.numel(), out)
        torch.cuda.synchronize()
        return out.cpu()


# ---- the front ends of the unconditional updates, on a Harness ---------------------------------------------------------------------------
def fused(hn, x, B, ns, delta, seed, first_row=0, state=None):
    """-> loss, grads, xbar, sigma, eps, h_1 of ardae_dae_perturb_loss_grads (kinds 2 / 3)"""
    N = B * ns
    ws = torch.empty(L.query("ardae_cdae_workspace_floats", hn.d, N, 1, 1), device="cuda")
    loss, grads = torch.zeros(1, device="cuda"), torch.full_like(hn.params, float("nan"))
    xbar, sigma, eps = torch.empty(N, hn.d_in, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, hn.d_in, device="cuda")
    L.call("ardae_dae_perturb_loss_grads", hn.d, hn.params, hn.packed, x, B, ns, delta, seed, 3, 4, state, first_row, xbar, sigma, eps, ws,
           ws.numel(), loss, grads)
    torch.cuda.synchronize()
    return loss.cpu(), split_flat(grads.cpu(), hn.spec), xbar, sigma, eps, ws[:N * hn.h].clone()


def unfused(hn, x, B, ns, delta, seed, first_row=0, state=None):
    """The same through two draws, the perturbation and ardae_cdae_loss_grads"""
    N = B * ns
    n, eps = torch.empty(N, device="cuda"), torch.empty(N, hn.d_in, device="cuda")
    L.call("ardae_philox_normal_at", n, N, seed, 3, state, first_row)
    L.call("ardae_philox_normal_at", eps, N * hn.d_in, seed, 4, state, first_row * hn.d_in)
    sigma = delta * n                                   # one fp32 multiply
    xbar = torch.empty(N, hn.d_in, device="cuda")
    L.call("ardae_dae_perturb", x, sigma, eps, B, ns, hn.d_in, xbar)
    loss, grads, _ = hn.loss_grads(xbar, sigma, eps)
    return loss, grads, xbar, sigma, eps, hn.ws[:N * hn.h].clone()


def front(hn, x, B, ns, sigma, dae_state, seed, first_row=0, state=None):
    """-> loss, grads, xbar, sigma_out, eps, h_1 of the plain update's three launches (kinds 6 / 7); the three outputs carry a NaN guard row"""
    N = B * ns
    (xb_all, xbar), (sg_all, sg), (ep_all, eps) = guarded(N, hn.d_in), guarded(N), guarded(N, hn.d_in)
    L.call("ardae_philox_normal_at", eps, N * hn.d_in, seed, 4, state, first_row * hn.d_in)
    L.call("ardae_dae_noise_perturb", x, eps, B, ns, hn.d_in, sigma, dae_state, xbar, sg)
    loss, grads, _ = hn.loss_grads(xbar, sg, eps)
    for full in (xb_all, sg_all, ep_all):
        assert torch.isnan(full[N:]).all() and not torch.isnan(full[:N]).any()
    return loss, grads, xbar, sg, eps, hn.ws[:N * hn.h].clone()


def assert_matches_reference(got, fx, prefix, what):
    for n, g in got.items():
        if f"{prefix}/{n}/none" in fx:
            assert torch.isnan(g).all(), f"{what}: {n} must stay untouched (the reference's .grad is None)"
        else:
            assert not torch.isnan(g).any(), (what, n)
            e = rel(g, fx[f"{prefix}/{n}"])
            assert e <= TENSOR_TOL, f"{what}: {n} relL2 {e:.2e}"


def same_bits(a, b):
    """Two results of Harness.loss_grads, bit for bit (the untouched tensors are NaN in both)"""
    return torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and all(torch.equal(torch.nan_to_num(a[1][n]), torch.nan_to_num(b[1][n])) for n in a[1])


def fixture_case(family, golden_dir, fid):
    """-> fx, kind, act, (B, S), (d, h, L, c), x [N, d], ctx [B, c] | None, eps, std (a float or [N, 1]) of one fixture, on the host"""
    fx = family.fixture(golden_dir, fid)
    if family.conditional:
        (B, S, d, c, h, nl), kind, act = dims(fx), str(fx["kind"]), str(fx["act"])
        ctx = torch.tensor(fx["ctx"]).view(B, c)
    else:
        (kind, act, B, d, h, nl), S, c, ctx = meta(fx), 1, 0, None
    return fx, kind, act, (B, S), (d, h, nl, c), torch.tensor(fx["x"]).view(B * S, d), ctx, torch.tensor(fx["eps"]), std_of(fx)


# ---- the bodies -------------------------------------------------------------------------------------------------------------------------
def check_abi_against_fixture(family, golden_dir, fid):
    """ardae_cdae_loss_grads and ardae_cdae_score on one fixture of the reference."""
    fx, kind, act, (B, S), (d, h, nl, c), x, ctx, eps, std = fixture_case(family, golden_dir, fid)
    N = B * S
    s = sigma_rows(std, N)
    hn = Harness(family, kind, d, h, nl, act, flat_of(state_dict_of(fx), family.spec_of(kind, d, h, nl, c)), c)
    xbar = x + std * eps                                        # add_gaussian_noise as the reference evaluates it
    got = loss, grads, sc = hn.loss_grads(xbar, s, eps, ctx, B, S)
    print(f"{fid}: loss {float(loss):.7f} (reference {float(fx['loss']):.7f})")
    assert abs(float(loss) - float(fx["loss"])) <= LOSS_TOL * abs(float(fx["loss"]))
    assert_matches_reference(grads, fx, "g", fid)
    assert [n for n, g in grads.items() if torch.isnan(g).any()] == (["neglogprob.fc.bias"] if kind == "grad" else [])       # the prefill survives there only
    if family.plain:           # score: the same bits whatever sigma is passed
        glog = hn.score(x, None, ctx, B, S)
        assert rel(glog, fx["glog"].reshape(N, d)) <= TENSOR_TOL
        for other in (s, torch.zeros(N), torch.full((N,), float("nan"))):
            assert torch.equal(glog, hn.score(x, other, ctx, B, S))
    else:
        assert rel(hn.score(x, torch.zeros(N), ctx, B, S), fx["glog0"].reshape(N, d)) <= TENSOR_TOL
        assert rel(hn.score(x, s, ctx, B, S), fx["glog"].reshape(N, d)) <= TENSOR_TOL
    # the same rows in another factorisation N = B S.  Without a context: the same bits.  With one, 4 x the images of a quarter of the samples
    # each, every context row 4 times, is the same function - but the context encoder and the per-image reductions then sum in another
    # order, so the fixtures' own bars hold, not the bits.
    if not family.conditional and N % 4 == 0:
        assert same_bits(got, hn.loss_grads(xbar, s, eps, None, N // 4, 4))
    if family.conditional and S % 4 == 0:
        loss2, grads2, sc2 = hn.loss_grads(xbar, s, eps, ctx.repeat_interleave(4, 0), 4 * B, S // 4)
        assert abs(float(loss2) - float(loss)) <= LOSS_TOL * abs(float(loss)) and rel(sc2, sc) <= TENSOR_TOL
        assert_matches_reference(grads2, fx, "g", f"{fid} as {4 * B} x {S // 4}")


def check_zero_sigma_column(family, kind, B, S, d, c, h, nl, act):
    """A plain family against its AR-DAE sibling with a zero sigma column - the same function: existing code as the oracle."""
    sibling, N = AR_SIBLING[family], B * S
    g = torch.Generator().manual_seed(N + d)
    x, sigma, eps = torch.randn(N, d, generator=g), 0.3 * torch.randn(N, generator=g), torch.randn(N, d, generator=g)
    ctx = torch.randn(B, c, generator=g) if family.conditional else None
    spec = family.spec_of(kind, d, h, nl, c)
    p = init_params(spec, 4)
    first = family.last[kind] + "layers.0.weight"
    q = dict(p)
    q[first] = torch.cat([p[first], torch.zeros(h, 1)], 1)                                  # fma(sigma, 0, v) = v
    xbar = torch.addcmul(x, sigma[:, None], eps)
    hn = Harness(family, kind, d, h, nl, act, flat_of(p, spec), c)
    ar = Harness(sibling, kind, d, h, nl, act, flat_of(q, sibling.spec_of(kind, d, h, nl, c)), c)
    loss, grads, sc = hn.loss_grads(xbar, sigma, eps, ctx, B, S)
    loss_o, grads_o, sc_o = ar.loss_grads(xbar, sigma, eps, ctx, B, S)
    grads_o[first] = grads_o[first][:, :p[first].shape[1]]                                  # all tensors but the sigma column
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
    assert rel(hn.score(x, None, ctx, B, S), ar.score(x, sigma, ctx, B, S)) <= TENSOR_TOL    # (N == B: kind 10 walks kind 0's one-launch chain)
    print(f"{kind} B={B} S={S} d={d} h={h} L={nl} {act}: {100 * same / total:.3f} % of the score and gradient elements bit-identical, loss {float(loss):.7f} / {float(loss_o):.7f}")


def check_module_forward_backward(family, golden_dir, fid):
    """The drop-in module on one fixture: loss and .grad against the reference and - the same ABI call on the same xbar - against the harness
    bit for bit; glogprob; the defaults of std and eps."""
    fx, kind, act, (B, S), (d, h, nl, c), x, ctx, eps, std = fixture_case(family, golden_dir, fid)
    N = B * S
    x, eps = x.cuda(), eps.cuda()
    std = std.cuda() if torch.is_tensor(std) else std
    m = family.module(kind, d, h, nl, act, c)
    m.load_state_dict(state_dict_of(fx))
    m = m.cuda()
    if family.conditional:           # the modules' own shapes: [B, S, d] samples of [B, 1, c] contexts
        args = (torch.tensor(fx["x"]).cuda(), torch.tensor(fx["ctx"]).cuda())
        assert args[0].shape == (B, S, d) and args[1].dim() == 3
    else:
        args = (x,)
    call = lambda *a, **kw: m(*args, *a, **kw)[1]
    none, loss = m(*args, std, eps=eps)
    assert none is None and loss.dim() == 0
    loss.backward()
    assert abs(float(loss.detach()) - float(fx["loss"])) <= LOSS_TOL * abs(float(fx["loss"]))
    hn = Harness(family, kind, d, h, nl, act, m.flat_params().detach().cpu(), c)
    s = sigma_rows(std, N).cuda()
    xbar = torch.empty_like(x)
    L.call("ardae_dae_perturb", x, s.contiguous(), eps, N, 1, d, xbar)
    abi_loss, abi_grads, _ = hn.loss_grads(xbar, s, eps, ctx, B, S)
    assert float(loss.detach()) == float(abi_loss)
    for n, p in m.named_parameters():
        if n == "neglogprob.fc.bias":
            assert p.grad is None
        else:
            assert torch.equal(p.grad.cpu(), abi_grads[n]), n
            assert rel(p.grad.cpu(), fx["g/" + n]) <= TENSOR_TOL, n
    glog = m.glogprob(*args)
    assert glog.shape == ((B, S, d) if family.conditional else (N, d))
    if family.plain:
        assert rel(glog.cpu(), fx["glog"]) <= TENSOR_TOL
        assert torch.equal(glog, m.glogprob(*args, 0.7)) and torch.equal(glog, m.glogprob(*args, torch.ones(N, 1, device="cuda")))
        # std=None: self.std; a number and the tensors that broadcast to [N, 1] are the same call
        m.std = 0.37
        a = float(call(eps=eps).detach())
        assert a == float(call(0.37, eps=eps).detach()) != float(loss.detach())
        assert a == float(call(torch.tensor(0.37, device="cuda"), eps=eps).detach()) == float(call(torch.full((N, 1), 0.37, device="cuda"), eps=eps).detach())
        # eps=None: the module's own Philox draw, a fresh one per call
        a, b = float(call(std).detach()), float(call(std).detach())
        assert np.isfinite(a) and np.isfinite(b) and a != b and a != float(loss.detach())
    else:
        assert rel(glog.cpu(), fx["glog0"]) <= TENSOR_TOL and rel(m.glogprob(*args, std).cpu(), fx["glog"]) <= TENSOR_TOL
        # std=None: zeros, so the loss is mean(eps^2) whatever the network says
        loss0 = call(eps=eps)
        assert abs(float(loss0.detach()) - float((eps ** 2).mean())) <= 1e-6 * float((eps ** 2).mean())
        a, b = float(call(std).detach()), float(call(std).detach())                  # the module's own Philox draw, a fresh one per call
        assert np.isfinite(a) and np.isfinite(b) and a != b and a != float(loss.detach())


def check_replay_equals_eager(family, module, cfg, B, S, data, flags, **engine_kw):
    """The steps on `data` (one tuple of step() arguments each) with the graph on and off: every parameter, loss, sigma, xbar and optimiser buffer
    after every step, and the step block at the end, bit for bit.  module: () -> a fresh network; flags: the launch-form attributes the engine
    must show at this shape.  -> the eager engine after the last step."""
    runs, n = [], len(data)
    for graph in (True, False):
        net.manual_seed(77)
        eng = family.engine(module(), cfg, B, *S, graph=graph, **engine_kw)
        assert eng.plain == family.plain and {k: getattr(eng, k) for k in flags} == flags
        trace = []
        for i, batch in enumerate(data):
            eng.step(*batch)
            trace += [getattr(eng, family.key).flat_params().clone(), eng.loss.clone(), eng.sigma.clone(), eng.xbar.clone()] + [b.clone() for b in eng.opt.buffers()]
            if family.plain:
                assert eng.stats()["sigma"] == sigma32(cfg, i) and torch.equal(eng.sigma, torch.full((eng.N,), sigma32(cfg, i), device="cuda"))
        torch.cuda.synchronize()
        assert (eng._graph is not None) == graph
        runs.append(trace + [eng.state.clone()])
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(a, b) for a, b in zip(*runs)), "replayed != eager"
    losses = torch.cat(runs[0][1::4 + len(eng.opt.buffers())][:n])
    assert torch.isfinite(losses).all() and len(set(losses.tolist())) == n          # fresh noise every step
    s = runs[0][-1]
    assert int(s[0]) == STRIDE * (n + 1) and int(s[1]) == n + 1                     # the block describes the coming step
    with pytest.raises(ValueError, match="computes sigma on the device" if family.plain else "inject them through noise"):
        eng.step(*data[0], sigma=0.5)
    assert eng.step_count == n
    return eng


def check_recorded_trajectory(family, golden_dir, kind):
    """A plain family's update on the fixture's samples / eps: every parameter after every step against the reference's fp32 run, and no further
    from its float64 run than max(2 x the fp32 reference's own distance, 2e-6)."""
    fx = load(os.path.join(golden_dir, f"{family.prefix}_traj_{kind}.npz"))
    c = {k[4:]: v for k, v in fx.items() if k.startswith("cfg/")}
    B, ns, d, h, nl, act, steps = int(c["B"]), int(c["nsigma"]), int(c["d"]), int(c["h"]), int(c["L"]), str(c["act"]), int(c["steps"])
    cfg = net.DaeConfig(sigma_max=float(c["sigma_max"]), sigma_min=float(c["sigma_min"]), sigma_annealing=int(c["sigma_annealing"]), nsigma=ns, lr=float(c["lr"]))
    m = family.module(kind, d, h, nl, act, int(c["c"]) if family.conditional else 0)
    m.load_state_dict(state_dict_of(fx))
    if family.conditional:
        eng, names = net.ArdaeCondScoreEngine(m.cuda(), cfg, B, int(c["S"]), std_scale=float(c["std_scale"])), ("latent", "ctx", "mean")
    else:
        eng, names = net.ArdaeScoreEngine(m.cuda(), cfg, B), ("x",)
    bad = []
    for s in range(steps):
        eng.step(*(torch.tensor(fx[f"{s}/{k}"]).cuda() for k in names), noise={"eps": torch.tensor(fx[f"{s}/eps"]).cuda()})
        st = eng.stats()
        assert st["sigma"] == float(np.float32(float(fx[f"{s}/sigma"])))
        assert abs(st["loss"] - float(fx[f"{s}/loss"])) <= LOSS_TOL * abs(float(fx[f"{s}/loss"])), (s, st["loss"])
        for n, p in getattr(eng, family.key).named_parameters():
            p32, p64 = fx[f"{s}/p/{n}"], fx[f"{s}/p_f64/{n}"]
            e32, e64, ref64 = rel(p.detach().cpu(), p32), rel(p.detach().cpu(), p64), rel(p32, p64)
            print(f"{kind} step {s} {n}: to fp32 reference {e32:.2e}, to float64 {e64:.2e} (fp32 reference to float64 {ref64:.2e})")
            if e32 > TENSOR_TOL or e64 > max(2 * ref64, 2e-6):
                bad.append((s, n, e32, e64, ref64))
    assert not bad, bad


def check_drop_in_route(family, kind, d, h, nl, act, c, B, S, ns, batch, n=6, scale=1.0):
    """The same n steps through the engine and through the module + torch.optim with host-computed noise levels; then torch.optim's state loads
    into the engine.  For the plain families and the conditional AR-DAE.  batch: the generator of the noise draws -> the next step()'s arguments,
    (x,) or (latent, ctx, mean).  -> engine, module, that generator."""
    assert family.plain or family.conditional
    if family.plain:
        cfg = net.DaeConfig(sigma_max=1.0, sigma_min=0.1, sigma_annealing=4, nsigma=ns)
    else:
        cfg = net.ScoreConfig(delta=0.1, nsigma=ns, lr=1e-3, optimizer="rmsprop", momentum=0.5)
    kw = dict(std_scale=scale) if family.conditional else {}
    eng = family.engine(fresh_module(family, kind, d, h, nl, act, c), cfg, B, *S, **kw)
    m = fresh_module(family, kind, d, h, nl, act, c)
    opt = torch.optim.Adam(m.parameters(), lr=cfg.lr) if family.plain else torch.optim.RMSprop(m.parameters(), lr=cfg.lr, momentum=0.5)
    g = torch.Generator().manual_seed(5)
    N = eng.N
    for i in range(n):
        args = batch(g)
        xi = torch.randn(N, generator=g).cuda() if family.conditional else None       # (the conditional file draws it for its plain kinds too)
        eps = torch.randn(N, d, generator=g).cuda()
        eng.step(*args, noise={"eps": eps} if family.plain else {"sigma": xi, "eps": eps})
        if family.conditional:
            lat, ctx, mean = args
            u = scale * (lat - mean[:, None, :])
            rows = (u.unsqueeze(2).expand(B, *S, ns, d).reshape(B, S[0] * ns, d), ctx.view(B, 1, c))
            # ivae_ardae.py:753-767: std = delta * mean_d std_S(u), one draw per row
            std = None if family.plain else cfg.delta * u.std(dim=1, keepdim=True).mean(dim=2, keepdim=True).expand(B, S[0] * ns, 1) * xi.view(B, S[0] * ns, 1)
        else:
            rows, std = (args[0].unsqueeze(1).expand(B, ns, d).contiguous().view(N, d),), None
        opt.zero_grad()
        _, loss = m(*rows, net.dae_sigma(1.0, 0.1, 4, i) if family.plain else std, eps=eps)
        loss.backward()
        opt.step()
        assert abs(eng.stats()["loss"] - float(loss.detach())) <= LOSS_TOL * abs(float(loss.detach())), i
        for (name, p), (_, q) in zip(getattr(eng, family.key).named_parameters(), m.named_parameters()):
            assert rel(p.detach().cpu(), q.detach().cpu()) <= TENSOR_TOL, (i, name, rel(p.detach().cpu(), q.detach().cpu()))
    # the two routes' checkpoints are interchangeable: torch.optim's state loads into the engine
    eng.load_state_dict({family.key: m.state_dict(), "optimizer": opt.state_dict()})
    assert eng.step_count == n and eng.state[:2].tolist() == [STRIDE * (n + 1), n + 1]
    if family.plain:
        assert eng.state[3:].view(torch.float32)[0].item() == sigma32(cfg, n)
    return eng, m, g


def check_resume(family, module, cfg, other, B, S, data, at, flags):
    """state_dict() after step `at` into a fresh engine under another library seed: the remaining steps (eager, eager, captured, replayed there)
    leave what the uninterrupted run leaves.  module: seed -> a fresh network; other: a config with another sigma schedule (the plain families)."""
    runs, sd, n = [], None, len(data)
    for resumed in (False, True):
        net.manual_seed(77)
        eng = family.engine(module(21), cfg, B, *S)
        assert {k: getattr(eng, k) for k in flags} == flags
        losses = []
        for i, batch in enumerate(data):
            if resumed and i == at:
                sd = eng.state_dict()
                net.manual_seed(1)                                 # the checkpoint, not the process, carries the RNG state
                eng = family.engine(module(5), cfg, B, *S, graph=True)
                eng.load_state_dict(sd)
                assert eng._graph is None and (eng.step_count, eng.opt.steps) == (at, at)
            eng.step(*batch)
            if family.plain:
                assert eng.stats()["sigma"] == sigma32(cfg, i)
            losses.append(eng.loss.clone())
        torch.cuda.synchronize()
        assert eng._graph is not None
        runs.append([getattr(eng, family.key).flat_params().clone(), eng.state.clone(), eng.sigma.clone(), torch.cat(losses)[at:]] + [b.clone() for b in eng.opt.buffers()])
    assert len(runs[0]) == len(runs[1]) == 4 + len(eng.opt.state_names())
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "the resumed run drifted"
    assert torch.isfinite(runs[0][3]).all() and len(set(runs[0][3].tolist())) == n - at
    assert list(sd) == [family.key, "optimizer", "engine"] and [int(st["step"]) for st in sd["optimizer"]["state"].values()] == [at] * len(sd["optimizer"]["state"])
    if family.plain:      # a checkpoint written under another schedule resumes at THIS engine's value: bytes 24..27 are recomputed from t
        new = family.engine(module(5), other, B, *S)
        new.load_state_dict(sd)
        assert torch.equal(new.state[:3].cpu(), sd["engine"]["step_state"][:3]) and new.state[3:].view(torch.float32)[0].item() == sigma32(other, at)
        new.step(*data[at])
        assert new.stats()["sigma"] == sigma32(other, at) and torch.equal(new.sigma, torch.full((new.N,), sigma32(other, at), device="cuda"))
    # a checkpoint assembled from torch objects has no "engine" entry: the block is rebuilt for the coming step, n = `at` steps done
    del sd["engine"]
    new = family.engine(module(5), cfg, B, *S)
    new.load_state_dict(sd)
    assert new.step_count == at and new.state[:2].tolist() == [STRIDE * (at + 1), at + 1]
    new.step(*data[at])
    assert np.isfinite(new.stats()["loss"]) and new.state[:2].tolist() == [STRIDE * (at + 2), at + 2]
    # an engine holds no reference cycle: it, and its captured graph, is freed where its last reference goes - not by a collector pass at some
    # later time, such as during another engine's capture, where destroying a graph aborts the process
    gone = [weakref.ref(new), weakref.ref(eng)]
    del new, eng
    assert [r() for r in gone] == [None, None], "an engine is kept alive by a reference cycle"


def check_refusals(family, module, sibling_module, B, S, good, wrong_first):
    """What every engine refuses, before anything reaches the device: the other family's config (both ways round), a ragged batch, injected noise
    of the wrong size or on the host, a second source of sigma.  module / sibling_module: () -> a network of `family` / of the family with the
    other config; good: a tuple of step() arguments; wrong_first: the first of them with a row missing.  -> the engine, untouched."""
    right, wrong = ("DaeConfig", "ScoreConfig") if family.plain else ("ScoreConfig", "DaeConfig")
    for mod, cfg, names in ((module, getattr(net, wrong)(), (right, wrong)), (sibling_module, family.config(), (wrong, right))):
        m = mod()
        with pytest.raises(TypeError, match=f"(?s){type(m).__name__}.*{names[0]}.*{names[1]}"):
            family.engine(m, cfg, B, *S)
    eng = family.engine(module(), family.config(nsigma=2), B, *S)
    N, w = eng.N, eng.eps.size(1)
    with pytest.raises(ValueError, match=f"batch_size={B}"):
        eng.step(wrong_first, *good[1:])
    noise = {"sigma": torch.zeros(N, device="cuda"), "eps": torch.zeros(N, w, device="cuda")}
    with pytest.raises(ValueError, match="eps must be"):
        eng.step(*good, noise=dict(noise, eps=torch.zeros(N // 2, w, device="cuda")))      # nsigma forgotten
    with pytest.raises(ValueError, match="eps must be"):
        eng.step(*good, noise=dict(noise, eps=torch.zeros(N, w)))
    if not family.plain:
        with pytest.raises(ValueError, match="sigma must be"):
            eng.step(*good, noise=dict(noise, sigma=torch.zeros(N // 2, device="cuda")))
    with pytest.raises(ValueError, match="computes sigma on the device" if family.plain else "inject them through noise"):
        eng.step(*good, sigma=0.5)
    assert eng.step_count == 0 and eng.opt.steps == 0 and eng.state[:2].tolist() == [STRIDE, 1]
    return eng
