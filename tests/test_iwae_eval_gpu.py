"""IWAE evaluation on the device: the fused proposal kernel and the reduce kernel against float64, the evaluator against the committed
fixtures and against model.logprob, chunking, a degenerate proposal, and ArdaeEngine.evaluate_iws.

Error criterion of the kernel tests (DESIGN section 2's, for gradients): the new path's max-abs error against the float64 formulas may be
at most 3 x that of the fp32 torch glue it replaces (model.logprob's lines, on the same device inputs) plus 1e-6 max|ref|."""
import math
import os

import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from oracle import ardae_oracle as O

pytestmark = pytest.mark.gpu

LOG2PI = math.log(2 * math.pi)


def _within(got, glue, ref, what):
    """got / glue: device fp32 results of the new path / the parent's torch glue; ref: float64 on the CPU."""
    ref = ref.double()
    e_new = float((got.double().cpu() - ref).abs().max())
    e_old = float((glue.double().cpu() - ref).abs().max())
    bound = 3 * e_old + 1e-6 * float(ref.abs().max())
    print(f"{what}: kernel {e_new:.3e}  torch glue {e_old:.3e}  bound {bound:.3e}")
    assert e_new <= bound, (what, e_new, e_old, bound)


# ---- 1. the proposal kernel against float64 ---------------------------------------------------------------------------------------------
def _proposal_ref64(zs, e, jitter):
    """O.iwae_logprob's lines between the sampler and the decoder, float64 on the CPU."""
    zs, e = zs.double().cpu(), e.double().cpu()
    mu = zs.mean(1)
    zc = zs - mu.unsqueeze(1)
    cov = zc.transpose(1, 2) @ zc / (zs.size(1) - 1)
    if jitter:
        cov = cov + jitter * torch.eye(zs.size(2), dtype=cov.dtype)
    Lc = torch.linalg.cholesky(cov)
    newz = mu.unsqueeze(1) + e @ Lc.transpose(1, 2)
    logq = -0.5 * (e ** 2).sum(2) - torch.log(torch.diagonal(Lc, dim1=1, dim2=2)).sum(1, keepdim=True) - 0.5 * zs.size(2) * LOG2PI
    return mu, Lc, newz, logq


def _proposal_glue32(zs, e, jitter):
    """ImplicitPosteriorVAE.logprob's lines (modules.py), fp32 torch on the device with the library's batched factorisation."""
    B, ke, zd = zs.shape
    mu = zs.mean(1)
    zc = zs - mu.unsqueeze(1)
    cov = zc.transpose(1, 2) @ zc / (ke - 1)
    if jitter:
        cov = cov + jitter * torch.eye(zd, device=cov.device)
    cov = cov.contiguous()
    Lc = torch.empty_like(cov)
    L.call("ardae_cholesky_batched", cov, B, zd, Lc)
    newz = (mu.unsqueeze(1) + e @ Lc.transpose(1, 2)).contiguous()
    logq = -0.5 * (e ** 2).sum(2) - torch.log(torch.diagonal(Lc, dim1=1, dim2=2)).sum(1, keepdim=True) - 0.5 * zd * math.log(2 * math.pi)
    return mu, Lc, newz, logq


def _proposal(zs, e, jitter, seed=0, offset=0, first=0, k=None):
    B, ke, zd = zs.shape
    k = e.size(1) if e is not None else k
    new = lambda *s: torch.full(s, float("nan"), device="cuda")                 # noqa: E731
    newz, logq, eps, mu, chol = new(B, k, zd), new(B, k), new(B, k, zd), new(B, zd), new(B, zd, zd)
    L.call("ardae_iwae_proposal", zs, e, B, ke, k, zd, jitter, seed, offset, first, newz, logq, eps, mu, chol)
    return mu, chol, newz, logq, eps


def _inputs(B, ke, k, zd, seed=0):
    g = torch.Generator().manual_seed(seed)
    mix = torch.eye(zd) + 0.1 * torch.randn(zd, zd, generator=g)
    zs = (torch.randn(B, ke, zd, generator=g) @ mix).contiguous()               # well conditioned
    return zs.cuda(), torch.randn(B, k, zd, generator=g).cuda()


SHAPES = [(3, 16, 16, 8), (2, 64, 64, 32), (2, 64, 8, 2), (1, 128, 128, 64), (5, 11, 11, 5)]


@pytest.mark.parametrize("jitter", [0.0, 1e-5])
@pytest.mark.parametrize("B,ke,k,zd", SHAPES)
def test_proposal_kernel_against_float64(B, ke, k, zd, jitter):
    zs, e = _inputs(B, ke, k, zd)
    got = _proposal(zs, e, jitter)
    glue = _proposal_glue32(zs, e, jitter)
    ref = _proposal_ref64(zs, e, jitter)
    assert torch.equal(got[4], e)                                               # eps_out: the e that was used
    assert bool((torch.triu(got[1], 1) == 0).all())
    for name, a, b, r in zip(("mu", "chol", "newz", "logq"), got, glue, ref):
        _within(a, b, r, f"({B}, {ke}, {k}, {zd}) jitter {jitter} {name}")


def test_proposal_outputs_are_optional_and_rows_stream_in_tiles():
    """NULL for eps_out / mu / chol skips them; ke beyond one LDS tile (the auxtoy form at k = 64: 4096 rows of z = 2) and k beyond one tile
    of proposal rows."""
    zs, e = _inputs(2, 4096, 64, 2, seed=3)
    full = _proposal(zs, e, 1e-5)
    newz, logq = torch.empty_like(full[2]), torch.empty_like(full[3])
    L.call("ardae_iwae_proposal", zs, e, 2, 4096, 64, 2, 1e-5, 0, 0, 0, newz, logq, None, None, None)
    assert torch.equal(newz, full[2]) and torch.equal(logq, full[3])
    for name, a, b, r in zip(("mu", "chol", "newz", "logq"), full, _proposal_glue32(zs, e, 1e-5), _proposal_ref64(zs, e, 1e-5)):
        _within(a, b, r, f"(2, 4096, 64, 2) {name}")
    zs, e = _inputs(1, 200, 200, 33, seed=4)                                    # 200 rows of 33: two tiles of 124 proposal rows, 36-column pad
    for name, a, b, r in zip(("mu", "chol", "newz", "logq"), _proposal(zs, e, 0.0), _proposal_glue32(zs, e, 0.0), _proposal_ref64(zs, e, 0.0)):
        _within(a, b, r, f"(1, 200, 200, 33) {name}")


# ---- 2. position independence -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,ke,k,zd", [(3, 16, 16, 8), (3, 64, 8, 2), (3, 11, 11, 5)])
def test_an_images_outputs_do_not_depend_on_the_launch(B, ke, k, zd):
    zs, e = _inputs(B, ke, k, zd, seed=1)
    batch = _proposal(zs, e, 1e-5)
    alone = _proposal(zs[1:2].contiguous(), e[1:2].contiguous(), 1e-5)
    for a, b in zip(batch, alone):
        assert torch.equal(a[1:2], b)


# ---- 3. the in-kernel draw --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,ke,k,zd", [(3, 16, 16, 8), (5, 11, 11, 5), (2, 64, 64, 32)])
def test_in_kernel_draw_is_the_stand_alone_draw(B, ke, k, zd):
    zs, _ = _inputs(B, ke, k, zd, seed=2)
    seed, offset = 0xC0FFEE, net.rng.HOST_STREAM | 77
    for first in (0, 4 * k * zd):
        want = torch.empty(B, k, zd, device="cuda")
        L.call("ardae_philox_normal_at", want, want.numel(), seed, offset, None, first)
        drawn = _proposal(zs, None, 0.0, seed, offset, first, k=k)
        assert torch.equal(drawn[4], want)
        injected = _proposal(zs, want, 0.0)
        for a, b in zip(drawn, injected):                                       # ... and it is used as an injected e would be
            assert torch.equal(a, b)
    # image 1 of a draw at first_element 0 is image 0 of a draw that starts one image later (what a chunked walk relies on)
    if (k * zd) % 4 == 0:
        whole = _proposal(zs, None, 0.0, seed, offset, 0, k=k)
        tail = _proposal(zs[1:].contiguous(), None, 0.0, seed, offset, k * zd, k=k)
        for a, b in zip(whole, tail):
            assert torch.equal(a[1:], b)


# ---- 4. the reduce kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,k", [(4, 16), (3, 300), (5, 11)])
def test_reduce_kernel_against_float64(B, k):
    g = torch.Generator().manual_seed(5)
    rec = (100 + 80 * torch.rand(B, k, generator=g))                            # rows that span 80 nats
    rec[:, 0], rec[:, 1] = 100.0, 180.0
    pri, logq = 3 * torch.randn(B, k, generator=g), 10 + 3 * torch.randn(B, k, generator=g)
    rec[-1], pri[-1], logq[-1] = 1e4, 0.0, 0.0                                  # every row -1e4: exp(lw - max) = 1 beside the 1e-10 floor
    rec, pri, logq = rec.cuda(), pri.cuda(), logq.cuda()
    out = torch.full((B,), float("nan"), device="cuda")
    L.call("ardae_iwae_reduce", rec, pri, logq, B, k, out)

    def formula(rec, pri, logq):                                                # ivae/mnist.py:427-436 as model.logprob writes it
        lw = -rec - pri - logq
        m, _ = lw.max(1, keepdim=True)
        return (torch.log(torch.mean((lw - m).exp(), 1, keepdim=True) + 1e-10) + m).view(-1)

    ref = formula(rec.double().cpu(), pri.double().cpu(), logq.double().cpu())
    assert abs(float(ref[-1]) + 1e4) < 1e-6
    glue = formula(rec, pri, logq)
    _within(out[:-1], glue[:-1], ref[:-1], f"reduce ({B}, {k}) rows over 80 nats")           # apart, so that 1e-6 x 1e4 does not cover the others
    _within(out[-1:], glue[-1:], ref[-1:], f"reduce ({B}, {k}) rows at -1e4")
    rec[1, k // 2] = float("nan")                                                # NaNs propagate, to their image only
    out2 = torch.empty_like(out)
    L.call("ardae_iwae_reduce", rec, pri, logq, B, k, out2)
    assert bool(torch.isnan(out2[1])) and torch.equal(out2[[0] + list(range(2, B))], out[[0] + list(range(2, B))])


# ---- 5. - 8. the evaluator on the committed fixtures ------------------------------------------------------------------------------------
FIXTURES = {"iwae_tiny": O.ModelCfg("mnist", 24, 10, 64, 8, 2, "softplus"),
            "iwae_tiny_auxmnist": O.ModelCfg("auxmnist", 24, 10, 48, 8, 2, "softplus"),
            "iwae_tiny_auxtoy": O.ModelCfg("auxtoy", 2, 2, 32, 2, 2, "tanh")}


def _build(mc):                                                                 # as test_engine_gpu.py builds them
    if mc.kind == "auxtoy":
        return net.ToyAuxIPVAE(input_dim=mc.input_dim, noise_dim=mc.noise_dim, h_dim=mc.h_dim, num_hidden_layers=mc.n_layers, nonlinearity=mc.nonlin,
                               enc_type="simple", z_dim=mc.z_dim, clip_z0_logvar=mc.clip_z0, clip_z_logvar=mc.clip_z)
    if mc.kind == "auxmnist":
        return net.MNISTAuxIPVAE(input_dim=mc.input_dim, noise_dim=mc.noise_dim, h_dim=mc.h_dim, num_hidden_layers=mc.n_layers, nonlinearity=mc.nonlin,
                                 enc_type="simple", z_dim=mc.z_dim, clip_z0_logvar=mc.clip_z0, clip_z_logvar=mc.clip_z)
    return net.MNISTIPVAE(input_dim=mc.input_dim, noise_dim=mc.noise_dim, h_dim=mc.h_dim, num_hidden_layers=mc.n_layers, nonlinearity=mc.nonlin,
                          enc_type="concat", z_dim=mc.z_dim)


_CASES = {}


def _case(golden_dir, name):
    """(mc, model on the device, fixture, k, x, enc_noise, prop_noise); built once per fixture and left unchanged."""
    if name not in _CASES:
        mc = FIXTURES[name]
        fx = dict(np.load(os.path.join(golden_dir, name + ".npz")))
        model = _build(mc)
        model.load_state_dict({n: torch.tensor(fx["pm/" + n]).float() for n, _ in O.model_param_spec(mc)})
        dev = lambda a: torch.tensor(fx[a]).float().cuda()                      # noqa: E731
        enc = (dev("enc_noise"), dev("enc_noise_z")) if "enc_noise_z" in fx else dev("enc_noise")
        _CASES[name] = (mc, model.to("cuda"), fx, int(fx["meta_k"]), dev("x"), enc, dev("prop_noise"))
    return _CASES[name]


def _take(t, idx):
    return tuple(_take(u, idx) for u in t) if isinstance(t, tuple) else t[idx].contiguous()


@pytest.mark.parametrize("name", list(FIXTURES))
def test_evaluate_on_the_committed_fixtures(golden_dir, name):
    mc, model, fx, k, x, enc, prop = _case(golden_dir, name)
    ev = net.IwaeEvaluator(model, k)
    got, ref = ev.evaluate(x, enc, prop), float(fx["logprob"])
    print(f"{name}: evaluate {got!r}  fixture {ref!r}  logprob {float(model.logprob(x, sample_size=k, enc_noise=enc, prop_noise=prop))!r}")
    assert abs(got - ref) < 1e-4 * abs(ref)
    rows = ev.evaluate_rows(x, enc, prop)
    assert rows.shape == (x.size(0),) and rows.is_cuda and abs(float(rows.double().mean()) - got) < 1e-12 * abs(got)
    own = ev.evaluate(x)                                                        # own draws
    assert math.isfinite(own)


def test_rows_against_float64_per_image(golden_dir):
    mc, model, fx, k, x, enc, prop = _case(golden_dir, "iwae_tiny")
    pm = {n: torch.tensor(fx["pm/" + n]).double() for n, _ in O.model_param_spec(mc)}
    rows = net.IwaeEvaluator(model, k).evaluate_rows(x, enc, prop)
    for i in range(x.size(0)):
        s = slice(i, i + 1)
        ref = float(O.iwae_logprob(mc, pm, x[s].double().cpu(), k, enc[s].double().cpu(), prop[s].double().cpu()))
        e_new = abs(float(rows[i]) - ref)
        e_old = abs(float(model.logprob(x[s], sample_size=k, enc_noise=enc[s], prop_noise=prop[s])) - ref)
        print(f"image {i}: ref {ref!r}  evaluate_rows error {e_new:.3e}  model.logprob error {e_old:.3e}")
        assert e_new <= 3 * e_old + 1e-6 * abs(ref)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_result_does_not_depend_on_the_chunks(golden_dir, name):
    mc, model, fx, k, x, enc, prop = _case(golden_dir, name)
    idx = [0, 1, 2, 0, 1, 2, 0]                                                 # N = 7
    x7, enc7, prop7 = _take(x, idx), _take(enc, idx), _take(prop, idx)
    one = net.IwaeEvaluator(model, k)
    two = net.IwaeEvaluator(model, k, max_workspace_floats=one.floats_per_chunk(4))
    assert one.plan(7) == [(0, 7)] and two.plan(7) == [(0, 4), (4, 7)]
    a, b = one.evaluate_rows(x7, enc7, prop7), two.evaluate_rows(x7, enc7, prop7)
    assert torch.equal(a, b)
    net.manual_seed(1234)
    a = one.evaluate_rows(x7)
    net.manual_seed(1234)
    b = two.evaluate_rows(x7)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert not torch.equal(a, one.evaluate_rows(x7))                            # the next call draws anew
    with pytest.raises(ValueError, match="a chunk of 4 images"):
        net.IwaeEvaluator(model, k, max_workspace_floats=one.floats_per_chunk(4) - 1).evaluate_rows(x7)


def test_degenerate_proposal_is_nan_for_its_image_only(golden_dir):
    mc, model, fx, k, x, enc, prop = _case(golden_dir, "iwae_tiny")
    bad = enc.clone()
    bad[1] = enc[1, :1]                                                         # all k encoder samples of image 1 identical: a zero covariance
    ev = net.IwaeEvaluator(model, k)
    rows = ev.evaluate_rows(x, bad, prop)
    assert bool(torch.isnan(rows[1])) and bool(torch.isfinite(rows[[0, 2]]).all())
    with pytest.raises(ValueError, match="not positive definite"):
        ev.evaluate(x, bad, prop)
    assert torch.equal(rows[[0, 2]], ev.evaluate_rows(_take(x, [0, 2]), _take(enc, [0, 2]), _take(prop, [0, 2])))


# ---- 9. the engine ----------------------------------------------------------------------------------------------------------------------
def test_engine_evaluate_iws_uses_the_averaged_weights():
    mc, cc, B, k = O.ModelCfg("mnist", 24, 10, 64, 8, 2, "softplus"), O.CdaeCfg("grad", 8, 8, 64, 3), 8, 16
    model = _build(mc)
    cdae = net.MLPGradCARDAE(input_dim=cc.input_dim, context_dim=cc.context_dim, std=1., h_dim=cc.h_dim, num_hidden_layers=cc.n_layers,
                             nonlinearity=cc.nonlin, noise_type="gaussian", enc_ctx=True, enc_input=True)
    model.load_state_dict(O.init_params(O.model_param_spec(mc), 0, O.model_init_special(mc)))
    cdae.load_state_dict(O.init_params(O.cdae_param_spec(cc), 1))
    model, cdae = model.to("cuda"), cdae.to("cuda")
    net.manual_seed(11)
    cfg = net.TrainConfig(nz_cdae=8, m_lr=1e-2, d_lr=1e-3, m_weight_avg="polyak", m_weight_avg_start=1, m_weight_avg_decay=0.5)
    eng = net.ArdaeEngine(model, cdae, cfg, batch_size=B)
    g = torch.Generator().manual_seed(6)
    batch = lambda: torch.bernoulli(torch.full((B, mc.input_dim), 0.3), generator=g).cuda()      # noqa: E731
    for _ in range(4):
        eng.step(batch(), batch())
    x = torch.bernoulli(torch.full((7, mc.input_dim), 0.3), generator=g).cuda()
    enc, prop = torch.randn(7, k, mc.noise_dim, generator=g).cuda(), torch.randn(7, k, mc.z_dim, generator=g).cuda()
    before = model._flat.clone()
    got = eng.evaluate_iws(x, k, enc, prop)
    assert torch.equal(model._flat, before)                                     # the trained weights are back, bit for bit
    with eng.averaged_weights():
        assert not torch.equal(model._flat, before)
        want = net.IwaeEvaluator(model, k).evaluate(x, enc, prop)
        assert eng.evaluate_iws(x, k, enc, prop) == want                        # inside use_averaged(): what is in, and it stays in
        assert not torch.equal(model._flat, before)
    assert torch.equal(model._flat, before)
    trained = net.IwaeEvaluator(model, k).evaluate(x, enc, prop)
    assert got == want and got != trained
    assert math.isfinite(eng.evaluate_iws(x, k))                                # own draws
    eng.step(batch(), batch())                                                  # ... and training goes on
    assert not torch.equal(model._flat, before) and math.isfinite(eng.stats()["model_loss"])
