"""The conv Gaussian-posterior baseline on the device (ardae_model_desc.kind 11; vae.py --model conv): forward / backward against the
reference's fixtures through the C ABI and through autograd, shapes the fixtures do not reach against the float64 restatement of
tests/test_vae_conv_baseline.py with NaN-filled buffers and guard rows, the Gaussian head at h = 800, the engine's trajectory, replay == eager,
resume, IWAE evaluation, the drop-in route.

The bodies these tests share with the other Gaussian families, and the tolerances, are tests/vae_gpu_checks.py's."""
import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
import vae_gpu_checks as G
import vae_restate as R
from vae_gpu_checks import DEV, TOL_LATENT, TOL_LOSS, TOL_PARAM, check_guard, check_losses, guarded, head, rel, relerr
from test_vae_conv_baseline import CASES, D, fixture_params, logprob_rows, loss_and_grads, restate, trajectory

pytestmark = pytest.mark.gpu


def build(z, act, sd=None, **kw):
    m = net.MNISTConvVAE(z_dim=z, nonlinearity=act, **kw)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV)


def from_fixture(fx):
    return build(int(fx["shape"][1]), str(fx["act"]), fixture_params(fx))


# this family's fused head is the default at every z <= 64 (README)
FAMILY = G.Family(from_fixture=from_fixture, restate=restate, loss_and_grads=loss_and_grads, logprob_rows=logprob_rows, image=True, fixture_grads="norm",
                  grads64=True, traj="restate", trajectory=trajectory, head_fused=1, logprob_is_evaluator=True)


# ---- 1. both fixtures, both betas --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_forward_backward_against_the_reference(golden_dir, case):
    G.forward_backward_against_the_reference(FAMILY, golden_dir, f"vae_conv_{case}", f"conv {case}")


# ---- 2. shapes the fixtures do not reach, against the float64 restatement ----------------------------------------------------------
@pytest.mark.parametrize("B,z,act", [(1, 32, "softplus"), (9, 32, "softplus"), (70, 6, "tanh")])
def test_other_batches_against_the_float64_restatement_with_guard_rows(B, z, act):
    """B = 1; one row past the head's 8-row tile; past a 64-row tile with the unaligned head.  Every buffer starts as NaN, so a read of something
    never written shows in the results, and nothing past B rows of any caller buffer (or past the workspace's declared size) may be written."""
    torch.manual_seed(100 + B)
    m = build(z, act)
    x, eps = torch.bernoulli(torch.full((B, D), 0.3)), torch.randn(B, z)
    out, zc = G.against_the_float64_restatement(FAMILY, m, act, x, eps, [(beta, f"conv B={B} z={z} beta {beta}") for beta in (1.0, 0.3)])
    # encode_stats, the head alone, decode: the same guards
    mu, lv = G.abi_encode_stats(m, x.to(DEV), z)
    assert rel(mu.cpu(), out["mu"]) <= TOL_LATENT and rel(lv.cpu(), out["lv"]) <= TOL_LATENT
    hid = torch.nn.functional.softplus(torch.randn(B, 800)).to(DEV).contiguous()
    for variant in (1, 2):
        o = [guarded(B, z) for _ in range(4)] + [guarded(B, 1)]
        L.call("ardae_vae_head", m._desc, m._flat, m._packed_weights(), hid, eps.to(DEV), B, 7, 0, None, variant, o[0], o[1], o[2], o[3], o[4])
        for buf, what in zip(o, G.HEAD_KEYS):
            check_guard(buf, B, f"head variant {variant} {what}")
    logit, _ = G.abi_decode(m, zc)
    assert rel(logit.cpu(), out["logit"]) <= TOL_LATENT


# ---- 3. the head at h = 800 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,z", [(9, 32), (5, 6)])
def test_head_variants_at_h_800(B, z):
    """Variant 1 (this family's fused head: the two products on the MFMA linears, then ONE launch for the draw, the reparameterisation and the KL
    rows) against variant 2 (the five unfused launches) on 800-wide hidden rows, own draw and injected eps: both against float64 on the host, and
    eps / mu / lv / z / kld bit for bit.  The figures are printed before the last assertion.  (gauss_head_kernel, the fused head of kinds 8 / 9,
    adds one FMA chain per output where the MFMA linears split k over four waves: it agrees with the unfused launches to 2.8 - 7.6e-7 relative
    L2 here, not to the bit, and took 51.0 us against their 19.8 at 128 x 800 -> 2 x 32 - which is why this family's fused head keeps the linears.)"""
    torch.manual_seed(B)
    m = build(z, "softplus")
    # the default is what the README says it is for this family: its fused head, at every z <= 64
    assert L.query("ardae_vae_head_fused_ok", m._desc) == 1
    hid = torch.nn.functional.softplus(torch.randn(B, 800)).to(DEV).contiguous()
    draw = G.philox_normal((B, z), 123, 5)
    given = torch.randn(B, z).to(DEV)
    mu, lv = G.head64(m, hid)
    equal = True
    for eps, used in ((None, draw), (given, given)):
        fused, unfused = head(m, hid, 1, eps), head(m, hid, 2, eps)
        assert torch.equal(fused["eps"], used) and torch.equal(unfused["eps"], used)
        for name, v in (("fused", fused), ("unfused", unfused)):      # both against float64 on the host
            G.check_head64(v, mu, lv, used, name)
        for k in ("mu", "lv", "z", "kld"):
            share = float((fused[k] == unfused[k]).float().mean())
            print(f"head B={B} h=800 z={z} {'own draw' if eps is None else 'injected'} {k}: rel L2 {rel(fused[k].cpu(), unfused[k].cpu()):.3g}, "
                  f"bit-identical {100 * share:.1f} %")
            equal = equal and torch.equal(fused[k], unfused[k])
        auto = head(m, hid, 0, eps)
        assert all(torch.equal(auto[k], fused[k]) for k in G.HEAD_KEYS)
    assert equal, "variant 1 and variant 2 differ in at least one bit (figures above)"


# ---- 4. the engine -------------------------------------------------------------------------------------------------------------------
def test_engine_trajectory_against_the_reference(golden_dir):
    G.engine_trajectory_against_the_reference(FAMILY, golden_dir, "vae_traj_conv", "conv", steps=4)


@pytest.mark.parametrize("avg", ["none", "polyak"])
def test_replay_equals_eager_and_resume_continues_to_the_same_bits(avg):
    B, z = 8, 8
    torch.manual_seed(3)
    sd0 = {k: v.clone() for k, v in build(z, "softplus").state_dict().items()}
    g = torch.Generator().manual_seed(4)
    xs = [torch.bernoulli(torch.full((B, D), 0.3), generator=g).to(DEV) for _ in range(6)]
    cfg = net.VaeConfig(lr=1e-3, beta_init=1e-4, beta_fin=1.0, beta_annealing=10, weight_avg=avg, weight_avg_start=1)
    G.replay_equals_eager_and_resume(lambda: build(z, "softplus", sd0), xs, cfg, resume_at=4)       # a fresh engine continues for 2 steps


def test_one_rmsprop_step_against_the_restatement():
    B, z = 5, 8
    torch.manual_seed(12)
    m = build(z, "softplus")
    p64 = FAMILY.p64_of(m)
    x, eps = torch.bernoulli(torch.full((B, D), 0.3)), torch.randn(B, z)
    eng = net.VaeEngine(m, net.VaeConfig(optimizer="rmsprop", lr=1e-3, momentum=0.5, beta_fin=0.7), batch_size=B)
    eng.step(x.to(DEV), eps=eps.to(DEV))
    out, grads = loss_and_grads(p64, "softplus", x.double(), eps.double(), 0.7, scale=1.0 / D)
    params = [v.clone().requires_grad_(True) for v in p64.values()]
    opt = torch.optim.RMSprop(params, lr=1e-3, momentum=0.5)            # vae.py:323-324
    for v, name in zip(params, p64):
        v.grad = grads[name]
    opt.step()
    st = eng.stats()
    check_losses((st["loss"], st["recon"], st["kld"]), out, "conv rmsprop step")
    worst = max(rel(q.detach().cpu(), v.detach()) for q, v in zip(m.parameters(), params))
    print(f"conv rmsprop step: worst parameter tensor against float64 {worst:.3g}")
    assert worst <= TOL_PARAM and st["beta"] == float(np.float32(0.7))


# ---- 5. evaluate_iws -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_iwae_on_injected_draws_against_the_float64_fixture(golden_dir, case):
    G.iwae_on_injected_draws(FAMILY, golden_dir, f"vae_conv_{case}", f"conv {case}")


def test_iwae_does_not_depend_on_the_chunking():
    """One chunk of 208 images against chunks of 64: the two lengths lie on either side of the row counts at which the library changes the
    kernel of the trunk's linears (conv1 leaves the small-M kernel above 83 images per call).  The evaluator calls the encoder and the ELBO
    pass's decoder on 64 images and the importance samples' decoder on 16 under either plan, so everything is equal to the bit."""
    torch.manual_seed(8)
    m = build(8, "softplus")
    N, k = 208, 16                                 # three whole groups of 64 images and a tail of 16
    x = torch.bernoulli(torch.full((N, D), 0.3)).to(DEV)
    eps, fwd_eps = torch.randn(N, k, 8).to(DEV), torch.randn(N, 8).to(DEV)
    assert m._eval_groups == (64, 16)
    # two budgets, two chunk lengths (whole groups under a budget of 100 images)
    G.iwae_does_not_depend_on_the_chunking(FAMILY, m, x, k, [(208, [208]), (100, [64, 64, 64, 16])], eps, fwd_eps)
    # what the groups are for: the encoder on all 208 images in one call takes other kernels than on 64 (printed, not asserted: rounding)
    mu_all, mu_64 = m.encode_stats(x)[0], torch.cat([m.encode_stats(x[i:i + 64].contiguous())[0] for i in range(0, N, 64)])
    print(f"encode_stats on 208 images at once against 64 per call: bit-identical {100 * float((mu_all == mu_64).float().mean()):.1f} %")


# ---- 6. drop-in ----------------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_and_generate():
    torch.manual_seed(5)
    a = build(8, "softplus", do_xavier=True, do_m5bias=True)
    b = build(8, "softplus")
    assert not torch.equal(a.flat_params(), b.flat_params())
    b.load_state_dict({k: v.cpu() for k, v in a.state_dict().items()})
    assert torch.equal(a.flat_params(), b.flat_params())
    net.manual_seed(5)
    xs, mean, z = b.generate(7)
    assert xs.shape == mean.shape == (7, D) and z.shape == (7, 8)
    assert all(bool(torch.isfinite(t).all()) for t in (xs, mean, z))
    x = torch.bernoulli(torch.full((3, D), 0.3)).to(DEV)
    eps = torch.randn(3, 8).to(DEV)
    la, lb = a(x, eps=eps)[3], b(x.view(3, 1, 28, 28), eps=eps)[3]
    assert torch.equal(la.detach(), lb.detach())
    # the decoder's sample of forward() is the relaxed Bernoulli of its logits on the injected uniform draw
    u = torch.rand(3, D).to(DEV)
    xs, mean, zz, _, _, _ = b(x, eps=eps, dec_noise=u)
    logit = b.decode_params(zz)[0]
    assert rel(xs.cpu(), R.relaxed_sample(logit.double().cpu(), u.double().cpu())) <= 1e-4 and rel(mean.cpu(), torch.sigmoid(logit.double().cpu())) <= TOL_LATENT


# ---- 7. the shared decoder's backward at an activation with act'(0) != 0, on the family that owned it ---------------------------------
@pytest.mark.parametrize("act", ["tanh", "elu"])
def test_conv_implicit_model_gradients_at_tanh_and_elu(act):
    """ConvIPVAE (kind 2) runs the decoder this family shares.  ZeroPad2d after deconv1 passes no gradient; conv_decoder_bwd used to multiply the
    gradient there by act'(0), which is 0 for the relu / softplus every earlier test of kinds 2 / 4 uses and 1 for tanh / elu.  Every gradient
    tensor against a float64 restatement of models/ivae/conv.py (the trunk, fc4 on [h3 | noise], fc5, this file's decoder, N(0, I) energy)."""
    B, nz, nd, z, beta = 3, 2, 5, 8, 0.7
    torch.manual_seed(31)
    m = net.ConvIPVAE(z_dim=z, noise_dim=nd, nonlinearity=act).to(DEV)
    m.return_samples = False
    x, noise = torch.bernoulli(torch.full((B, D), 0.3)), torch.randn(B * nz, nd)
    p = {k: v.clone().requires_grad_(True) for k, v in FAMILY.p64_of(m).items()}
    h3 = R.conv_trunk(p, "encode.", act, x.double())
    t1 = R.ACTS[act](R.lin(p, "encode.fc4", torch.cat([h3.repeat_interleave(nz, 0), noise.double()], 1)))
    zz = R.lin(p, "encode.fc5", t1)
    rec, _ = R.conv_recon_rows(p, act, x.double().repeat_interleave(nz, 0), zz)
    want = (rec + beta * 0.5 * (zz ** 2 + R.LOG_2PI).sum(1)).mean()
    g64 = dict(zip(p, torch.autograd.grad(want / D, list(p.values()))))
    _, _, zd, loss, _, _ = m(x.to(DEV), beta=beta, nz=nz, noise=noise.to(DEV))
    (loss / float(D)).backward()
    assert rel(zd.reshape(B * nz, z).cpu(), zz.detach()) <= TOL_LATENT and relerr(loss.detach(), want.detach()) <= TOL_LOSS
    G.check_grads64(m, [q.grad for q in m.parameters()], g64, f"ConvIPVAE {act}")
