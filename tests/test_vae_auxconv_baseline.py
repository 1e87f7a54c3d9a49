"""The hierarchical conv Gaussian baseline (ardae_model_desc.kind 17, the reference's `vae.py --model auxconv`): layout, descriptor rules and argument
validation through the C ABI (ardae_conv_tail included), the module surface, and the float64 torch restatement of the family - three conv trunks on
the same 2x - 1, the two concatenations with the trunk output FIRST, both KLs, the three-stage logprob - that the GPU tests lean on, pinned here to the
reference's float64 fixtures.  No GPU needed.

The fixtures (tools/gen_vae_golden.py, family auxconv) do not store the parameters: `auxconv_params` regenerates them from the stored seed with the
recipe the tool called (oracle.fixture_params.auxconv)."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import layout
from oracle import fixture_params as P
import vae_restate as R
from vae_restate import ACTS, BETAS, TOL64, fails, kld_rows, lin, load, log_normal_rows, pair_kld_rows, rel, relaxed_sample

CASES = ("auxconv_n100_z32_b3", "auxconv_n10_z6_b5_elu")
D = 784


def shape_of(fx):
    """-> (B, noise, z), act"""
    return tuple(int(v) for v in fx["shape"]), str(fx["act"])


def auxconv_params(fx, dtype=torch.float32):
    """The recipe tools/gen_vae_golden.py called: oracle.fixture_params.auxconv (the float64 runs start from the fp32 numbers, widened)"""
    (_, nd, z), _ = shape_of(fx)
    return {k: v.to(dtype) for k, v in P.auxconv(nd, z, int(fx["seed"])).items()}


# ---- the test-side oracle: the family restated in plain torch (trunk and decoder: vae_restate) ---------------------------------------
def stats(p, prefix, act, x, s=None, k=1):
    """-> (mean, logvar) of the network `prefix`: fc on h3 (aux_encode) or on cat[h3, s] with the trunk output first and each image's h3 repeated for
    its k rows of s (encode, aux_decode)"""
    h3 = R.conv_trunk(p, prefix, act, x)
    if s is not None:
        h3 = torch.cat([h3.repeat_interleave(k, 0), s], 1)
    h4 = ACTS[act](lin(p, prefix + "fc", h3))
    return lin(p, prefix + "reparam.mean_fn", h4), lin(p, prefix + "reparam.logvar_fn", h4)


def forward(p, act, x, eps, beta):
    """-> dict(mu0, lv0, z, mean, logit, loss, recon, kld): VAE.forward (vae/auxconv.py:261-288); kld = kld + aux_kld"""
    nd = p["aux_encode.reparam.mean_fn.weight"].size(0)
    mu0, lv0 = stats(p, "aux_encode.", act, x)
    z0 = mu0 + torch.exp(0.5 * lv0) * eps[:, :nd]
    mu, lv = stats(p, "encode.", act, x, z0)
    z = mu + torch.exp(0.5 * lv) * eps[:, nd:]
    mup, lvp = stats(p, "aux_decode.", act, x, z)
    rec, logit = R.conv_recon_rows(p, act, x, z)
    kld, aux = kld_rows(mu, lv), pair_kld_rows(mu0, lv0, mup, lvp)
    return dict(mu0=mu0, lv0=lv0, z=z, mean=torch.sigmoid(logit), logit=logit, loss=(rec + beta * kld + beta * aux).mean(), recon=rec.mean(),
                kld=(kld + aux).mean())


loss_and_grads = functools.partial(R.loss_and_grads, forward)      # (p, act, x, eps, beta, scale=) -> forward's dict (detached), {name: gradient}


def logq_rows(p, act, x, eps):
    """The three stochastic stages of VAE.logprob (vae/auxconv.py:305-339, sample_size2 = 1) on injected draws eps [B, k, noise + z]
    -> z [B k, zd], logq [B k] = log q(z0|x) + log q(z|z0,x) - log r(z0|z,x)"""
    B, k, _ = eps.shape
    nd = p["aux_encode.reparam.mean_fn.weight"].size(0)
    mu0, lv0 = (v.repeat_interleave(k, 0) for v in stats(p, "aux_encode.", act, x))
    e = eps.reshape(B * k, -1)
    z0 = mu0 + torch.exp(0.5 * lv0) * e[:, :nd]
    mu, lv = stats(p, "encode.", act, x, z0, k)
    z = mu + torch.exp(0.5 * lv) * e[:, nd:]
    mup, lvp = stats(p, "aux_decode.", act, x, z, k)
    return z, log_normal_rows(z0, mu0, lv0) + log_normal_rows(z, mu, lv) - log_normal_rows(z0, mup, lvp)


def logprob_rows(p, act, x, eps):
    """VAE.logprob before its mean, [B]"""
    B, k, _ = eps.shape
    z, logq = logq_rows(p, act, x, eps)
    rec, _ = R.conv_recon_rows(p, act, x.repeat_interleave(k, 0), z)
    return R.iw_logsumexp((-rec + log_normal_rows(z, torch.zeros_like(z), torch.zeros_like(z)) - logq).view(B, k))


def tail_logit(p, act, u1):
    """The decoder's last two stages on u1 [R, 8, 8, 32] NHWC (deconv1's activated, zero-padded output) -> logits [R, 784]: stage A, decode.deconv2 +
    activation; stage B, decode.reparam.logit_fn cropped to 28 x 28"""
    hdn = ACTS[act](F.conv_transpose2d(u1.permute(0, 3, 1, 2), p["decode.deconv2.weight"], p["decode.deconv2.bias"], stride=2, padding=2))
    logit = F.conv_transpose2d(hdn, p["decode.reparam.logit_fn.weight"], p["decode.reparam.logit_fn.bias"], stride=2, padding=2)
    return logit[:, :, :28, :28].reshape(-1, D)


def restate(fx):
    """-> the fixture's parameters in float64, cfg (the activation)"""
    return auxconv_params(fx, torch.float64), str(fx["act"])


def trajectory(fx):
    """The fixture's loop restated in float64: yields (step, forward's dict, the parameters after the vendored Adam's step)"""
    p, act = restate(fx)
    return R.trajectory(fx, p, lambda p, x, eps, beta: loss_and_grads(p, act, R.t64(x), R.t64(eps), beta, scale=1.0 / D))


# ---- 1. the restatement, pinned to the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_restatement_is_the_reference_in_float64(golden_dir, case):
    fx = load(golden_dir, "vae_" + case)
    p, act = restate(fx)
    x, eps, dec = (R.t64(fx[k]) for k in ("x", "eps", "dec_noise"))
    for b, beta in BETAS.items():
        out, grads = loss_and_grads(p, act, x, eps, beta, scale=1.0 / D)
        for k in ("z", "mean", "loss", "recon", "kld"):
            assert rel(out[k], fx[f"{b}/{k}_f64"]) <= TOL64, (b, k)
        assert rel(relaxed_sample(out["logit"], dec), fx[f"{b}/x_sample_f64"]) <= TOL64
        assert rel(out["mu0"], fx["mu0_f64"]) <= TOL64 and rel(out["lv0"], fx["lv0_f64"]) <= TOL64
        R.check_grads_f64(grads, fx, b, TOL64, params=p)
    lp = logprob_rows(p, act, x, R.t64(fx["lp/eps"])).mean()
    assert rel(lp, fx["lp/value_f64"]) <= TOL64
    # the fp32 fixture is the same computation at fp32's precision
    assert rel(fx["b1/loss"], fx["b1/loss_f64"]) <= 1e-5 and rel(fx["lp/value"], fx["lp/value_f64"]) <= 1e-5


def test_restated_trajectory_is_the_reference_in_float64(golden_dir):
    fx = load(golden_dir, "vae_traj_auxconv")
    assert int(fx["cfg/steps"]) == 4
    R.check_traj_f64(trajectory(fx), fx, TOL64)
    assert float(fx["1/beta"]) < 1.0 == float(fx["2/beta"]) == float(fx["3/beta"])          # the ramp ends inside the run


# ---- 2. layout -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES + ("traj_auxconv",))
def test_spec_names_and_shapes_are_the_fixtures(golden_dir, name):
    fx = load(golden_dir, "vae_" + name)
    (B, nd, z), act = shape_of(fx)
    spec = layout.aux_conv_vae_spec(nd, z)
    assert [n for n, _ in spec] == [str(n) for n in fx["names"]]
    assert [",".join(str(d) for d in s) for _, s in spec] == [str(s) for s in fx["shapes"]]
    assert spec[0][0] == "aux_encode.conv1.weight" and spec[-1][0] == "aux_decode.reparam.logvar_fn.bias"
    desc = L.ModelDesc(17, D, nd, 800, z, 1, L.ACT[act], 0)
    total = layout.offsets(spec)[1]
    assert total == L.query("ardae_model_param_floats", desc) == sum(v.numel() for v in auxconv_params(fx).values())
    assert L.query("ardae_model_packed_floats", desc) > total
    mod = net.MNISTConvAuxVAE(z0_dim=nd, z_dim=z, nonlinearity=act)
    assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == [(n, tuple(s)) for n, s in spec]
    sd = auxconv_params(fx)
    mod.load_state_dict(sd)
    assert torch.equal(mod.flat_params(), torch.cat([v.reshape(-1) for v in sd.values()]))
    assert (mod._desc.kind, mod._desc.flags, mod._desc.noise_dim, mod._desc.h_dim, mod._desc.n_layers) == (17, 0, nd, 800, 1)


def test_parameter_count_at_the_recipe_widths(golden_dir):
    counts = load(golden_dir, "vae_auxconv_param_counts")
    assert sorted(counts) == ["auxconv_100_32"]
    d = L.ModelDesc(17, D, 100, 800, 32, 1, L.ACT["softplus"], 0)
    assert layout.offsets(layout.aux_conv_vae_spec(100, 32))[1] == L.query("ardae_model_param_floats", d) == int(counts["auxconv_100_32"])
    assert sum(p.numel() for p in net.MNISTConvAuxVAE().parameters()) == int(counts["auxconv_100_32"])
    assert net.modules.KIND_IDS["vae_auxconv"] == 17
    with pytest.raises(NotImplementedError):
        layout.aux_vae_spec("conv", 784, 100, 800, 32, 1)                 # the MLP families' spec stays theirs
    # the z head has kind 11's policy: the tail form, the default wherever it runs
    assert [L.query("ardae_vae_head_fused_ok", L.ModelDesc(17, D, 100, 800, z, 1, 2, 0)) for z in (32, 6, 64, 65)] == [1, 1, 1, 0]


# ---- 3. descriptor rules and refusals, before any HIP call --------------------------------------------------------------------------
one, big, small = ctypes.c_void_p(64), ctypes.c_size_t(1 << 40), ctypes.c_size_t(16)      # any non-null address: validation fails before it is read
ref = ctypes.byref


def desc(**kw):
    return L.ModelDesc(*[kw.get(k, v) for k, v in (("kind", 17), ("input_dim", 784), ("noise_dim", 1), ("h_dim", 800), ("z_dim", 1), ("n_layers", 1),
                                                    ("act", 1), ("flags", 0))])


def test_descriptor_rules():
    lib = L.lib()
    ok = desc()                                                            # the smallest descriptor
    assert lib.ardae_model_param_floats(ref(ok)) > 0 and lib.ardae_model_packed_floats(ref(ok)) > lib.ardae_model_param_floats(ref(ok))
    assert all(lib.ardae_model_workspace_floats(ref(ok), 3, 1, mode) > 0 for mode in (0, 1, 2))
    fails(lib.ardae_model_pack(ref(ok), one, None, None), "null pointer")
    assert lib.ardae_model_param_floats(ref(desc(noise_dim=128, z_dim=200, act=6))) > 0
    for bad, why in ((desc(input_dim=783), "input_dim 784"), (desc(h_dim=300), "h_dim must be 800"), (desc(n_layers=2), "n_layers must be 1"),
                     (desc(noise_dim=0), "noise_dim must be 1 .. 128"), (desc(noise_dim=129), "noise_dim must be 1 .. 128"),
                     (desc(noise_dim=-1), "noise_dim must be 1 .. 128"), (desc(flags=1), "flags must be 0"),
                     (desc(flags=4 << L.MODEL_CLIP_Z0_SHIFT), "flags must be 0"), (desc(z_dim=0), "bad dimensions"), (desc(act=0), "unknown activation"),
                     (desc(act=99), "unknown activation")):
        assert lib.ardae_model_param_floats(ref(bad)) == lib.ardae_model_packed_floats(ref(bad)) == 0
        assert all(lib.ardae_model_workspace_floats(ref(bad), 4, 1, mode) == 0 for mode in (0, 1, 2))
        assert lib.ardae_model_workspace_floats(ref(bad), 4, 16, 4) == 0
        assert lib.ardae_conv_tail_workspace_floats(ref(bad), 4, 2) == 0 and lib.ardae_vae_head_fused_ok(ref(bad)) == 0
        fails(lib.ardae_model_pack(ref(bad), one, one, None), why)
    # 16 is no kind, as 10 and 13 are not; 18 neither
    for k in (16, 18):
        bad = desc(kind=k)
        assert lib.ardae_model_param_floats(ref(bad)) == 0
        fails(lib.ardae_model_pack(ref(bad), one, one, None), "kind must be")
        assert b"17 (MNISTConvAuxVAE)" in lib.ardae_last_error()
        fails(lib.ardae_vae_encode_stats(ref(bad), one, one, one, 4, one, big, one, one, None), "kind must be")
        assert b"17 (MNISTConvAuxVAE)" in lib.ardae_last_error()
    # the workspace modes: one draw per image, no sampler pair; the evaluation pass grows with B and k
    d = desc(noise_dim=10, z_dim=6)
    ws = lambda B, nz, mode: lib.ardae_model_workspace_floats(ref(d), B, nz, mode)      # noqa: E731
    assert ws(4, 2, 0) == ws(4, 2, 1) == ws(4, 1, 3) == 0
    assert ws(4, 1, 1) > ws(4, 1, 0) > 0
    assert 0 < ws(4, 8, 4) < ws(4, 16, 4) < ws(9, 16, 4) < ws(70, 16, 4)
    for per_mode in ([ws(b, 1, mode) for b in (1, 9, 70)] for mode in (0, 1, 2)):
        assert 0 < per_mode[0] < per_mode[1] < per_mode[2]
    # the decode-only carve with the fused tail: no c2 / u2 / c3 - about 16 200 floats per decoded row against kind 11's 51 800
    d11 = L.ModelDesc(11, 784, 0, 800, 6, 1, 1, 0)
    assert ws(1024, 1, 2) / 1024 < 17000 < 51000 < lib.ardae_model_workspace_floats(ref(d11), 1024, 1, 2) / 1024
    assert lib.ardae_conv_tail_workspace_floats(ref(d), 1024, 0) == lib.ardae_conv_tail_workspace_floats(ref(d), 1024, 1) == 0
    assert lib.ardae_conv_tail_workspace_floats(ref(d), 1024, 2) >= 1024 * (64 * 400 + 225 * 16 + 225 * 25 + 784)


def test_argument_validation_of_every_entry_point():
    lib = L.lib()
    fwd = lambda d, x, B, wsf, z, losses: lib.ardae_vae_forward(ref(d), one, one, x, None, B, 1.0, 1.0, 7, 0, None, one, wsf, z, None, losses, None)
    fwd_dev = lambda d, st: lib.ardae_vae_forward_dev(ref(d), one, one, one, None, 4, st, 1.0, 7, 0, None, one, big, one, None, one, None)
    bwd = lambda d, B, wsf, g: lib.ardae_vae_backward(ref(d), one, one, one, B, 1.0, 1.0, one, wsf, g, 0.0, None)
    bwd_dev = lambda d, st: lib.ardae_vae_backward_dev(ref(d), one, one, one, 4, st, 1.0, one, big, one, 0.0, None)
    stats_ = lambda d, B, wsf, mu, lv: lib.ardae_vae_encode_stats(ref(d), one, one, one, B, one, wsf, mu, lv, None)
    head = lambda d, B, variant, mu, eps_out=one: lib.ardae_vae_head(ref(d), one, one, one, None, B, 7, 0, None, variant, mu, one, one, eps_out, one, None)
    draw = lambda d, x, B, k, first, wsf, z, lq, eps=None: lib.ardae_vae_aux_iwae_draw(ref(d), one, one, x, one, one, eps, B, k, 7, 0, 1, first, one, wsf, z, lq,
                                                                                       None, None)
    elbo = lambda d, x, B, first, wsf, rec, kld, eps=None: lib.ardae_vae_aux_elbo_rows(ref(d), one, one, x, eps, B, 7, 0, 1, first, one, wsf, rec, kld, None)
    ok = desc(noise_dim=3, z_dim=5, act=2)
    bad, why = desc(noise_dim=0, z_dim=5), "noise_dim must be"
    for rc in (fwd(bad, one, 4, big, one, one), bwd(bad, 4, big, one), stats_(bad, 4, big, one, one), head(bad, 4, 0, one)):
        fails(rc, why)
    fails(draw(bad, one, 4, 16, 0, big, one, one), why)
    fails(elbo(bad, one, 4, 0, big, one, one), why)
    fails(lib.ardae_model_decode(ref(bad), one, one, one, 4, one, big, one, None, None), why)
    fails(fwd(ok, one, 0, big, one, one), "bad batch")
    fails(fwd(ok, one, -3, big, one, one), "bad batch")
    fails(fwd(ok, one, 4, small, one, one), "workspace too small")
    fails(fwd(ok, None, 4, big, one, one), "null pointer")
    fails(fwd(ok, one, 4, big, None, one), "null pointer")
    fails(fwd(ok, one, 4, big, one, None), "null pointer")
    fails(fwd_dev(ok, None), "beta_state is NULL")
    fails(bwd(ok, 0, big, one), "bad batch")
    fails(bwd(ok, 4, small, one), "workspace too small")
    fails(bwd(ok, 4, big, None), "null pointer")
    fails(bwd_dev(ok, None), "beta_state is NULL")
    fails(stats_(ok, 0, big, one, one), "bad batch")
    fails(stats_(ok, 4, small, one, one), "workspace too small")
    fails(stats_(ok, 4, big, None, one), "null pointer")
    fails(stats_(ok, 4, big, one, None), "null pointer")
    fails(head(ok, 0, 1, one), "bad batch")
    fails(head(ok, 4, 3, one), "variant must be")
    fails(head(ok, 4, 1, None), "null pointer")
    fails(head(ok, 4, 2, one, eps_out=None), "null pointer")
    fails(head(desc(noise_dim=3, z_dim=65), 4, 1, one), "the fused head takes")
    fails(lib.ardae_model_decode(ref(ok), one, one, one, 4, one, small, one, None, None), "workspace too small")
    fails(lib.ardae_model_decode(ref(ok), one, one, None, 4, one, big, one, None, None), "bad arguments")
    # the two aux entry points
    fails(draw(ok, one, 0, 16, 0, big, one, one), "bad batch")
    fails(draw(ok, one, 4, 0, 0, big, one, one), "bad batch")
    fails(draw(ok, one, 1 << 20, 1 << 12, 0, big, one, one), "bad batch")
    fails(draw(ok, one, 4, 16, 0, small, one, one), "workspace too small")
    fails(draw(ok, None, 4, 16, 0, big, one, one), "null pointer")
    fails(draw(ok, one, 4, 16, 0, big, None, one), "null pointer")
    fails(draw(ok, one, 4, 16, 0, big, one, None), "null pointer")
    fails(draw(ok, one, 4, 3, 1, big, one, one), "multiples of 4")                        # 1 x 3 x 3 normals before the chunk: no whole counter
    fails(draw(ok, one, 4, 3, 1, small, one, one, eps=one), "workspace too small")        # ... which injected draws do not need
    fails(draw(desc(noise_dim=3, z_dim=129), one, 4, 16, 0, big, one, one), "z_dim <= 128")
    fails(elbo(ok, one, 0, 0, big, one, one), "bad batch")
    fails(elbo(ok, one, 4, 0, small, one, one), "workspace too small")
    fails(elbo(ok, None, 4, 0, big, one, one), "null pointer")
    fails(elbo(ok, one, 4, 0, big, None, one), "null pointer")
    fails(elbo(ok, one, 4, 0, big, one, None), "null pointer")
    fails(elbo(ok, one, 4, 2, big, one, one), "multiples of 4")
    # their kind message keeps the earlier fragment and names the new kind
    for other in (L.ModelDesc(11, 784, 0, 800, 4, 1, 2, 0), L.ModelDesc(4, 784, 3, 800, 4, 1, 2, 0), desc(kind=16)):
        for rc in (draw(other, one, 4, 16, 0, big, one, one), elbo(other, one, 4, 0, big, one, one)):
            fails(rc, "kind must be 14 (MNISTAuxVAE) or 15 (ToyAuxVAE) or 17 (MNISTConvAuxVAE)")
    # the implicit models' calls refuse the family: there is no sampler
    fails(lib.ardae_model_encode(ref(ok), one, one, one, None, 4, 1, one, big, one, None), "analytic posterior")
    fails(lib.ardae_model_vae_forward(ref(ok), one, one, one, one, 4, 1, 1.0, one, big, one, one, None), "ardae_vae_forward")
    fails(lib.ardae_model_vae_backward(ref(ok), one, one, one, one, 4, 1, 1.0, 1.0, None, one, big, one, 0.0, None), "ardae_vae_backward")
    fails(lib.ardae_model_vae_backward_decoder(ref(ok), one, one, one, one, 4, 1, 1.0, 1.0, one, big, None), "no split backward")
    fails(lib.ardae_model_encode_hidden(ref(ok), one, one, one, 4, one, big, one, None, None), "hidden1a context")


def test_argument_validation_of_conv_tail():
    lib = L.lib()
    tail = lambda d, R, variant, u1=one, ws=one, wsf=big, out=one, params=one: lib.ardae_conv_tail(ref(d), params, one, u1, R, variant, ws, wsf, out, None)
    ok = desc(noise_dim=3, z_dim=5, act=2)
    fails(lib.ardae_conv_tail(None, one, one, one, 4, 1, one, big, one, None), "desc is NULL")
    for variant in (-1, 3):
        fails(tail(ok, 4, variant), "variant must be")
        assert lib.ardae_conv_tail_workspace_floats(ref(ok), 4, variant) == 0
    for R in (0, -2, 1 << 20):
        fails(tail(ok, R, 1), "bad batch")
        assert lib.ardae_conv_tail_workspace_floats(ref(ok), R, 2) == 0
    fails(tail(ok, 4, 1, u1=None), "null pointer")
    fails(tail(ok, 4, 1, out=None), "null pointer")
    fails(tail(ok, 4, 1, params=None), "null pointer")
    fails(tail(ok, 4, 2, ws=None), "need a workspace")                    # variant 2 without a workspace
    fails(tail(ok, 4, 2, wsf=small), "workspace too small")
    fails(tail(desc(noise_dim=3, z_dim=5, act=0), 4, 1), "unknown activation")
    for other in (L.ModelDesc(11, 784, 0, 800, 5, 1, 2, 0), L.ModelDesc(4, 784, 3, 800, 5, 1, 2, 0), L.ModelDesc(2, 784, 3, 800, 5, 1, 2, 0)):
        fails(tail(other, 4, 1), "kind must be 17 (MNISTConvAuxVAE)")
        assert lib.ardae_conv_tail_workspace_floats(ref(other), 4, 2) == 0


# ---- 4. the module surface -----------------------------------------------------------------------------------------------------------
def test_module_surface_and_refusals():
    torch.manual_seed(0)
    m = net.MNISTConvAuxVAE()
    assert (m.input_height, m.input_channels, m.z0_dim, m.noise_dim, m.h_dim, m.z_dim, m.nonlinearity, m.do_xavier, m.do_m5bias, m.input_dim) == \
        (28, 1, 100, 100, 800, 32, "softplus", True, False, 784)
    assert isinstance(m, net.GaussianVAE) and m.latent_dim == 32 and m._eps_width == 132 and m.return_samples and m._eval_groups[0] % 4 == 0
    p = {k: v.detach() for k, v in m.named_parameters()}
    # do_xavier (the default here): weight_init on Conv2d / Linear - xavier-uniform weights, zero biases; ConvTranspose2d keeps torch's default
    for k, v in p.items():
        if k.endswith("bias") and "deconv" not in k and "logit_fn" not in k:
            assert float(v.abs().max()) == 0.0, k
    for k, fan in (("aux_encode.conv2.weight", (16 + 32) * 25), ("encode.fc.weight", 612 + 800), ("aux_decode.fc.weight", 544 + 800),
                   ("aux_decode.reparam.logvar_fn.weight", 800 + 100), ("decode.fc.fc.weight", 300 + 512)):
        bound = math.sqrt(6.0 / fan)
        assert 0.9 * bound < float(p[k].abs().max()) <= bound, k
    for k, fan_in in (("decode.deconv1", 32 * 25), ("decode.deconv2", 16 * 25)):
        bound = 1.0 / math.sqrt(fan_in)
        assert 0.9 * bound < float(p[k + ".weight"].abs().max()) <= bound and 0.0 < float(p[k + ".bias"].abs().max()) <= bound, k
    assert abs(float(p["decode.reparam.logit_fn.bias"])) <= 1.0 / 5
    m5 = net.MNISTConvAuxVAE(z0_dim=5, z_dim=4, do_xavier=False, do_m5bias=True, nonlinearity="elu")
    q = {k: v.detach() for k, v in m5.named_parameters()}
    assert float(q["decode.reparam.logit_fn.bias"]) == -5.0 and float(q["aux_decode.fc.bias"].abs().max()) > 0.0
    assert float(q["encode.fc.weight"].abs().max()) <= 1.0 / math.sqrt(517)
    with pytest.raises(NotImplementedError, match="28x28x1"):
        net.MNISTConvAuxVAE(input_height=32)
    with pytest.raises(NotImplementedError, match="28x28x1"):
        net.MNISTConvAuxVAE(input_channels=2)
    with pytest.raises(NotImplementedError, match="nonlinearity"):
        net.MNISTConvAuxVAE(nonlinearity="gelu")
    with pytest.raises(NotImplementedError, match="normal_energy_func"):
        net.MNISTConvAuxVAE(energy_func=lambda z: z.sum(1))
    for bad in (0, 129):
        with pytest.raises(ValueError, match="noise_dim must be 1 .. 128"):
            net.MNISTConvAuxVAE(z0_dim=bad)
    for call in (lambda: m5(torch.zeros(3, 784)), lambda: m5(torch.zeros(3, 1, 28, 28)), lambda: m5.logprob(torch.zeros(3, 784), sample_size=4),
                 lambda: m5.logprob_rows(torch.zeros(3, 784), 4), lambda: m5.encode_stats(torch.zeros(3, 784)), lambda: m5.generate(2),
                 lambda: m5.decode_params(torch.zeros(3, 4))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    with pytest.raises(RuntimeError, match="no CPU path"):
        net.VaeEngine(m5, net.VaeConfig(), batch_size=4)
    # the engine / evaluator type checks keep naming the existing classes in order, and name the new one
    with pytest.raises(TypeError, match="VaeEngine drives.*net.MNISTVAE / net.ToyVAE / net.MNISTConvVAE / net.MNISTResConvVAE.*net.MNISTAuxVAE / "
                                        "net.ToyAuxVAE / net.MNISTConvAuxVAE"):
        net.VaeEngine(net.MNISTConvAuxIPVAE(), net.VaeConfig(), batch_size=4)
    with pytest.raises(TypeError, match="net.MNISTVAE / net.ToyVAE / net.MNISTConvVAE / net.MNISTResConvVAE.*net.ToyAuxVAE / net.MNISTConvAuxVAE"):
        net.GaussianIwaeEvaluator(net.MNISTConvAuxIPVAE(), 16)
    with pytest.raises(NotImplementedError, match="z_dim 129 > 128"):
        net.GaussianIwaeEvaluator(net.MNISTConvAuxVAE(z0_dim=5, z_dim=129), 16)


def test_evaluator_plans_whole_groups_within_the_default_budget():
    ev = net.GaussianIwaeEvaluator(net.MNISTConvAuxVAE(), 256)
    assert ev.aux and ev.sd == 100 and not ev.gaussian
    G, g = ev.image_group, ev.group
    assert (G, g) == net.MNISTConvAuxVAE._eval_groups and G % g == 0 and g % 4 == 0
    plan = ev.plan(2048)
    assert plan[0][0] == 0 and plan[-1][1] == 2048 and all(a[1] == b[0] for a, b in zip(plan, plan[1:]))
    assert all((b - a) % G == 0 for a, b in plan[:-1]) and ev.floats_per_chunk(plan[0][1]) <= ev.budget == 1 << 28
    # the group of the importance samples' decoder is sized from the fused tail's carve: twice the group would not fit the budget
    d = ev.model._desc
    assert L.query("ardae_model_workspace_floats", d, g * 256, 1, 2) < ev.budget < L.query("ardae_model_workspace_floats", d, 2 * g * 256, 1, 2) + 2 * g * 256 * 784
    small = net.GaussianIwaeEvaluator(ev.model, 256, max_workspace_floats=ev.floats_per_chunk(150))
    assert [b - a for a, b in small.plan(300)] == [64, 64, 64, 64, 44]       # cut down to whole groups
    with pytest.raises(ValueError, match="one group of 64 images"):
        net.GaussianIwaeEvaluator(ev.model, 256, max_workspace_floats=ev.floats_per_chunk(40)).plan(100)
    assert net.GaussianIwaeEvaluator(ev.model, 256, max_workspace_floats=ev.floats_per_chunk(12)).plan(12) == [(0, 12)]
