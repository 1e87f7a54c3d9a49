"""The conv Gaussian-posterior baseline (ardae_model_desc.kind 11, the reference's `vae.py --model conv`): layout, initialisation, argument
validation of kind 11 at every entry point, refusals of the module, and the float64 restatement of the family (F.conv2d / F.conv_transpose2d,
padding and crop as models/vae/conv.py) that the GPU tests lean on - pinned here to the reference's float64 fixtures.  No GPU needed.

The fixtures (tools/gen_vae_golden.py, family conv) do not store the 703 405 parameters: `conv_params` regenerates them from the stored seed
with the recipe the tool called (oracle.fixture_params.conv)."""
import ctypes
import functools
import math

import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import layout
from oracle import fixture_params as P
import vae_restate as R
from vae_restate import BETAS, TOL64, fails, lin, load, rel, relaxed_sample

CASES = ("z32_b3", "z6_b5")
D = 784


conv_params = P.conv      # (z, seed, special, dtype=): the recipe tools/gen_vae_golden.py loaded into the reference class


def fixture_params(fx, dtype=torch.float32):
    """(the float64 runs of the tool start from the fp32 numbers, widened)"""
    return {k: v.to(dtype) for k, v in conv_params(int(fx["shape"][1]), int(fx["seed"]), bool(int(fx["special"]))).items()}


# ---- the test-side oracle: the family restated in plain torch (trunk and decoder: vae_restate) ---------------------------------------
def encode(p, act, x):
    """Encoder.forward up to the statistics (vae/conv.py:59-72)"""
    hdn = R.ACTS[act](lin(p, "encode.fc", R.conv_trunk(p, "encode.", act, x)))
    return lin(p, "encode.reparam.mean_fn", hdn), lin(p, "encode.reparam.logvar_fn", hdn)


def forward(p, act, x, eps, beta):
    """-> dict(mu, lv, z, mean, logit, loss, recon, kld): VAE.forward (vae/conv.py:170-201)"""
    mu, lv = encode(p, act, x)
    z = mu + torch.exp(0.5 * lv) * eps
    kld = R.kld_rows(mu, lv)
    rec, logit = R.conv_recon_rows(p, act, x, z)
    return dict(mu=mu, lv=lv, z=z, mean=torch.sigmoid(logit), logit=logit, loss=(rec + beta * kld).mean(), recon=rec.mean(), kld=kld.mean())


loss_and_grads = functools.partial(R.loss_and_grads, forward)      # (p, act, x, eps, beta, scale=) -> forward's dict (detached), {name: gradient}


def logprob_rows(p, act, x, eps):
    """VAE.logprob before its mean (vae/conv.py:218-257) on injected draws eps [B, k, zd]"""
    return R.gaussian_logprob_rows(*encode(p, act, x), x, eps, lambda xr, zr: R.conv_recon_rows(p, act, xr, zr)[0])


def restate(fx):
    """-> the fixture's parameters in float64, cfg (the activation)"""
    return fixture_params(fx, torch.float64), str(fx["act"])


def trajectory(fx):
    """The fixture's loop restated in float64: yields (step, forward's dict, the parameters after the vendored Adam's step)"""
    p, act = restate(fx)
    return R.trajectory(fx, p, lambda p, x, eps, beta: loss_and_grads(p, act, R.t64(x), R.t64(eps), beta, scale=1.0 / D))


# ---- 1. layout, initialisation -----------------------------------------------------------------------------------------------------
def test_layout_is_the_reference_state_dict(golden_dir):
    for name, z in (("vae_conv_z32_b3", 32), ("vae_conv_z6_b5", 6), ("vae_traj_conv", 32)):
        fx = load(golden_dir, name)
        assert int(fx["shape"][1]) == z
        ref = [(str(n), tuple(int(v) for v in str(s).split(","))) for n, s in zip(fx["names"], fx["shapes"])]
        spec = layout.conv_vae_spec(z)
        assert [(n, tuple(s)) for n, s in spec] == ref
        desc = L.ModelDesc(11, D, 0, 800, z, 1, L.ACT[str(fx["act"])], 0)
        total = layout.offsets(spec)[1]
        assert total == L.query("ardae_model_param_floats", desc) == sum(v.numel() for v in fixture_params(fx).values())
        assert L.query("ardae_model_packed_floats", desc) > total
        mod = net.MNISTConvVAE(z_dim=z, nonlinearity=str(fx["act"]))
        assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == ref
        assert (mod.input_dim, mod.h_dim, mod.latent_dim, mod.z_dim, mod.noise_dim) == (D, 800, z, z, 0)
        sd = fixture_params(fx)
        mod.load_state_dict(sd)
        assert torch.equal(mod.flat_params(), torch.cat([v.reshape(-1) for v in sd.values()]))
    counts = load(golden_dir, "vae_conv_param_counts")
    d32 = L.ModelDesc(11, D, 0, 800, 32, 1, L.ACT["softplus"], 0)
    assert layout.offsets(layout.conv_vae_spec(32))[1] == L.query("ardae_model_param_floats", d32) == int(counts["conv_32"])
    sizes = [[L.query("ardae_model_workspace_floats", d32, b, 1, mode) for b in (1, 9, 70)] for mode in (0, 1, 2)]
    for per_mode in sizes:
        assert 0 < per_mode[0] < per_mode[1] < per_mode[2]
    assert all(a < b for a, b in zip(sizes[0], sizes[1]))               # the training workspace holds the encoder's and more
    with pytest.raises(NotImplementedError):
        layout.vae_spec("conv", 784, 800, 32, 1)                         # the MLP families' spec stays theirs


def test_initialisation_of_do_xavier_and_do_m5bias():
    torch.manual_seed(0)
    m = net.MNISTConvVAE(z_dim=8, do_xavier=True, do_m5bias=True)
    p = {k: v.detach() for k, v in m.named_parameters()}
    assert float(p["decode.reparam.logit_fn.bias"]) == -5.0
    for k, v in p.items():
        if "deconv" in k or "logit_fn" in k:
            continue
        if k.endswith("bias"):
            assert float(v.abs().max()) == 0.0, k
    for k, fan in (("encode.conv2.weight", (16 + 32) * 25), ("encode.fc.weight", 512 + 800), ("decode.fc.fc.weight", 300 + 512)):
        bound = math.sqrt(6.0 / fan)                                    # xavier-uniform
        assert 0.9 * bound < float(p[k].abs().max()) <= bound, k
    # ConvTranspose2d keeps torch's default: U(+-1 / sqrt(fan_in)), fan_in = weight.size(1) * 25, biases not zeroed
    for k, fan_in in (("decode.deconv1", 32 * 25), ("decode.deconv2", 16 * 25)):
        bound = 1.0 / math.sqrt(fan_in)
        assert 0.9 * bound < float(p[k + ".weight"].abs().max()) <= bound and 0.0 < float(p[k + ".bias"].abs().max()) <= bound, k
    plain = {k: v.detach() for k, v in net.MNISTConvVAE(z_dim=8).named_parameters()}
    assert float(plain["encode.fc.bias"].abs().max()) > 0.0 and float(plain["encode.fc.weight"].abs().max()) <= 1.0 / math.sqrt(512)
    assert abs(float(plain["decode.reparam.logit_fn.bias"])) <= 1.0 / 5


# ---- 2. the float64 restatement, pinned to the reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_restatement_is_the_reference_in_float64(golden_dir, case):
    fx = load(golden_dir, f"vae_conv_{case}")
    p, act = restate(fx)
    x, eps, dec = (R.t64(fx[k]) for k in ("x", "eps", "dec_noise"))
    for b, beta in BETAS.items():
        out, grads = loss_and_grads(p, act, x, eps, beta, scale=1.0 / D)
        for k in ("z", "mean", "loss", "recon", "kld"):
            assert rel(out[k], fx[f"{b}/{k}_f64"]) <= TOL64, (b, k)
        assert rel(relaxed_sample(out["logit"], dec), fx[f"{b}/x_sample_f64"]) <= TOL64
        assert rel(out["mu"], fx["mu_f64"]) <= TOL64 and rel(out["lv"], fx["lv_f64"]) <= TOL64
        R.check_grads_f64(grads, fx, b, TOL64)
    lp = logprob_rows(p, act, x, R.t64(fx["lp/eps"])).mean()
    assert rel(lp, fx["lp/value_f64"]) <= TOL64
    # the fp32 fixture is the same computation at fp32's precision
    assert rel(fx["b1/loss"], fx["b1/loss_f64"]) <= 1e-5 and rel(fx["lp/value"], fx["lp/value_f64"]) <= 1e-5


def test_restated_trajectory_is_the_reference_in_float64(golden_dir):
    fx = load(golden_dir, "vae_traj_conv")
    assert int(fx["special"]) == 1 and int(fx["cfg/steps"]) == 4                # the run starts from the do_xavier / do_m5bias init
    R.check_traj_f64(trajectory(fx), fx, TOL64)
    assert float(fx["1/beta"]) < 1.0 == float(fx["2/beta"]) == float(fx["3/beta"])          # the ramp ends inside the run


# ---- 3. validation before any HIP call ---------------------------------------------------------------------------------------------
def test_argument_validation_of_kind_11_at_every_entry_point():
    lib = L.lib()
    one, big, small = ctypes.c_void_p(64), ctypes.c_size_t(1 << 40), ctypes.c_size_t(16)      # any non-null address: validation fails before it is read
    ref = ctypes.byref

    fwd = lambda d, x, B, wsf, z, losses: lib.ardae_vae_forward(ref(d), one, one, x, None, B, 1.0, 1.0, 7, 0, None, one, wsf, z, None, losses, None)
    fwd_dev = lambda d, st: lib.ardae_vae_forward_dev(ref(d), one, one, one, None, 4, st, 1.0, 7, 0, None, one, big, one, None, one, None)
    bwd = lambda d, B, wsf, g: lib.ardae_vae_backward(ref(d), one, one, one, B, 1.0, 1.0, one, wsf, g, 0.0, None)
    bwd_dev = lambda d, st: lib.ardae_vae_backward_dev(ref(d), one, one, one, 4, st, 1.0, one, big, one, 0.0, None)
    stats = lambda d, B, wsf, mu, lv: lib.ardae_vae_encode_stats(ref(d), one, one, one, B, one, wsf, mu, lv, None)
    head = lambda d, B, variant, mu, eps_out=one: lib.ardae_vae_head(ref(d), one, one, one, None, B, 7, 0, None, variant, mu, one, one, eps_out, one, None)
    desc = lambda **kw: L.ModelDesc(*[kw.get(k, v) for k, v in (("kind", 11), ("input_dim", 784), ("noise_dim", 0), ("h_dim", 800), ("z_dim", 32),
                                                                  ("n_layers", 1), ("act", 2), ("flags", 0))])
    ok = desc()
    assert lib.ardae_model_param_floats(ref(ok)) == 703405 and lib.ardae_model_packed_floats(ref(ok)) > 703405
    assert lib.ardae_model_workspace_floats(ref(ok), 4, 1, 1) > lib.ardae_model_workspace_floats(ref(ok), 4, 1, 0) > 0
    assert lib.ardae_model_workspace_floats(ref(ok), 4, 1, 2) > 0
    assert lib.ardae_model_workspace_floats(ref(ok), 4, 2, 1) == lib.ardae_model_workspace_floats(ref(ok), 4, 2, 0) == 0     # one draw per image
    assert lib.ardae_model_workspace_floats(ref(ok), 4, 1, 3) == 0                                                            # no sampler pair
    # this family's fused head (the two MFMA products + one tail launch) is the default wherever its tail runs: z <= 64 (README)
    assert [lib.ardae_vae_head_fused_ok(ref(desc(z_dim=z))) for z in (32, 6, 64, 65)] == [1, 1, 1, 0]
    # each descriptor rule
    for bad, why in ((desc(input_dim=783), "input_dim 784"), (desc(h_dim=300), "h_dim must be 800"), (desc(n_layers=2), "n_layers must be 1"),
                     (desc(noise_dim=3), "noise_dim must be 0"), (desc(flags=1), "flags must be 0"), (desc(z_dim=0), "bad dimensions"),
                     (desc(act=0), "unknown activation"), (desc(act=99), "unknown activation")):
        assert lib.ardae_model_param_floats(ref(bad)) == lib.ardae_model_packed_floats(ref(bad)) == 0
        assert all(lib.ardae_model_workspace_floats(ref(bad), 4, 1, mode) == 0 for mode in (0, 1, 2))
        assert lib.ardae_vae_head_fused_ok(ref(bad)) == 0
        fails(lib.ardae_model_pack(ref(bad), one, one, None), why)
        fails(lib.ardae_model_decode(ref(bad), one, one, one, 4, one, big, one, None, None), why)
        fails(fwd(bad, one, 4, big, one, one), why)
        fails(bwd(bad, 4, big, one), why)
        fails(stats(bad, 4, big, one, one), why)
        fails(head(bad, 4, 0, one), why)
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
    fails(stats(ok, 0, big, one, one), "bad batch")
    fails(stats(ok, 4, small, one, one), "workspace too small")
    fails(stats(ok, 4, big, None, one), "null pointer")
    fails(stats(ok, 4, big, one, None), "null pointer")
    fails(head(ok, 0, 1, one), "bad batch")
    fails(head(ok, 4, 3, one), "variant must be")
    fails(head(ok, 4, 1, None), "null pointer")
    fails(head(ok, 4, 2, one, eps_out=None), "null pointer")                               # the unfused head draws into eps_out
    fails(head(desc(z_dim=65), 4, 1, one), "the fused head takes")
    fails(lib.ardae_model_decode(ref(ok), one, one, one, 4, one, small, one, None, None), "workspace too small")
    fails(lib.ardae_model_decode(ref(ok), one, one, None, 4, one, big, one, None, None), "bad arguments")
    # the implicit models' calls refuse the family: there is no sampler
    fails(lib.ardae_model_encode(ref(ok), one, one, one, None, 4, 1, one, big, one, None), "analytic posterior")
    fails(lib.ardae_model_vae_forward(ref(ok), one, one, one, one, 4, 1, 1.0, one, big, one, one, None), "ardae_vae_forward")
    fails(lib.ardae_model_vae_backward(ref(ok), one, one, one, one, 4, 1, 1.0, 1.0, None, one, big, one, 0.0, None), "ardae_vae_backward")
    # 10 is still not a kind, anywhere; the messages name the third kind
    bad = desc(kind=10)
    assert lib.ardae_model_param_floats(ref(bad)) == lib.ardae_model_packed_floats(ref(bad)) == lib.ardae_model_workspace_floats(ref(bad), 4, 1, 1) == 0
    assert lib.ardae_vae_head_fused_ok(ref(bad)) == 0
    for rc in (lib.ardae_model_pack(ref(bad), one, one, None), lib.ardae_model_decode(ref(bad), one, one, one, 4, one, big, one, None, None),
               lib.ardae_model_encode(ref(bad), one, one, one, None, 4, 1, one, big, one, None)):
        fails(rc, "kind must be")
        assert b"11 (MNISTConvVAE)" in lib.ardae_last_error()
    for call in (lambda: fwd(bad, one, 4, big, one, one), lambda: bwd(bad, 4, big, one), lambda: stats(bad, 4, big, one, one), lambda: head(bad, 4, 0, one)):
        fails(call(), "kind must be 8 (MNISTVAE), 9 (ToyVAE) or 11 (MNISTConvVAE)")


# ---- 4. refusals on the module -----------------------------------------------------------------------------------------------------
def test_module_surface_and_refusals():
    with pytest.raises(NotImplementedError, match="28x28x1"):
        net.MNISTConvVAE(input_height=32)
    with pytest.raises(NotImplementedError, match="28x28x1"):
        net.MNISTConvVAE(input_channels=2)
    with pytest.raises(NotImplementedError, match="nonlinearity"):
        net.MNISTConvVAE(nonlinearity="gelu")
    with pytest.raises(NotImplementedError, match="normal_energy_func"):
        net.MNISTConvVAE(energy_func=lambda z: z.sum(1))
    m = net.MNISTConvVAE(z_dim=8)
    assert isinstance(m, net.GaussianVAE) and m.return_samples and (m.input_height, m.input_channels, m.do_xavier, m.do_m5bias) == (28, 1, False, False)
    for call in (lambda: m(torch.zeros(3, 784)), lambda: m(torch.zeros(3, 1, 28, 28)), lambda: m.logprob(torch.zeros(3, 784), sample_size=4),
                 lambda: m.logprob_rows(torch.zeros(3, 784), 4), lambda: m.encode(torch.zeros(3, 784)), lambda: m.encode_stats(torch.zeros(3, 784)),
                 lambda: m.generate(2)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    with pytest.raises(RuntimeError, match="no CPU path"):
        net.VaeEngine(m, net.VaeConfig(), batch_size=4)
    with pytest.raises(TypeError, match="MNISTConvVAE"):
        net.VaeEngine(net.ConvIPVAE(z_dim=8, noise_dim=4), net.VaeConfig(), batch_size=4)
    with pytest.raises(TypeError, match="MNISTConvVAE"):
        net.GaussianIwaeEvaluator(net.ConvIPVAE(z_dim=8, noise_dim=4), 16)
    with pytest.raises(NotImplementedError, match="z_dim 65 > 64"):
        net.GaussianIwaeEvaluator(net.MNISTConvVAE(z_dim=65), 16)
    # the evaluator plans the recipe's evaluation at the default budget (this decoder keeps ~5e4 floats per decoded row, so the importance samples
    # are decoded 16 images per call; the encoder runs on 64); chunks are whole groups of 64 images, and a budget below one group is refused
    ev = net.GaussianIwaeEvaluator(net.MNISTConvVAE(z_dim=32), 256)
    plan = ev.plan(2048)
    assert plan[0][0] == 0 and plan[-1][1] == 2048 and all(a[1] == b[0] for a, b in zip(plan, plan[1:]))
    assert (ev.image_group, ev.group) == (64, 16) and ev.floats_per_chunk(plan[0][1]) <= ev.budget
    assert all((b - a) % 64 == 0 for a, b in plan[:-1]) and len(plan) > 1
    small = net.GaussianIwaeEvaluator(ev.model, 256, max_workspace_floats=ev.floats_per_chunk(150))
    assert [b - a for a, b in small.plan(300)] == [64, 64, 64, 64, 44]       # three equal chunks of 100 fit, cut down to whole groups
    with pytest.raises(ValueError, match="one group of 64 images"):
        net.GaussianIwaeEvaluator(ev.model, 256, max_workspace_floats=ev.floats_per_chunk(40)).plan(100)
    assert net.GaussianIwaeEvaluator(ev.model, 256, max_workspace_floats=ev.floats_per_chunk(12)).plan(12) == [(0, 12)]
    mlp = net.GaussianIwaeEvaluator(net.MNISTVAE(input_dim=12, h_dim=16, z_dim=4), 16)
    assert (mlp.image_group, mlp.group) == (None, None)                     # the MLP families: a chunk per call, as before
