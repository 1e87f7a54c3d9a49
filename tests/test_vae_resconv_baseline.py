"""The residual-conv Gaussian-posterior baseline (ardae_model_desc.kind 12, the reference's `vae.py --model resconv`): layout, initialisation,
argument validation of kind 12 at every entry point and of ardae_resconv_tail, refusals of the module, the decode-only workspace, and the float64
restatement of the family (F.conv2d, F.interpolate and the oracle's weight-norm block helpers) that the GPU tests lean on - pinned here to the
reference's float64 fixtures.  No GPU needed.

The fixtures (tools/gen_vae_golden.py, family resconv) do not store the parameters: `resconv_params` regenerates them from the stored seed with
the recipe the tool called (oracle.fixture_params.resconv)."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import layout
from oracle import ardae_oracle as O
from oracle import fixture_params as P
import vae_restate as R
from vae_restate import BETAS, TOL64, fails, lin, load, rel, relaxed_sample

CASES = ("z32_b3", "z6_c42_b5_ct")
D = 784
ELU = 3               # ARDAE_ACT_ELU


resconv_params = P.resconv      # (z, c_dim, seed, special, dtype=): the recipe tools/gen_vae_golden.py loaded into the reference class


def fixture_params(fx, dtype=torch.float32):
    """(the float64 runs of the tool start from the fp32 numbers, widened)"""
    return {k: v.to(dtype) for k, v in resconv_params(int(fx["shape"][1]), int(fx["shape"][2]), int(fx["seed"]), bool(int(fx["special"]))).items()}


def desc_of(z, c_dim, center):
    return L.ModelDesc(12, D, 0, c_dim, z, 1, ELU, 0 if center else L.MODEL_NO_CENTER)


# ---- the test-side oracle: the family restated in plain torch (trunk and decoder: vae_restate) ---------------------------------------
def encode(p, center, x):
    """Encoder.forward up to the statistics (vae/resconv.py:58-68)"""
    h = R.resconv_trunk(p, "encode.enc.", center, x)
    return lin(p, "encode.reparam.mean_fn", h), lin(p, "encode.reparam.logvar_fn", h)


def forward(p, center, x, eps, beta):
    """-> dict(mu, lv, z, mean, logit, loss, recon, kld): VAE.forward (vae/resconv.py:161-181)"""
    mu, lv = encode(p, center, x)
    z = mu + torch.exp(0.5 * lv) * eps
    kld = R.kld_rows(mu, lv)
    rec, logit = R.resconv_recon_rows(p, x, z)
    return dict(mu=mu, lv=lv, z=z, mean=torch.sigmoid(logit), logit=logit, loss=(rec + beta * kld).mean(), recon=rec.mean(), kld=kld.mean())


loss_and_grads = functools.partial(R.loss_and_grads, forward)      # (p, center, x, eps, beta, scale=) -> forward's dict (detached), {name: gradient}


def logprob_rows(p, center, x, eps):
    """VAE.logprob before its mean (vae/resconv.py:198-240) on injected draws eps [B, k, zd]"""
    return R.gaussian_logprob_rows(*encode(p, center, x), x, eps, lambda xr, zr: R.resconv_recon_rows(p, xr, zr)[0])


def restate(fx):
    """-> the fixture's parameters in float64, cfg (do_center)"""
    return fixture_params(fx, torch.float64), bool(int(fx["do_center"]))


def trajectory(fx):
    """The fixture's loop restated in float64: yields (step, forward's dict, the parameters after the vendored Adam's step)"""
    p, center = restate(fx)
    return R.trajectory(fx, p, lambda p, x, eps, beta: loss_and_grads(p, center, R.t64(x), R.t64(eps), beta, scale=1.0 / D))


# ---- 1. layout, initialisation, workspace sizes ------------------------------------------------------------------------------------
def test_layout_is_the_reference_state_dict(golden_dir):
    for name, z, c, center in (("vae_resconv_z32_b3", 32, 450, False), ("vae_resconv_z6_c42_b5_ct", 6, 42, True), ("vae_traj_resconv", 32, 450, False)):
        fx = load(golden_dir, name)
        assert (int(fx["shape"][1]), int(fx["shape"][2]), bool(int(fx["do_center"])), str(fx["act"])) == (z, c, center, "elu")
        ref = [(str(n), tuple(int(v) for v in str(s).split(","))) for n, s in zip(fx["names"], fx["shapes"])]
        spec = layout.resconv_vae_spec(z, c)
        assert [(n, tuple(s)) for n, s in spec] == ref
        desc = desc_of(z, c, center)
        total = layout.offsets(spec)[1]
        assert total == L.query("ardae_model_param_floats", desc) == sum(v.numel() for v in fixture_params(fx).values())
        assert L.query("ardae_model_packed_floats", desc) > total
        mod = net.MNISTResConvVAE(z_dim=z, c_dim=c, do_center=center)
        assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == ref
        assert (mod.input_dim, mod.h_dim, mod.c_dim, mod.latent_dim, mod.z_dim, mod.noise_dim) == (D, c, c, z, z, 0)
        assert (mod._desc.kind, mod._desc.flags) == (12, 0 if center else L.MODEL_NO_CENTER)
        sd = fixture_params(fx)
        mod.load_state_dict(sd)
        assert torch.equal(mod.flat_params(), torch.cat([v.reshape(-1) for v in sd.values()]))
    names = [n for n, _ in layout.resconv_vae_spec(32, 450)]
    for pre, ops in (("encode.enc.", ("0.conv_0h", "2.conv_h1", "4.conv_01", "6.conv_0h", "8.conv_01", "11.dot_0h", "11.dot_h1", "11.dot_01")),
                     ("decode.dec.", ("0.dot_0h", "2.dot_01", "6.conv_0h", "8.conv_h1", "12.conv_01", "14.conv_0h", "17.conv_01"))):
        for op in ops:
            assert all(f"{pre}{op}.{leaf}" in names for leaf in ("direction", "scale", "bias")), (pre, op)
    counts = load(golden_dir, "vae_resconv_param_counts")
    d32 = desc_of(32, 450, False)
    assert layout.offsets(layout.resconv_vae_spec(32, 450))[1] == L.query("ardae_model_param_floats", d32) == int(counts["resconv_32_450"]) == 1813487
    sizes = [[L.query("ardae_model_workspace_floats", d32, b, 1, mode) for b in (1, 9, 70)] for mode in (0, 1, 2)]
    for per_mode in sizes:
        assert 0 < per_mode[0] < per_mode[1] < per_mode[2]
    assert all(a < b for a, b in zip(sizes[0], sizes[1]))               # the training workspace holds the encoder's and more
    assert all(a < b for a, b in zip(sizes[2], sizes[1]))               # ... and the decoder's


def test_decode_only_workspace_is_below_the_training_carving_of_the_same_decoder():
    """Mode 2 of kind 12 keeps one columns scratch for all blocks and (the fused tail) no buffer of the last stage; kind 6 at the same widths keeps
    every block's columns.  From the carving: dec[6] alone holds 784 x (144 + 9 + 1 + 1) + 12544 of ~3.5e5 floats per row, the other blocks' columns
    another ~1e5 that the shared scratch (56448 + 28224) replaces - so well below half."""
    d12, d6 = desc_of(32, 450, False), L.ModelDesc(6, D, 100, 450, 32, 1, ELU, 0)
    for R in (1, 256, 2048):
        w12, w6 = L.query("ardae_model_workspace_floats", d12, R, 1, 2), L.query("ardae_model_workspace_floats", d6, R, 1, 2)
        print(f"mode-2 floats per decoded row at R = {R}: kind 12 {w12 / R:.0f}, kind 6 {w6 / R:.0f}")
        assert 0 < w12 < w6 and 2 * w12 < w6
    assert L.query("ardae_model_workspace_floats", d12, 64, 4, 2) == L.query("ardae_model_workspace_floats", d12, 256, 1, 2)
    # the unfused tail's own buffers, and none for the kernel
    assert L.query("ardae_resconv_tail_workspace_floats", d12, 3, 1) == L.query("ardae_resconv_tail_workspace_floats", d12, 3, 0) == 0
    assert L.query("ardae_resconv_tail_workspace_floats", d12, 3, 2) >= 3 * (12544 + 784 * (144 + 9 + 2))


def test_initialisation_follows_the_weight_norm_init_and_do_m5bias():
    torch.manual_seed(0)
    m = net.MNISTResConvVAE(z_dim=8, c_dim=40, do_m5bias=True)
    p = {k: v.detach() for k, v in m.named_parameters()}
    assert abs(float(p["decode.dec.17.conv_01.bias"]) + 3.0) < 1e-3
    for k, v in p.items():
        if k.endswith(".scale"):
            assert bool((v == 1.0).all()), k
    for k, fan in (("encode.enc.4.conv_0h", 16), ("encode.enc.11.dot_01", 512), ("decode.dec.0.dot_0h", 8), ("decode.dec.12.conv_h1", 16)):
        bound = 1.0 / math.sqrt(fan)                                    # U(+-1 / sqrt(in_features | in_channels)) for direction and bias
        assert 0.8 * bound < float(p[k + ".direction"].abs().max()) <= bound and 0.0 < float(p[k + ".bias"].abs().max()) <= bound, k
    bound = 1.0 / math.sqrt(40)                                         # the two heads are nn.Linear: torch's default
    assert 0.0 < float(p["encode.reparam.mean_fn.weight"].abs().max()) <= bound and 0.0 < float(p["encode.reparam.logvar_fn.bias"].abs().max()) <= bound
    plain = net.MNISTResConvVAE(z_dim=8, c_dim=40)
    assert abs(float(dict(plain.named_parameters())["decode.dec.17.conv_01.bias"].detach())) <= 1.0 / 4


# ---- 2. the float64 restatement, pinned to the reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_restatement_is_the_reference_in_float64(golden_dir, case):
    fx = load(golden_dir, f"vae_resconv_{case}")
    p, center = restate(fx)
    x, eps, dec = (R.t64(fx[k]) for k in ("x", "eps", "dec_noise"))
    for b, beta in BETAS.items():
        out, grads = loss_and_grads(p, center, x, eps, beta, scale=1.0 / D)
        for k in ("z", "mean", "loss", "recon", "kld"):
            assert rel(out[k], fx[f"{b}/{k}_f64"]) <= TOL64, (b, k)
        assert rel(relaxed_sample(out["logit"], dec), fx[f"{b}/x_sample_f64"]) <= TOL64
        assert rel(out["mu"], fx["mu_f64"]) <= TOL64 and rel(out["lv"], fx["lv_f64"]) <= TOL64
        R.check_grads_f64(grads, fx, b, TOL64)
    lp = logprob_rows(p, center, x, R.t64(fx["lp/eps"])).mean()
    assert rel(lp, fx["lp/value_f64"]) <= TOL64
    # the last stage on its own is the decoder's last stage
    z = out["z"][:2]
    h = F.elu(O.res_linear(p, "decode.dec.2.", F.elu(O.res_linear(p, "decode.dec.0.", z, True)), True)).view(-1, 32, 4, 4)
    up = lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=True)      # noqa: E731
    h = F.elu(O.res_conv(p, "decode.dec.8.", F.elu(O.res_conv(p, "decode.dec.6.", up(h), 1, F.elu)), 1, F.elu))[:, :, :-1, :-1]
    h = F.elu(O.res_conv(p, "decode.dec.14.", F.elu(O.res_conv(p, "decode.dec.12.", up(h), 1, F.elu)), 1, F.elu))
    assert rel(R.resconv_tail_logit(p, h.permute(0, 2, 3, 1)), out["logit"][:2]) <= TOL64
    # the fp32 fixture is the same computation at fp32's precision
    assert rel(fx["b1/loss"], fx["b1/loss_f64"]) <= 1e-5 and rel(fx["lp/value"], fx["lp/value_f64"]) <= 1e-5


def test_restated_trajectory_is_the_reference_in_float64(golden_dir):
    fx = load(golden_dir, "vae_traj_resconv")
    assert int(fx["special"]) == 1 and int(fx["cfg/steps"]) == 4 and float(fx["cfg/beta1"]) == 0.9        # the recipe's Adam, from the do_m5bias setting
    R.check_traj_f64(trajectory(fx), fx, TOL64)
    assert float(fx["1/beta"]) < 1.0 == float(fx["2/beta"]) == float(fx["3/beta"])          # the ramp ends inside the run


# ---- 3. validation before any HIP call ---------------------------------------------------------------------------------------------
def test_argument_validation_of_kind_12_at_every_entry_point():
    lib = L.lib()
    one, big, small = ctypes.c_void_p(64), ctypes.c_size_t(1 << 40), ctypes.c_size_t(16)      # any non-null address: validation fails before it is read
    ref = ctypes.byref

    fwd = lambda d, x, B, wsf, z, losses: lib.ardae_vae_forward(ref(d), one, one, x, None, B, 1.0, 1.0, 7, 0, None, one, wsf, z, None, losses, None)
    fwd_dev = lambda d, st: lib.ardae_vae_forward_dev(ref(d), one, one, one, None, 4, st, 1.0, 7, 0, None, one, big, one, None, one, None)
    bwd = lambda d, B, wsf, g: lib.ardae_vae_backward(ref(d), one, one, one, B, 1.0, 1.0, one, wsf, g, 0.0, None)
    bwd_dev = lambda d, st: lib.ardae_vae_backward_dev(ref(d), one, one, one, 4, st, 1.0, one, big, one, 0.0, None)
    stats = lambda d, B, wsf, mu, lv: lib.ardae_vae_encode_stats(ref(d), one, one, one, B, one, wsf, mu, lv, None)
    head = lambda d, B, variant, mu, eps_out=one: lib.ardae_vae_head(ref(d), one, one, one, None, B, 7, 0, None, variant, mu, one, one, eps_out, one, None)
    tail = lambda d, R, variant, y=one, ws=one, wsf=big, out=one, params=one: lib.ardae_resconv_tail(ref(d), params, one, y, R, variant, ws, wsf, out, None)
    desc = lambda **kw: L.ModelDesc(*[kw.get(k, v) for k, v in (("kind", 12), ("input_dim", 784), ("noise_dim", 0), ("h_dim", 450), ("z_dim", 32),
                                                                  ("n_layers", 1), ("act", ELU), ("flags", 1))])
    ok = desc()
    assert lib.ardae_model_param_floats(ref(ok)) == 1813487 and lib.ardae_model_packed_floats(ref(ok)) > 1813487
    assert lib.ardae_model_param_floats(ref(desc(flags=0))) == 1813487                                                        # do_center: the same layout
    assert lib.ardae_model_workspace_floats(ref(ok), 4, 1, 1) > lib.ardae_model_workspace_floats(ref(ok), 4, 1, 0) > 0
    assert lib.ardae_model_workspace_floats(ref(ok), 4, 1, 2) > 0
    assert lib.ardae_model_workspace_floats(ref(ok), 4, 2, 1) == lib.ardae_model_workspace_floats(ref(ok), 4, 2, 0) == 0     # one draw per image
    assert lib.ardae_model_workspace_floats(ref(ok), 4, 1, 3) == 0                                                            # no sampler pair
    # each descriptor rule
    for bad, why in ((desc(input_dim=783), "input_dim 784"), (desc(noise_dim=3), "noise_dim must be 0"), (desc(h_dim=0), "bad dimensions"),
                     (desc(z_dim=0), "bad dimensions"), (desc(n_layers=2), "n_layers must be 1"), (desc(act=2), "ELU only"), (desc(act=0), "ELU only"),
                     (desc(flags=2), "flags must be 0 or ARDAE_MODEL_NO_CENTER"), (desc(flags=17), "flags must be 0 or ARDAE_MODEL_NO_CENTER")):
        assert lib.ardae_model_param_floats(ref(bad)) == lib.ardae_model_packed_floats(ref(bad)) == 0
        assert all(lib.ardae_model_workspace_floats(ref(bad), 4, 1, mode) == 0 for mode in (0, 1, 2))
        assert lib.ardae_vae_head_fused_ok(ref(bad)) == 0 and lib.ardae_resconv_tail_workspace_floats(ref(bad), 4, 2) == 0
        fails(lib.ardae_model_pack(ref(bad), one, one, None), why)
        fails(lib.ardae_model_decode(ref(bad), one, one, one, 4, one, big, one, None, None), why)
        fails(fwd(bad, one, 4, big, one, one), why)
        fails(bwd(bad, 4, big, one), why)
        fails(stats(bad, 4, big, one, one), why)
        fails(head(bad, 4, 0, one), why)
        fails(tail(bad, 4, 1), why)
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
    # the tail on its own
    fails(tail(ok, 4, 3), "variant must be")
    fails(tail(ok, 4, -1), "variant must be")
    fails(tail(ok, 0, 1), "bad batch")
    fails(tail(ok, 1 << 20, 1), "bad batch")
    fails(tail(ok, 4, 1, y=None), "null pointer")
    fails(tail(ok, 4, 1, out=None), "null pointer")
    fails(tail(ok, 4, 1, params=None), "null pointer")
    fails(tail(ok, 4, 2, ws=None), "null pointer")                                         # the unfused launches need their buffers
    fails(tail(ok, 4, 2, wsf=small), "workspace too small")
    fails(tail(L.ModelDesc(11, 784, 0, 800, 32, 1, 2, 0), 4, 1), "kind must be 12")
    fails(tail(L.ModelDesc(6, 784, 100, 450, 32, 1, ELU, 0), 4, 1), "kind must be 12")
    fails(lib.ardae_resconv_tail(None, one, one, one, 4, 1, one, big, one, None), "desc is NULL")
    # the implicit models' calls refuse the family: there is no sampler
    fails(lib.ardae_model_encode(ref(ok), one, one, one, None, 4, 1, one, big, one, None), "analytic posterior")
    fails(lib.ardae_model_vae_forward(ref(ok), one, one, one, one, 4, 1, 1.0, one, big, one, one, None), "ardae_vae_forward")
    fails(lib.ardae_model_vae_backward(ref(ok), one, one, one, one, 4, 1, 1.0, 1.0, None, one, big, one, 0.0, None), "ardae_vae_backward")
    # 13 is not a kind; the messages name the new one
    bad = desc(kind=13)
    assert lib.ardae_model_param_floats(ref(bad)) == lib.ardae_model_workspace_floats(ref(bad), 4, 1, 1) == 0
    fails(lib.ardae_model_pack(ref(bad), one, one, None), "12 (MNISTResConvVAE)")
    fails(fwd(bad, one, 4, big, one, one), "12 (MNISTResConvVAE)")


# ---- 4. refusals on the module, the evaluator's plan -------------------------------------------------------------------------------
def test_module_surface_and_refusals():
    with pytest.raises(NotImplementedError, match="28x28x1"):
        net.MNISTResConvVAE(input_height=32)
    with pytest.raises(NotImplementedError, match="28x28x1"):
        net.MNISTResConvVAE(input_channels=2)
    with pytest.raises(NotImplementedError, match="'elu'"):
        net.MNISTResConvVAE(nonlinearity="softplus")
    with pytest.raises(NotImplementedError, match="normal_energy_func"):
        net.MNISTResConvVAE(energy_func=lambda z: z.sum(1))
    m = net.MNISTResConvVAE(z_dim=8, c_dim=40)
    assert isinstance(m, net.GaussianVAE) and m.return_samples
    assert (m.input_height, m.input_channels, m.c_dim, m.nonlinearity, m.do_center, m.do_m5bias) == (28, 1, 40, "elu", False, False)
    for call in (lambda: m(torch.zeros(3, 784)), lambda: m(torch.zeros(3, 1, 28, 28)), lambda: m.logprob(torch.zeros(3, 784), sample_size=4),
                 lambda: m.logprob_rows(torch.zeros(3, 784), 4), lambda: m.encode(torch.zeros(3, 784)), lambda: m.encode_stats(torch.zeros(3, 784)),
                 lambda: m.generate(2), lambda: m.decode_params(torch.zeros(3, 8))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    with pytest.raises(RuntimeError, match="no CPU path"):
        net.VaeEngine(m, net.VaeConfig(), batch_size=4)
    with pytest.raises(TypeError, match="MNISTResConvVAE"):
        net.VaeEngine(net.ResConvIPVAE(z_dim=8, noise_dim=4, h_dim=16), net.VaeConfig(), batch_size=4)
    with pytest.raises(TypeError, match="MNISTResConvVAE"):
        net.GaussianIwaeEvaluator(net.ResConvIPVAE(z_dim=8, noise_dim=4, h_dim=16), 16)
    with pytest.raises(NotImplementedError, match="z_dim 65 > 64"):
        net.GaussianIwaeEvaluator(net.MNISTResConvVAE(z_dim=65, c_dim=40), 16)
    # the evaluator plans the recipe's evaluation at the default budget: the importance samples are decoded 8 images (2048 rows) per call, the
    # encoder runs on 64; chunks are whole groups of 64 images, and a budget below one group is refused
    ev = net.GaussianIwaeEvaluator(net.MNISTResConvVAE(z_dim=32, c_dim=450), 256)
    assert ev.budget == 1 << 28 and (ev.image_group, ev.group) == (64, 8)
    plan = ev.plan(2048)
    assert plan[0][0] == 0 and plan[-1][1] == 2048 and all(a[1] == b[0] for a, b in zip(plan, plan[1:]))
    assert all(ev.floats_per_chunk(b - a) <= ev.budget for a, b in plan)
    assert all((b - a) % 64 == 0 for a, b in plan)
    with pytest.raises(ValueError, match="one group of 64 images"):
        net.GaussianIwaeEvaluator(ev.model, 256, max_workspace_floats=ev.floats_per_chunk(40)).plan(100)
    assert net.GaussianIwaeEvaluator(ev.model, 256, max_workspace_floats=ev.floats_per_chunk(12)).plan(12) == [(0, 12)]
