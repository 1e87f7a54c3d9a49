"""Gaussian-posterior VAE baselines (ardae_model_desc.kind 8 / 9, the reference's vae.py --model mnist / toy): layout, argument validation
of every new entry point, the beta schedule on the host, and the float64 restatement of the two families that the GPU tests lean on -
pinned here to the reference's fp64 fixtures.  No GPU needed."""
import ctypes
import functools
import math

import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import layout
import vae_restate as R
from vae_restate import ACTS, BETAS, fails, lin, load, rel

KIND_ID = {"mnist": 8, "toy": 9}
CASES = {"mnist": ("d64_h40_z6", "d36_h300_z32"), "toy": ("h40_relu", "h40_tanh")}


def case_names():
    return [(f, c) for f, cs in CASES.items() for c in cs]


def state_dict_of(fx, dtype=torch.float32):
    return {k[3:]: torch.tensor(v).to(dtype) for k, v in fx.items() if k.startswith("sd/")}


# ---- the test-side oracle: both families restated in plain torch -------------------------------------------------------------------
def mlp_act(p, prefix, hdn, act):
    """models/layers.py MLP(..., use_nonlinearity_output=True): `layers.*` then `fc`, every one followed by the activation"""
    n = len([k for k in p if k.startswith(prefix + "layers.") and k.endswith("weight")])
    for name in [f"layers.{i}" for i in range(n)] + ["fc"]:
        hdn = ACTS[act](hdn @ p[f"{prefix}{name}.weight"].t() + p[f"{prefix}{name}.bias"])
    return hdn


def encode(family, p, act, x):
    hdn = mlp_act(p, "encode.main.", 2 * x - 1 if family == "mnist" else x, act)
    return lin(p, "encode.reparam.mean_fn", hdn), lin(p, "encode.reparam.logvar_fn", hdn)


def recon_rows(family, p, act, x, z):
    """-log p(x | z) per row of z [R, zd] against x [R, D]; -> rows, decoder mean"""
    hdn = mlp_act(p, "decode.main.", z, act)
    if family == "mnist":
        logit = lin(p, "decode.reparam.logit_fn", hdn)
        return torch.nn.functional.binary_cross_entropy_with_logits(logit, x, reduction="none").sum(1), torch.sigmoid(logit)
    mu, lv = lin(p, "decode.reparam.mean_fn", hdn), lin(p, "decode.reparam.logvar_fn", hdn)
    return 0.5 * (lv + (x - mu) ** 2 / lv.exp() + math.log(2 * math.pi)).sum(1), mu


def forward(p, cfg, x, eps, beta):
    """-> dict(mu, lv, z, mean, loss, recon, kld): VAE.forward (vae/mnist.py:142-162, vae/toy.py:133-152); cfg = (family, activation)"""
    family, act = cfg
    mu, lv = encode(family, p, act, x)
    z = mu + torch.exp(0.5 * lv) * eps
    kld = R.kld_rows(mu, lv)
    rec, mean = recon_rows(family, p, act, x, z)
    return dict(mu=mu, lv=lv, z=z, mean=mean, loss=(rec + beta * kld).mean(), recon=rec.mean(), kld=kld.mean())


loss_and_grads = functools.partial(R.loss_and_grads, forward)      # (p, cfg, x, eps, beta, scale=) -> forward's dict (detached), {name: gradient}


def logprob_rows(p, cfg, x, eps):
    """VAE.logprob before its mean (vae/mnist.py:179-217) on injected draws eps [B, k, zd]"""
    family, act = cfg
    return R.gaussian_logprob_rows(*encode(family, p, act, x), x, eps, lambda xr, zr: recon_rows(family, p, act, xr, zr)[0])


def restate(fx):
    """-> the fixture's parameters in float64, cfg"""
    return state_dict_of(fx, torch.float64), (str(fx["family"]), str(fx["act"]))


# ---- 1. layout ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,case", case_names())
def test_layout_names_and_shapes_are_the_fixtures(golden_dir, family, case):
    fx = load(golden_dir, f"vae_{family}_{case}")
    B, D, h, z, nl = (int(v) for v in fx["shape"])
    sd = state_dict_of(fx)
    spec = layout.vae_spec(family, D, h, z, nl)
    assert [(n, tuple(s)) for n, s in spec] == [(k, tuple(v.shape)) for k, v in sd.items()]
    desc = L.ModelDesc(KIND_ID[family], D, 0, h, z, nl, L.ACT[str(fx["act"])], 0)
    total = layout.offsets(spec)[1]
    assert total == L.query("ardae_model_param_floats", desc) == sum(v.numel() for v in sd.values())
    assert L.query("ardae_model_packed_floats", desc) > total
    sizes = [[L.query("ardae_model_workspace_floats", desc, b, 1, mode) for b in (6, 70, 129)] for mode in (0, 1, 2)]
    for per_mode in sizes:
        assert 0 < per_mode[0] < per_mode[1] < per_mode[2]
    assert all(a < b for a, b in zip(sizes[0], sizes[1]))               # the training workspace holds the encoder's and more
    # the module's parameters are the spec, in order, with the reference's state_dict names
    ctor = net.MNISTVAE if family == "mnist" else net.ToyVAE
    mod = ctor(input_dim=D, h_dim=h, z_dim=z, nonlinearity=str(fx["act"]), num_hidden_layers=nl)
    assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == [(n, tuple(s)) for n, s in spec]
    mod.load_state_dict(sd)
    assert torch.equal(mod.flat_params(), torch.cat([v.reshape(-1) for v in sd.values()]))


def test_layout_count_at_the_recipe_shape_and_trajectory_fixtures(golden_dir):
    # parameter counts of the reference's own classes at the recipe widths, recorded by tools/gen_vae_golden.py
    counts = load(golden_dir, "vae_param_counts")
    for family, key in (("mnist", "mnist_784_300_32_2"), ("toy", "toy_2_256_2_2")):
        D, h, z, nl = (int(v) for v in key.split("_")[1:])
        d = L.ModelDesc(KIND_ID[family], D, 0, h, z, nl, L.ACT["softplus"], 0)
        assert layout.offsets(layout.vae_spec(family, D, h, z, nl))[1] == L.query("ardae_model_param_floats", d) == int(counts[key])
    desc = L.ModelDesc(8, 784, 0, 300, 32, 2, L.ACT["softplus"], 0)
    assert L.query("ardae_vae_head_fused_ok", desc) == 1
    assert L.query("ardae_vae_head_fused_ok", L.ModelDesc(9, 2, 0, 256, 2, 2, L.ACT["relu"], 0)) == 0               # the logvar rows start 8 bytes off the 16-byte grid
    assert L.query("ardae_vae_head_fused_ok", L.ModelDesc(8, 784, 0, 302, 32, 2, L.ACT["softplus"], 0)) == 0       # h no multiple of 4
    assert L.query("ardae_vae_head_fused_ok", L.ModelDesc(8, 784, 0, 300, 65, 2, L.ACT["softplus"], 0)) == 0       # wider than the fused kernel takes
    assert L.query("ardae_vae_head_fused_ok", L.ModelDesc(0, 784, 100, 300, 32, 2, L.ACT["softplus"], 0)) == 0     # not a kind of this family
    for family in ("mnist", "toy"):
        fx = load(golden_dir, f"vae_traj_{family}")
        B, D, h, z, nl = (int(v) for v in fx["shape"])
        assert [(n, tuple(s)) for n, s in layout.vae_spec(family, D, h, z, nl)] == [(k, tuple(v.shape)) for k, v in state_dict_of(fx).items()]
    with pytest.raises(NotImplementedError):
        layout.vae_spec("conv", 784, 300, 32, 2)


def test_module_surface_and_refusals():
    m = net.MNISTVAE(input_dim=12, h_dim=16, z_dim=4, nonlinearity="softplus", num_hidden_layers=2, do_xavier=True, do_m5bias=True)
    p = {k: v.detach() for k, v in m.named_parameters()}
    assert float(p["decode.reparam.logit_fn.bias"].min()) == float(p["decode.reparam.logit_fn.bias"].max()) == -5.0
    assert all(float(v.abs().max()) == 0.0 for k, v in p.items() if k.endswith("bias") and "logit_fn" not in k)
    bound = math.sqrt(6.0 / (12 + 16))
    assert 0.5 * bound < float(p["encode.main.layers.0.weight"].abs().max()) <= bound      # xavier-uniform
    torch.manual_seed(0)
    t = net.ToyVAE(input_dim=2, h_dim=256, z_dim=2, nonlinearity="relu", num_hidden_layers=2, init="gaussian")
    w = dict(t.named_parameters())["decode.reparam.mean_fn.weight"].detach()
    assert float(w.abs().max()) > 1.5 and abs(float(w.std()) - 1.0) < 0.15                # N(0, 1), not U(+-1/16)
    plain = dict(net.ToyVAE(input_dim=2, h_dim=256, z_dim=2, nonlinearity="relu", num_hidden_layers=2, init=None).named_parameters())
    assert float(plain["decode.reparam.mean_fn.weight"].detach().abs().max()) <= 1.0 / 16
    for mod in (m, t):       # execution on the CPU is refused
        with pytest.raises(RuntimeError, match="no CPU path"):
            mod(torch.zeros(3, mod.input_dim))
        with pytest.raises(RuntimeError, match="no CPU path"):
            mod.logprob(torch.zeros(3, mod.input_dim), sample_size=4)
        with pytest.raises(RuntimeError, match="no CPU path"):
            mod.generate(2)
    wide = net.MNISTVAE(input_dim=12, h_dim=16, z_dim=65, num_hidden_layers=1)      # trains through the unfused head; its IWAE draw is not built
    with pytest.raises(NotImplementedError, match="z_dim 65 > 64"):
        net.GaussianIwaeEvaluator(wide, 16)
    with pytest.raises(NotImplementedError):
        net.MNISTVAE(nonlinearity="gelu")
    with pytest.raises(ValueError, match="num_hidden_layers"):
        net.ToyVAE(num_hidden_layers=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        net.VaeEngine(m, net.VaeConfig(), batch_size=4)
    with pytest.raises(TypeError, match="VaeEngine drives"):
        net.VaeEngine(net.MNISTIPVAE(input_dim=12, noise_dim=4, h_dim=16, z_dim=4), net.VaeConfig(), batch_size=4)


# ---- 2. validation before any HIP call ---------------------------------------------------------------------------------------------
def test_argument_validation_of_every_new_entry_point():
    lib = L.lib()
    one, big, small = ctypes.c_void_p(64), ctypes.c_size_t(1 << 40), ctypes.c_size_t(16)      # any non-null address: validation fails before it is read
    ref = ctypes.byref

    fwd = lambda d, x, B, wsf, z, losses: lib.ardae_vae_forward(ref(d), one, one, x, None, B, 1.0, 1.0, 7, 0, None, one, wsf, z, None, losses, None)
    fwd_dev = lambda d, st: lib.ardae_vae_forward_dev(ref(d), one, one, one, None, 4, st, 1.0, 7, 0, None, one, big, one, None, one, None)
    bwd = lambda d, B, wsf, g: lib.ardae_vae_backward(ref(d), one, one, one, B, 1.0, 1.0, one, wsf, g, 0.0, None)
    bwd_dev = lambda d, st: lib.ardae_vae_backward_dev(ref(d), one, one, one, 4, st, 1.0, one, big, one, 0.0, None)
    stats = lambda d, B, wsf, mu, lv: lib.ardae_vae_encode_stats(ref(d), one, one, one, B, one, wsf, mu, lv, None)
    head = lambda d, B, variant, mu, eps_out=one: lib.ardae_vae_head(ref(d), one, one, one, None, B, 7, 0, None, variant, mu, one, one, eps_out, one, None)
    for k in (8, 9):
        ok = L.ModelDesc(k, 12, 0, 16, 4, 2, 2, 0)
        assert lib.ardae_model_param_floats(ref(ok)) > 0 and lib.ardae_model_packed_floats(ref(ok)) > 0
        assert lib.ardae_model_workspace_floats(ref(ok), 4, 1, 1) > lib.ardae_model_workspace_floats(ref(ok), 4, 1, 0) > 0
        assert lib.ardae_model_workspace_floats(ref(ok), 4, 2, 1) == 0                      # one draw per image
        # a noise input, flags, no layers: no such network
        for bad, why in ((L.ModelDesc(k, 12, 3, 16, 4, 2, 2, 0), "noise_dim must be 0"), (L.ModelDesc(k, 12, 0, 16, 4, 2, 2, 1), "flags must be 0"),
                         (L.ModelDesc(k, 12, 0, 16, 4, 0, 2, 0), "bad dimensions"), (L.ModelDesc(k, 12, 0, 16, 4, 2, 0, 0), "unknown activation")):
            assert lib.ardae_model_param_floats(ref(bad)) == lib.ardae_model_packed_floats(ref(bad)) == lib.ardae_model_workspace_floats(ref(bad), 4, 1, 1) == 0
            assert lib.ardae_vae_head_fused_ok(ref(bad)) == 0
            fails(lib.ardae_model_pack(ref(bad), one, one, None), why)
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
        fails(head(ok, 4, 2, one, eps_out=None), "null pointer")                           # the unfused head draws into eps_out
        fails(head(L.ModelDesc(k, 12, 0, 16, 65, 2, 2, 0), 4, 1, one), "the fused head takes")
        # the implicit models' calls refuse the family: there is no sampler
        fails(lib.ardae_model_encode(ref(ok), one, one, one, None, 4, 1, one, big, one, None), "analytic posterior")
        fails(lib.ardae_model_vae_forward(ref(ok), one, one, one, one, 4, 1, 1.0, one, big, one, one, None), "ardae_vae_forward")
        fails(lib.ardae_model_vae_backward(ref(ok), one, one, one, one, 4, 1, 1.0, 1.0, None, one, big, one, 0.0, None), "ardae_vae_backward")
    # unknown kinds, and the kinds of the other families at the new entry points
    for k in (10, -1, 0, 7):
        bad = L.ModelDesc(k, 12, 0 if k > 7 or k < 0 else 3, 16, 4, 2, 2, 0)
        fails(fwd(bad, one, 4, big, one, one), "kind must be")
        fails(bwd(bad, 4, big, one), "kind must be")
        fails(stats(bad, 4, big, one, one), "kind must be")
        fails(head(bad, 4, 0, one), "kind must be")
    for k in (10, -1):
        bad = L.ModelDesc(k, 12, 0, 16, 4, 2, 2, 0)
        assert lib.ardae_model_param_floats(ref(bad)) == lib.ardae_model_packed_floats(ref(bad)) == 0
        fails(lib.ardae_model_pack(ref(bad), one, one, None), "kind must be")
    fails(lib.ardae_vae_kld_rows(one, one, 0, 4, one, None), "B > 0 and z > 0")
    fails(lib.ardae_vae_kld_rows(one, one, 4, 0, one, None), "B > 0 and z > 0")
    fails(lib.ardae_vae_kld_rows(one, None, 4, 4, one, None), "null pointer")
    fails(lib.ardae_vae_kld_rows(one, one, 4, 4, None, None), "null pointer")
    draw = lambda mu, B, k, z, first, zo, lq: lib.ardae_vae_iwae_draw(mu, one, None, B, k, z, 7, 0, first, zo, lq, None, None)
    fails(draw(one, 0, 16, 4, 0, one, one), "B > 0 and k > 0")
    fails(draw(one, 4, 0, 4, 0, one, one), "B > 0 and k > 0")
    fails(draw(one, 4, -2, 4, 0, one, one), "B > 0 and k > 0")
    fails(draw(one, 4, 16, 0, 0, one, one), "1 <= z <= 64")
    fails(draw(one, 4, 16, 65, 0, one, one), "1 <= z <= 64")
    fails(draw(one, 1 << 20, 1 << 12, 4, 0, one, one), "exceeds 2^31")
    fails(draw(one, 4, 16, 4, 2, one, one), "multiple of 4")
    fails(draw(None, 4, 16, 4, 0, one, one), "null pointer")
    fails(draw(one, 4, 16, 4, 0, None, one), "null pointer")
    fails(draw(one, 4, 16, 4, 0, one, None), "null pointer")


# ---- 3. the float64 restatement, pinned to the reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("family,case", case_names())
def test_restatement_is_the_reference_in_float64(golden_dir, family, case):
    fx = load(golden_dir, f"vae_{family}_{case}")
    D = int(fx["shape"][1])
    p, cfg = restate(fx)
    assert cfg[0] == family
    x, eps = R.t64(fx["x"]), R.t64(fx["eps"])
    for b, beta in BETAS.items():
        out, grads = loss_and_grads(p, cfg, x, eps, beta, scale=1.0 / D)
        for k in ("z", "mean", "loss", "recon", "kld"):
            assert rel(out[k], fx[f"{b}/{k}_f64"]) <= 1e-12, (b, k)
        assert rel(out["mu"], fx["mu_f64"]) <= 1e-12 and rel(out["lv"], fx["lv_f64"]) <= 1e-12
        R.check_grads_f64(grads, fx, b, 1e-12)
    lp = logprob_rows(p, cfg, x, R.t64(fx["lp/eps"])).mean()
    assert rel(lp, fx["lp/value_f64"]) <= 1e-12
    # the fp32 fixture is the same computation at fp32's precision
    assert rel(fx["b1/loss"], fx["b1/loss_f64"]) <= 1e-5 and rel(fx["lp/value"], fx["lp/value_f64"]) <= 1e-5


@pytest.mark.parametrize("family", ["mnist", "toy"])
def test_restated_trajectory_is_the_reference_in_float64(golden_dir, family):
    fx = load(golden_dir, f"vae_traj_{family}")
    p, cfg = restate(fx)
    D = int(fx["shape"][1])
    steps = R.trajectory(fx, p, lambda p, x, eps, beta: loss_and_grads(p, cfg, R.t64(x), R.t64(eps), beta, scale=1.0 / D))
    R.check_traj_f64(steps, fx, 1e-10, keys=("loss",))
    assert float(fx["2/beta"]) < 1.0 == float(fx["3/beta"]) == float(fx["4/beta"])          # the ramp ends inside the run


# ---- 4. beta on the host, configuration ---------------------------------------------------------------------------------------------
def test_host_beta_schedule_is_annealing_func_on_the_zero_based_step():
    annealing = 50000
    cfg = net.VaeConfig(beta_init=1e-4, beta_fin=1.0, beta_annealing=annealing)
    assert cfg.beta_schedule() == (1e-4, 1.0, annealing)
    for i_ep in (0, 1, annealing - 1, annealing, 10 * annealing):
        assert cfg.beta_at(i_ep) == net.annealing_func(1e-4, 1.0, annealing, i_ep)
        assert cfg.beta_at(i_ep) == float(1e-4 + (1.0 - 1e-4) / float(annealing) * float(min(annealing, i_ep)))        # utils/msc.py:53-55
    assert cfg.beta_at(0) == 1e-4 and cfg.beta_at(annealing) == cfg.beta_at(10 * annealing) == 1.0
    const = net.VaeConfig(beta_init=0.1, beta_fin=0.7)
    assert const.beta_schedule() is None and const.beta_at(0) == const.beta_at(12345) == 0.7


def test_config_refuses_what_vae_py_refuses():
    with pytest.raises(NotImplementedError, match="unknown optimizer"):
        net.VaeConfig(optimizer="lion")
    with pytest.raises(NotImplementedError, match="unknown optimizer"):
        net.VaeConfig(optimizer="adam_torch")                          # vae.py builds the vendored Adam
    with pytest.raises(NotImplementedError, match="unknown weight averaging"):
        net.VaeConfig(weight_avg="ema")
    with pytest.raises(ValueError, match="weight_avg_decay"):
        net.VaeConfig(weight_avg="polyak", weight_avg_decay=1.5)
    with pytest.raises(ValueError, match="beta_annealing"):
        net.VaeConfig(beta_annealing=0)
    with pytest.raises(ValueError, match="beta_annealing"):
        net.VaeConfig(beta_annealing=2.5)
    for opt in ("sgd", "adam", "amsgrad", "rmsprop"):
        for avg in ("none", "polyak", "swa"):
            net.VaeConfig(optimizer=opt, weight_avg=avg)


def test_engine_batches_go_through_check_batch():
    """VaeEngine._check_batch is engine_common.check_batch on (B, input_dim): exercised without a device on an engine shell"""
    from ardae_amd.vae import VaeEngine
    eng = object.__new__(VaeEngine)
    eng.B, eng.D, eng.dev = 4, 6, torch.device("cuda", 0)
    with pytest.raises(TypeError, match="expected a tensor"):
        eng._check_batch([[0.0] * 6] * 4, "step(x)")
    with pytest.raises(ValueError, match="batch_size=4"):
        eng._check_batch(torch.zeros(3, 6), "step(x)")                 # a ragged last batch
    with pytest.raises(ValueError, match="batch_size=4"):
        eng._check_batch(torch.zeros(4, 5), "step(x)")
    with pytest.raises(ValueError, match="float32"):
        eng._check_batch(torch.zeros(4, 6, dtype=torch.float64), "step(x)")
    with pytest.raises(ValueError, match="expected a tensor on"):
        eng._check_batch(torch.zeros(4, 6), "step(x)")                 # a host tensor
    with pytest.raises(ValueError, match="contiguous"):
        eng._check_batch(torch.zeros(6, 4).t(), "step(x)")
