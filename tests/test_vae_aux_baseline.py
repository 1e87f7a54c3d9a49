"""Auxiliary-variable Gaussian baselines (ardae_model_desc.kind 14 / 15, the reference's vae.py --model auxmnist / auxtoy): layout, descriptor rules
and argument validation through the C ABI, the module surface, and a float64 numpy restatement of the model - forward, both KLs, the closed-form
backward and the three-stage logprob - that the GPU tests lean on, pinned here to the reference's fp64 fixtures.  No GPU needed."""
import ctypes
import math

import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import layout
from oracle import fixture_params as P
import vae_restate as R
from vae_restate import BETAS, TOL64, clip_logvar, fails, lin, load, mlp_fwd, rel
from vae_restate import aux_forward_backward as forward_backward      # the family's restatement, in float64 numpy with the backward by hand
from vae_restate import aux_logprob_rows as logprob_rows

KIND_ID = {"mnist": 14, "toy": 15}
CASES = ("auxmnist_n100_z32_b3", "auxmnist_n10_z6_b5_spm6", "auxtoy_n2_z2_b7", "auxtoy_n5_z3_b4_hard")
TRAJ = ("auxmnist", "auxtoy")


def shape_of(fx):
    """-> family, (B, D, h, noise, z, L), act, clip"""
    return str(fx["family"]), tuple(int(v) for v in fx["shape"]), str(fx["act"]), str(fx["clip"])


def aux_params(fx, dtype=torch.float32):
    """The parameters of a fixture, regenerated with the recipe tools/gen_vae_golden.py called (oracle.fixture_params.aux)"""
    family, (B, D, h, nd, z, nl), _, _ = shape_of(fx)
    return P.aux(family, D, nd, h, z, nl, int(fx["seed"]), dtype)


def params64(fx):
    """... as the float64 runs of the generator saw them: the fp32 numbers, widened"""
    return {k: v.double().numpy() for k, v in aux_params(fx).items()}


def restate(fx):
    """-> the fixture's parameters as float64 numpy, cfg = (family, activation, clip) of vae_restate's aux_* functions"""
    family, _, act, clip = shape_of(fx)
    return params64(fx), (family, act, clip)


# ---- 1. the restatement, pinned to the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_restatement_is_the_reference_in_float64(golden_dir, case):
    fx = load(golden_dir, "vae_" + case)
    family, (B, D, h, nd, z, nl), act, clip = shape_of(fx)
    p, cfg = restate(fx)
    x, eps = fx["x"].astype(np.float64), fx["eps"].astype(np.float64)
    for b, beta in BETAS.items():
        out, grads = forward_backward(p, cfg, x, eps, beta, 1.0 / D)
        for k in ("z", "mean", "loss", "recon", "kld"):
            assert rel(out[k], fx[f"{b}/{k}_f64"]) <= TOL64, (b, k)
        assert rel(out["mu0"], fx["mu0_f64"]) <= TOL64 and rel(out["lv0"], fx["lv0_f64"]) <= TOL64
        assert all(g.shape == p[k].shape for k, g in grads.items())
        R.check_grads_f64(grads, fx, b, TOL64, params=p)
    lp = logprob_rows(p, cfg, x, fx["lp/eps"].astype(np.float64)).mean()
    assert rel(lp, fx["lp/value_f64"]) <= TOL64
    # the fp32 fixture is the same computation at fp32's precision
    assert rel(fx["b1/loss"], fx["b1/loss_f64"]) <= 1e-5 and rel(fx["lp/value"], fx["lp/value_f64"]) <= 1e-5
    if clip != "none":       # the clip acts on part of the elements
        raw = lin(p, "aux_encode.reparam.logvar_fn", mlp_fwd(p, "aux_encode.main.", 2 * x - 1 if family == "mnist" else x, act)[0])
        assert 0.0 < np.mean(np.abs(clip_logvar(clip, raw)[1] - 1.0) > 1e-2) < 1.0


@pytest.mark.parametrize("name", TRAJ)
def test_restated_trajectory_is_the_reference_in_float64(golden_dir, name):
    fx = load(golden_dir, "vae_traj_" + name)
    D = shape_of(fx)[1][1]
    p, cfg = restate(fx)
    steps = R.trajectory(fx, p, lambda p, x, eps, beta: forward_backward(p, cfg, x.astype(np.float64), eps.astype(np.float64), beta, 1.0 / D))
    R.check_traj_f64(steps, fx, TOL64, keys=("loss", "kld"))
    assert float(fx["1/beta"]) < 1.0 == float(fx["2/beta"]) == float(fx["3/beta"])          # the ramp ends inside the run


# ---- 2. layout -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES + tuple("traj_" + t for t in TRAJ))
def test_spec_names_and_shapes_are_the_fixtures(golden_dir, name):
    fx = load(golden_dir, "vae_" + name)
    family, (B, D, h, nd, z, nl), act, clip = shape_of(fx)
    spec = layout.aux_vae_spec(family, D, nd, h, z, nl)
    assert [n for n, _ in spec] == [str(n) for n in fx["names"]]
    assert [",".join(str(d) for d in s) for _, s in spec] == [str(s) for s in fx["shapes"]]
    desc = L.ModelDesc(KIND_ID[family], D, nd, h, z, nl, L.ACT[act], L.LOGVAR_CLIP[clip] << L.MODEL_CLIP_Z0_SHIFT)
    total = layout.offsets(spec)[1]
    assert total == L.query("ardae_model_param_floats", desc)
    assert L.query("ardae_model_packed_floats", desc) > total
    sizes = [[L.query("ardae_model_workspace_floats", desc, b, 1, mode) for b in (6, 70, 129)] for mode in (0, 1, 2)]
    sizes.append([L.query("ardae_model_workspace_floats", desc, b, 16, 4) for b in (6, 70, 129)])
    for per_mode in sizes:
        assert 0 < per_mode[0] < per_mode[1] < per_mode[2]
    assert all(a < b for a, b in zip(sizes[0], sizes[1]))               # the training workspace holds aux_encode's and more
    assert L.query("ardae_model_workspace_floats", desc, 6, 2, 1) == L.query("ardae_model_workspace_floats", desc, 6, 1, 3) == 0
    # the module's parameters are the spec, in order, with the reference's state_dict names
    ctor = net.MNISTAuxVAE if family == "mnist" else net.ToyAuxVAE
    mod = ctor(input_dim=D, noise_dim=nd, h_dim=h, z_dim=z, nonlinearity=act, num_hidden_layers=nl, clip_logvar=clip)
    assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == [(n, tuple(s)) for n, s in spec]
    sd = aux_params(fx)
    mod.load_state_dict(sd)
    assert torch.equal(mod.flat_params(), torch.cat([v.reshape(-1) for v in sd.values()]))
    assert mod._desc.flags == desc.flags and mod._desc.kind == desc.kind


def test_parameter_counts_at_the_recipe_widths(golden_dir):
    counts = load(golden_dir, "vae_aux_param_counts")
    assert sorted(counts) == ["auxmnist_784_100_300_32_2", "auxtoy_2_2_64_2_1"]
    for key, want in counts.items():
        family = "mnist" if key.startswith("auxmnist") else "toy"
        D, nd, h, z, nl = (int(v) for v in key.split("_")[1:])
        d = L.ModelDesc(KIND_ID[family], D, nd, h, z, nl, L.ACT["softplus"], 0)
        assert layout.offsets(layout.aux_vae_spec(family, D, nd, h, z, nl))[1] == L.query("ardae_model_param_floats", d) == int(want)
    assert sum(p.numel() for p in net.MNISTAuxVAE().parameters()) == int(counts["auxmnist_784_100_300_32_2"])
    assert sum(p.numel() for p in net.ToyAuxVAE().parameters()) == int(counts["auxtoy_2_2_64_2_1"])
    assert L.query("ardae_vae_head_fused_ok", L.ModelDesc(14, 784, 100, 300, 32, 2, L.ACT["softplus"], 0)) == 1      # the recipe's z head: kind 8's policy
    assert L.query("ardae_vae_head_fused_ok", L.ModelDesc(15, 2, 2, 64, 2, 1, L.ACT["tanh"], 0)) == 0
    assert net.modules.KIND_IDS["vae_auxmnist"] == 14 and net.modules.KIND_IDS["vae_auxtoy"] == 15
    with pytest.raises(NotImplementedError):
        layout.aux_vae_spec("conv", 784, 100, 300, 32, 2)


# ---- 3. descriptor rules and refusals, before any HIP call --------------------------------------------------------------------------
one, big, small = ctypes.c_void_p(64), ctypes.c_size_t(1 << 40), ctypes.c_size_t(16)      # any non-null address: validation fails before it is read
ref = ctypes.byref


def accepted(d):
    lib = L.lib()
    ok = lib.ardae_model_param_floats(ref(d)) > 0
    assert ok == (lib.ardae_model_packed_floats(ref(d)) > 0) == (lib.ardae_model_workspace_floats(ref(d), 3, 1, 1) > 0)
    assert ok == (lib.ardae_model_pack(ref(d), one, None, None) == -1 and b"null pointer" in lib.ardae_last_error())
    return ok


def test_descriptor_rules():
    for k in (14, 15):
        assert accepted(L.ModelDesc(k, 1, 1, 1, 1, 1, 1, 0))                                   # the smallest descriptor
        assert accepted(L.ModelDesc(k, 12, 128, 16, 4, 4, 2, 0)) and not accepted(L.ModelDesc(k, 12, 129, 16, 4, 2, 2, 0))
        assert not accepted(L.ModelDesc(k, 12, 0, 16, 4, 2, 2, 0)) and not accepted(L.ModelDesc(k, 12, -1, 16, 4, 2, 2, 0))
        fails(L.lib().ardae_model_pack(ref(L.ModelDesc(k, 12, 0, 16, 4, 2, 2, 0)), one, one, None), "noise_dim must be 1 .. 128")
        for bad in (L.ModelDesc(k, 12, 3, 16, 0, 2, 2, 0), L.ModelDesc(k, 12, 3, 16, 4, 0, 2, 0), L.ModelDesc(k, 12, 3, 16, 4, 5, 2, 0),
                    L.ModelDesc(k, 0, 3, 16, 4, 2, 2, 0), L.ModelDesc(k, 12, 3, 0, 4, 2, 2, 0)):
            assert not accepted(bad)
            fails(L.lib().ardae_model_pack(ref(bad), one, one, None), "bad dimensions")
        assert not accepted(L.ModelDesc(k, 12, 3, 16, 4, 2, 0, 0)) and not accepted(L.ModelDesc(k, 12, 3, 16, 4, 2, 7, 0))
        # flags: aux_encode's clip code 0 .. 10, nothing else
        for code in range(16):
            assert accepted(L.ModelDesc(k, 12, 3, 16, 4, 2, 2, code << L.MODEL_CLIP_Z0_SHIFT)) == (code <= 10), code
        for bit in range(31):
            if not 8 <= bit <= 11:
                assert not accepted(L.ModelDesc(k, 12, 3, 16, 4, 2, 2, 1 << bit)), bit
                assert not accepted(L.ModelDesc(k, 12, 3, 16, 4, 2, 2, (1 << bit) | (4 << L.MODEL_CLIP_Z0_SHIFT))), bit
        fails(L.lib().ardae_model_pack(ref(L.ModelDesc(k, 12, 3, 16, 4, 2, 2, 1 << L.MODEL_CLIP_Z_SHIFT)), one, one, None), "unknown flags")
    # 13 stays no kind, as 10 does
    for k in (10, 13, 16, -1):
        bad = L.ModelDesc(k, 12, 3, 16, 4, 2, 2, 0)
        assert L.lib().ardae_model_param_floats(ref(bad)) == 0
        fails(L.lib().ardae_model_pack(ref(bad), one, one, None), "kind must be")
        fails(L.lib().ardae_vae_encode_stats(ref(bad), one, one, one, 4, one, big, one, one, None), "kind must be")
    # kind 15 needs the Gaussian decoder's second output, kind 14 does not
    assert L.lib().ardae_model_decode(ref(L.ModelDesc(15, 2, 2, 16, 2, 1, 2, 0)), one, one, one, 4, one, small, one, None, None) < 0
    assert b"needs out1" in L.lib().ardae_last_error()
    fails(L.lib().ardae_model_decode(ref(L.ModelDesc(14, 12, 3, 16, 4, 2, 2, 0)), one, one, one, 4, one, small, one, None, None), "workspace too small")


def test_argument_validation_of_every_entry_point():
    lib = L.lib()
    fwd = lambda d, x, B, wsf, z, losses: lib.ardae_vae_forward(ref(d), one, one, x, None, B, 1.0, 1.0, 7, 0, None, one, wsf, z, None, losses, None)
    fwd_dev = lambda d, st: lib.ardae_vae_forward_dev(ref(d), one, one, one, None, 4, st, 1.0, 7, 0, None, one, big, one, None, one, None)
    bwd = lambda d, B, wsf, g: lib.ardae_vae_backward(ref(d), one, one, one, B, 1.0, 1.0, one, wsf, g, 0.0, None)
    bwd_dev = lambda d, st: lib.ardae_vae_backward_dev(ref(d), one, one, one, 4, st, 1.0, one, big, one, 0.0, None)
    stats = lambda d, B, wsf, mu, lv: lib.ardae_vae_encode_stats(ref(d), one, one, one, B, one, wsf, mu, lv, None)
    head = lambda d, B, variant, mu, eps_out=one: lib.ardae_vae_head(ref(d), one, one, one, None, B, 7, 0, None, variant, mu, one, one, eps_out, one, None)
    draw = lambda d, x, B, k, first, wsf, z, lq, eps=None: lib.ardae_vae_aux_iwae_draw(ref(d), one, one, x, one, one, eps, B, k, 7, 0, 1, first, one, wsf, z, lq,
                                                                                       None, None)
    elbo = lambda d, x, B, first, wsf, rec, kld, eps=None: lib.ardae_vae_aux_elbo_rows(ref(d), one, one, x, eps, B, 7, 0, 1, first, one, wsf, rec, kld, None)
    for k in (14, 15):
        ok = L.ModelDesc(k, 12, 3, 16, 5, 2, 2, 0)
        assert lib.ardae_model_workspace_floats(ref(ok), 4, 1, 1) > lib.ardae_model_workspace_floats(ref(ok), 4, 1, 0) > 0
        assert lib.ardae_model_workspace_floats(ref(ok), 4, 16, 4) > lib.ardae_model_workspace_floats(ref(ok), 4, 8, 4) > 0
        bad = L.ModelDesc(k, 12, 0, 16, 5, 2, 2, 0)
        why = "noise_dim must be"
        assert lib.ardae_vae_head_fused_ok(ref(bad)) == 0
        for rc in (fwd(bad, one, 4, big, one, one), bwd(bad, 4, big, one), stats(bad, 4, big, one, one), head(bad, 4, 0, one)):
            fails(rc, why)
        fails(draw(bad, one, 4, 16, 0, big, one, one), why)
        fails(elbo(bad, one, 4, 0, big, one, one), why)
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
        fails(head(ok, 4, 2, one, eps_out=None), "null pointer")
        fails(head(L.ModelDesc(k, 12, 3, 16, 65, 2, 2, 0), 4, 1, one), "the fused head takes")
        # the two new entry points
        fails(draw(ok, one, 0, 16, 0, big, one, one), "bad batch")
        fails(draw(ok, one, 4, 0, 0, big, one, one), "bad batch")
        fails(draw(ok, one, 1 << 20, 1 << 12, 0, big, one, one), "bad batch")
        fails(draw(ok, one, 4, 16, 0, small, one, one), "workspace too small")
        fails(draw(ok, None, 4, 16, 0, big, one, one), "null pointer")
        fails(draw(ok, one, 4, 16, 0, big, None, one), "null pointer")
        fails(draw(ok, one, 4, 16, 0, big, one, None), "null pointer")
        fails(draw(ok, one, 4, 3, 1, big, one, one), "multiples of 4")                        # 1 x 3 x 3 normals before the chunk: no whole counter
        fails(draw(ok, one, 4, 3, 1, small, one, one, eps=one), "workspace too small")        # ... which injected draws do not need
        fails(draw(L.ModelDesc(k, 12, 3, 16, 129, 2, 2, 0), one, 4, 16, 0, big, one, one), "z_dim <= 128")
        fails(elbo(ok, one, 0, 0, big, one, one), "bad batch")
        fails(elbo(ok, one, 4, 0, small, one, one), "workspace too small")
        fails(elbo(ok, None, 4, 0, big, one, one), "null pointer")
        fails(elbo(ok, one, 4, 0, big, None, one), "null pointer")
        fails(elbo(ok, one, 4, 0, big, one, None), "null pointer")
        fails(elbo(ok, one, 4, 2, big, one, one), "multiples of 4")
        # the implicit models' calls refuse the family: there is no sampler
        fails(lib.ardae_model_encode(ref(ok), one, one, one, None, 4, 1, one, big, one, None), "analytic posterior")
        fails(lib.ardae_model_vae_forward(ref(ok), one, one, one, one, 4, 1, 1.0, one, big, one, one, None), "ardae_vae_forward")
        fails(lib.ardae_model_vae_backward(ref(ok), one, one, one, one, 4, 1, 1.0, 1.0, None, one, big, one, 0.0, None), "ardae_vae_backward")
        fails(lib.ardae_model_vae_backward_decoder(ref(ok), one, one, one, one, 4, 1, 1.0, 1.0, one, big, None), "no split backward")
        fails(lib.ardae_model_encode_hidden(ref(ok), one, one, one, 4, one, big, one, None, None), "hidden1a context")
    # the kinds of the other families at the new entry points
    for k in (8, 3, 13):
        other = L.ModelDesc(k, 12, 0 if k == 8 else 3, 16, 4, 2, 2, 0)
        fails(draw(other, one, 4, 16, 0, big, one, one), "kind must be 14 (MNISTAuxVAE) or 15 (ToyAuxVAE)")
        fails(elbo(other, one, 4, 0, big, one, one), "kind must be 14 (MNISTAuxVAE) or 15 (ToyAuxVAE)")
    pair = lambda mu, B, n, out: lib.ardae_vae_pair_kld_rows(mu, one, one, one, B, n, out, None)
    fails(pair(one, 0, 4, one), "bad batch")
    fails(pair(one, 4, 0, one), "bad batch")
    fails(pair(one, 4, 129, one), "bad batch")
    fails(pair(None, 4, 4, one), "null pointer")
    fails(pair(one, 4, 4, None), "null pointer")


# ---- 4. the module surface -----------------------------------------------------------------------------------------------------------
def test_module_surface_and_refusals():
    m = net.MNISTAuxVAE()
    assert (m.input_dim, m.noise_dim, m.h_dim, m.z_dim, m.nonlinearity, m.num_hidden_layers, m.enc_type, m.clip_logvar, m.do_xavier, m.do_m5bias) == \
        (784, 100, 300, 32, "softplus", 2, "simple", None, True, False)
    assert isinstance(m, net.GaussianVAE) and m.latent_dim == 32 and m._eps_width == 132
    p = {k: v.detach() for k, v in m.named_parameters()}
    assert all(float(v.abs().max()) == 0.0 for k, v in p.items() if k.endswith("bias"))                       # do_xavier: weight_init
    bound = math.sqrt(6.0 / (884 + 300))
    assert 0.5 * bound < float(p["encode.fc.layers.0.weight"].abs().max()) <= bound
    m5 = net.MNISTAuxVAE(input_dim=12, noise_dim=5, h_dim=16, z_dim=4, do_xavier=False, do_m5bias=True, clip_logvar="none")
    assert m5.clip_logvar is None and m5._desc.flags == 0                                                      # 'none' means None (vae/auxmnist.py:291)
    b = dict(m5.named_parameters())["decode.reparam.logit_fn.bias"].detach()
    assert float(b.min()) == float(b.max()) == -5.0
    assert float(dict(m5.named_parameters())["aux_decode.fc.fc.bias"].detach().abs().max()) > 0.0
    torch.manual_seed(0)
    t = net.ToyAuxVAE(h_dim=256)
    assert (t.input_dim, t.noise_dim, t.h_dim, t.z_dim, t.nonlinearity, t.num_hidden_layers, t.init, t.enc_type, t.clip_logvar) == \
        (2, 2, 256, 2, "tanh", 1, "gaussian", "simple", None)
    w = dict(t.named_parameters())["decode.reparam.mean_fn.weight"].detach()
    assert float(w.abs().max()) > 1.5 and abs(float(w.std()) - 1.0) < 0.15                                     # N(0, 1), not U(+-1/16)
    assert net.ToyAuxVAE(clip_logvar="spm6")._desc.flags == 4 << L.MODEL_CLIP_Z0_SHIFT
    for ctor in (net.MNISTAuxVAE, net.ToyAuxVAE):
        with pytest.raises(NotImplementedError, match="enc_type 'mlp'"):
            ctor(enc_type="mlp")
        with pytest.raises(NotImplementedError, match="clip_logvar 'sigmoid'"):
            ctor(clip_logvar="sigmoid")
        with pytest.raises(NotImplementedError, match="normal_energy_func"):
            ctor(energy_func=lambda z: z)
        with pytest.raises(NotImplementedError, match="gelu"):
            ctor(nonlinearity="gelu")
        with pytest.raises(ValueError, match="noise_dim"):
            ctor(noise_dim=0)
        with pytest.raises(ValueError, match="noise_dim"):
            ctor(noise_dim=129)
    for mod in (m5, t):       # execution on the CPU is refused
        with pytest.raises(RuntimeError, match="no CPU path"):
            mod(torch.zeros(3, mod.input_dim))
        with pytest.raises(RuntimeError, match="no CPU path"):
            mod.logprob(torch.zeros(3, mod.input_dim), sample_size=4)
        with pytest.raises(RuntimeError, match="no CPU path"):
            mod.encode_stats(torch.zeros(3, mod.input_dim))
        with pytest.raises(RuntimeError, match="no CPU path"):
            mod.generate(2)
        with pytest.raises(RuntimeError, match="no CPU path"):
            net.VaeEngine(mod, net.VaeConfig(), batch_size=4)
    # the engine / evaluator type checks keep naming the existing classes, and name the new ones
    with pytest.raises(TypeError, match="VaeEngine drives.*net.MNISTVAE / net.ToyVAE / net.MNISTConvVAE / net.MNISTResConvVAE.*net.MNISTAuxVAE"):
        net.VaeEngine(net.MNISTAuxIPVAE(input_dim=12, noise_dim=4, h_dim=16, z_dim=4), net.VaeConfig(), batch_size=4)
    with pytest.raises(TypeError, match="net.MNISTVAE / net.ToyVAE / net.MNISTConvVAE / net.MNISTResConvVAE.*net.ToyAuxVAE"):
        net.GaussianIwaeEvaluator(net.ToyAuxIPVAE(), 16)
    ev = net.GaussianIwaeEvaluator(m5, 16)
    assert ev.aux and ev.sd == 5 and not ev.gaussian and net.GaussianIwaeEvaluator(t, 16).gaussian
    with pytest.raises(NotImplementedError, match="z_dim 129 > 128"):
        net.GaussianIwaeEvaluator(net.MNISTAuxVAE(input_dim=12, noise_dim=5, h_dim=16, z_dim=129), 16)
    wide = net.MNISTAuxVAE(input_dim=12, noise_dim=5, h_dim=16, z_dim=100)      # wider than kind 8's draw takes: the aux draw's own limit holds
    assert net.GaussianIwaeEvaluator(wide, 16).plan(5) == [(0, 5)]
