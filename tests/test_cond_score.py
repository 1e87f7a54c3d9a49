"""Plain conditional DAE score networks (ardae_cdae_desc.kind 10 / 11) and the conditional score engine: layout, argument validation, module
and engine surface, and the float64 restatement of the two networks that the GPU tests lean on (tests/score_restate.py) - pinned here to the reference's fp64
fixtures.  No GPU needed."""
import ctypes
import math
import os

import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import layout
from score_restate import CDAE, dims, inputs_of, load, loss_and_grads, rel, score, state_dict_of, std_of

KIND_ID = CDAE.kind_id
fixtures = CDAE.fixtures
# (kind, (d, c, h, L)) -> parameter floats, packed floats, workspace floats at (B, S) = (4, 8) without / with gradients; recorded like DAE_SIZES
# of test_abi.py (these kinds share the layout, workspace and gradient-list code of kinds 0 / 1: what they do NOT take of it is pinned here)
CDAE_PLAIN_SIZES = [("grad", (2, 2, 64, 3), 33665, 70656, (25856, 85824)), ("grad", (3, 5, 100, 2), 51501, 141824, (27328, 107264)),
                    ("grad", (32, 32, 256, 3), 543233, 1081344, (104576, 753024)), ("grad", (2, 2, 64, 1), 8705, 21504, (8960, 26688)),
                    ("res", (2, 2, 64, 3), 33730, 73216, (25856, 86016)), ("res", (3, 5, 100, 2), 51703, 146176, (27328, 107648)),
                    ("res", (32, 32, 256, 3), 551200, 1097728, (104576, 761280)), ("res", (2, 2, 64, 1), 8770, 24064, (8960, 26880))]


def build(fx, **kw):
    _, _, d, c, h, nl = dims(fx)
    return CDAE.module(str(fx["kind"]), d, h, nl, str(fx["act"]), c, **kw)


# ---- 1. layout ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,args,params,packed,workspace", CDAE_PLAIN_SIZES, ids=[f"{r[0]}-d{r[1][0]}-c{r[1][1]}-h{r[1][2]}-L{r[1][3]}" for r in CDAE_PLAIN_SIZES])
def test_layout_matches_c_side(kind, args, params, packed, workspace):
    d, c, h, nl = args
    total = layout.offsets(layout.cdae_plain_spec(kind, d, c, h, nl))[1]
    desc = L.CdaeDesc(KIND_ID[kind], d, c, h, nl, L.ACT["softplus"])
    assert L.query("ardae_cdae_param_floats", desc) == total == params
    assert L.query("ardae_cdae_packed_floats", desc) == packed
    assert tuple(L.query("ardae_cdae_workspace_floats", desc, 4, 8, g) for g in (0, 1)) == workspace
    # the AR-DAE sibling has the sigma column on top: h more parameters and a packed copy of it, in the same workspace
    sib = L.CdaeDesc(KIND_ID[kind] - 10, d, c, h, nl, L.ACT["softplus"])
    assert L.query("ardae_cdae_param_floats", sib) == total + h == layout.offsets(layout.cdae_spec(kind, d, c, h, nl))[1]
    assert packed + h <= L.query("ardae_cdae_packed_floats", sib) < packed + h + 64      # (pieces of the packed image are padded)
    assert tuple(L.query("ardae_cdae_workspace_floats", sib, 4, 8, g) for g in (0, 1)) == workspace
    # cdae_spec is untouched: [h, 2h + 1] first layer
    first = "neglogprob.layers.0.weight" if kind == "grad" else "dae.layers.0.weight"
    assert dict(layout.cdae_spec(kind, d, c, h, nl))[first] == (h, 2 * h + 1) and dict(layout.cdae_plain_spec(kind, d, c, h, nl))[first] == (h, 2 * h)


def test_layout_names_and_shapes_are_the_fixtures(golden_dir):
    for path in fixtures(golden_dir):
        fx = load(path)
        (_, _, d, c, h, nl), kind = dims(fx), str(fx["kind"])
        sd = state_dict_of(fx)
        spec = layout.cdae_plain_spec(kind, d, c, h, nl)
        assert [(n, tuple(s)) for n, s in spec] == [(k, tuple(v.shape)) for k, v in sd.items()], path
        assert layout.offsets(spec)[1] == sum(v.numel() for v in sd.values()) == L.query("ardae_cdae_param_floats", L.CdaeDesc(KIND_ID[kind], d, c, h, nl, 2))
    for kind in ("grad", "res"):
        fx = load(os.path.join(golden_dir, f"cdae_plain_traj_{kind}.npz"))
        spec = layout.cdae_plain_spec(kind, int(fx["cfg/d"]), int(fx["cfg/c"]), int(fx["cfg/h"]), int(fx["cfg/L"]))
        assert [(n, tuple(s)) for n, s in spec] == [(k, tuple(v.shape)) for k, v in state_dict_of(fx).items()]
    with pytest.raises(NotImplementedError):
        layout.cdae_plain_spec("mlp", 2, 2, 64, 3)


# ---- 2. validation before any HIP call ---------------------------------------------------------------------------------------------
def test_argument_validation_of_the_plain_conditional_entry_points():
    lib = L.lib()
    one, big = ctypes.c_void_p(64), ctypes.c_size_t(1 << 40)      # any non-null address: validation must fail before it is dereferenced
    ref = ctypes.byref

    def fails(rc, fragment):
        assert rc < 0
        assert fragment.encode() in lib.ardae_last_error(), lib.ardae_last_error()

    for k in (10, 11):
        ok = L.CdaeDesc(k, 2, 2, 64, 3, 2)
        assert lib.ardae_cdae_param_floats(ref(ok)) > 0 and lib.ardae_cdae_packed_floats(ref(ok)) > 0 and lib.ardae_cdae_workspace_floats(ref(ok), 4, 8, 1) > 0
        # a context is required: in the descriptor and as a pointer
        bad = L.CdaeDesc(k, 2, 0, 64, 3, 2)
        assert lib.ardae_cdae_param_floats(ref(bad)) == lib.ardae_cdae_packed_floats(ref(bad)) == lib.ardae_cdae_workspace_floats(ref(bad), 4, 8, 1) == 0
        fails(lib.ardae_cdae_pack(ref(bad), one, one, None), "context_dim >= 1")
        fails(lib.ardae_cdae_loss_grads(ref(bad), one, one, one, one, one, one, 4, 8, one, big, one, one, None, None), "context_dim >= 1")
        fails(lib.ardae_cdae_loss_grads(ref(ok), one, one, one, one, one, None, 4, 8, one, big, one, one, None, None), "null pointer")
        fails(lib.ardae_cdae_score(ref(ok), one, one, one, None, None, 4, 8, one, big, one, None), "null pointer")
        # the loss needs its sigma; the score does not (the null output is the first thing it then misses)
        fails(lib.ardae_cdae_loss_grads(ref(ok), one, one, one, None, one, one, 4, 8, one, big, one, one, None, None), "null pointer")
        fails(lib.ardae_cdae_loss_grads(ref(ok), one, one, None, one, one, one, 4, 8, one, big, one, one, None, None), "null pointer")
        fails(lib.ardae_cdae_score(ref(ok), one, one, one, None, one, 4, 8, one, big, None, None), "score_out is NULL")
        fails(lib.ardae_cdae_loss_grads(ref(ok), one, one, one, one, one, one, 0, 8, one, big, one, one, None, None), "bad batch")
        fails(lib.ardae_cdae_loss_grads(ref(ok), one, one, one, one, one, one, 4, 8, one, ctypes.c_size_t(16), one, one, None, None), "workspace too small")
        fails(lib.ardae_cdae_score(ref(ok), one, one, one, None, one, 4, 8, one, ctypes.c_size_t(16), one, None), "workspace too small")
        # the kernels that draw sigma refuse the plain kinds, whatever the shape
        wide = L.CdaeDesc(k, 32, 32, 256, 3, 2)
        sib = L.CdaeDesc(k - 10, 32, 32, 256, 3, 2)
        assert lib.ardae_cdae_perturb_fused_ok(ref(sib), 256, 1) == 1 and lib.ardae_cdae_perturb_fused_ok(ref(wide), 256, 1) == 0
        assert lib.ardae_dae_perturb_fused_ok(ref(ok), 10) == 0 and lib.ardae_dae_perturb_fused_ok(ref(wide), 10) == 0
        fails(lib.ardae_cdae_perturb_loss_grads(ref(wide), one, one, one, one, one, 4, 256, 1.0, 0.1, 7, 0, 1, None, 0, one, one, one, one, one, big, one, one,
                                                None), "not eligible")
        fails(lib.ardae_dae_perturb_loss_grads(ref(ok), one, one, one, 4, 8, 1.0, 7, 0, 1, None, 0, one, one, one, one, big, one, one, None), "not eligible")
    # 4, 5, 8 and 9 are not kinds
    for k in (4, 5, 8, 9, 12, -1):
        for c in (0, 2):
            bad = L.CdaeDesc(k, 2, c, 64, 3, 2)
            assert lib.ardae_cdae_param_floats(ref(bad)) == lib.ardae_cdae_packed_floats(ref(bad)) == lib.ardae_cdae_workspace_floats(ref(bad), 4, 8, 1) == 0
            fails(lib.ardae_cdae_pack(ref(bad), one, one, None), "kind must be")
            fails(lib.ardae_cdae_score(ref(bad), one, one, one, one, one, 4, 8, one, big, one, None), "kind must be")
            assert lib.ardae_cdae_perturb_fused_ok(ref(bad), 256, 1) == 0
    # the two perturbation entries
    pert = lambda lat, z0, eps, B, nz, nstd, z, xbar, sg: lib.ardae_latent_noise_perturb(lat, z0, eps, B, nz, nstd, z, 1.0, 0.5, None, xbar, sg, None)
    fails(pert(None, one, one, 4, 8, 2, 2, one, one), "null pointer")
    fails(pert(one, None, one, 4, 8, 2, 2, one, one), "null pointer")
    fails(pert(one, one, None, 4, 8, 2, 2, one, one), "null pointer")
    fails(pert(one, one, one, 4, 8, 2, 2, None, one), "null pointer")
    fails(pert(one, one, one, 4, 8, 2, 2, one, None), "null pointer")
    fails(pert(one, one, one, 0, 8, 2, 2, one, one), "bad batch")
    fails(pert(one, one, one, 4, 0, 2, 2, one, one), "bad batch")
    fails(pert(one, one, one, 4, 8, 0, 2, one, one), "bad batch")
    fails(pert(one, one, one, 4, 8, 2, 0, one, one), "bad batch")
    fails(pert(one, one, one, 1 << 16, 1 << 10, 1 << 3, 4, one, one), "bad batch")                        # 2^31 elements
    draw = lambda lat, z0, B, nz, nstd, z, first, xbar, sg, eps: lib.ardae_latent_noise_perturb_draw(lat, z0, B, nz, nstd, z, 1.0, 0.5, None, 7, 1, first,
                                                                                                  xbar, sg, eps, None)
    fails(draw(None, one, 4, 8, 2, 2, 0, one, one, one), "null pointer")
    fails(draw(one, None, 4, 8, 2, 2, 0, one, one, one), "null pointer")
    fails(draw(one, one, 4, 8, 2, 2, 0, None, one, one), "null pointer")
    fails(draw(one, one, 4, 8, 2, 2, 0, one, None, one), "null pointer")
    fails(draw(one, one, 4, 8, 2, 2, 0, one, one, None), "null pointer")
    fails(draw(one, one, 0, 8, 2, 2, 0, one, one, one), "bad batch")
    fails(draw(one, one, 4, 8, 2, 0, 0, one, one, one), "bad batch")
    fails(draw(one, one, 1 << 16, 1 << 10, 1 << 3, 4, 0, one, one, one), "bad batch")
    fails(draw(one, one, 4, 8, 2, 2, 6, one, one, one), "first_row must be a multiple of 4")
    assert lib.ardae_latent_noise_perturb_draw_ok(1, 1, 1) == lib.ardae_latent_noise_perturb_draw_ok(12, 1, 3) == 1
    assert lib.ardae_latent_noise_perturb_draw_ok(0, 1, 2) == lib.ardae_latent_noise_perturb_draw_ok(8, 0, 2) == lib.ardae_latent_noise_perturb_draw_ok(8, 1, 0) == 0
    assert lib.ardae_abi_version() == 1


# ---- 3. modules --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["grad", "res"])
def test_module_defaults_are_the_references(kind, golden_dir):
    cls = CDAE.classes[kind]
    last = "neglogprob" if kind == "grad" else "dae"
    names = ["ctx_encode.fc.weight", "ctx_encode.fc.bias", "inp_encode.fc.weight", "inp_encode.fc.bias",
             f"{last}.layers.0.weight", f"{last}.layers.0.bias", f"{last}.fc.weight", f"{last}.fc.bias"]
    m = cls()
    assert issubclass(cls, net.ConditionalDAE) and not issubclass(cls, net.ConditionalARDAE)
    assert (m.input_dim, m.h_dim, m.context_dim, m.std, m.num_hidden_layers, m.nonlinearity, m.noise_type, m.enc_input, m.enc_ctx) == \
        (2, 128, 2, 0.01, 1, "tanh", "gaussian", True, True)
    assert [n for n, _ in m.named_parameters()] == names == list(m.state_dict())
    assert m.state_dict()[names[4]].shape == (128, 256)                       # [W1a | W1c]: no sigma column
    assert int(m._desc.kind) == KIND_ID[kind] and int(m._desc.context_dim) == 2
    assert set(m._no_grad_names) == ({"neglogprob.fc.bias"} if kind == "grad" else set())
    # nn.Linear's default init, which the reference constructor leaves in place: U(+-1/sqrt(fan_in)) for weight and bias, filling the range
    torch.manual_seed(3)
    m = cls(input_dim=3, context_dim=5, h_dim=100, num_hidden_layers=2, nonlinearity="elu")
    fx = load(os.path.join(golden_dir, f"cdae_plain_{kind}_b5_s12_d3_elu.npz"))
    sd_ref, sd = state_dict_of(fx), m.state_dict()
    assert [(k, v.shape) for k, v in sd.items()] == [(k, v.shape) for k, v in sd_ref.items()]
    for k, v in sd.items():
        bound = 1.0 / math.sqrt(sd[k[:-len("bias")] + "weight"].shape[1] if k.endswith("bias") else v.shape[1])
        for t in (v, sd_ref[k]):
            assert float(t.abs().max()) <= bound and (t.numel() < 50 or float(t.abs().max()) > 0.9 * bound), k
    for bad in (dict(noise_type="laplace"), dict(noise_type="uniform"), dict(enc_input=False), dict(enc_ctx=False), dict(nonlinearity="gelu")):
        with pytest.raises(NotImplementedError):
            cls(**bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cls(h_dim=16)(torch.zeros(4, 3, 2), torch.zeros(4, 1, 2), 0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cls(h_dim=16).glogprob(torch.zeros(4, 3, 2), torch.zeros(4, 1, 2))


def test_load_state_dict_keeps_flat_views(golden_dir):
    for path in fixtures(golden_dir):
        fx = load(path)
        m = build(fx)
        sd = state_dict_of(fx)
        m.load_state_dict(sd)
        off = 0
        for n, p in m.named_parameters():
            assert p.data_ptr() == m.flat_params().data_ptr() + 4 * off and torch.equal(p, sd[n])
            off += p.numel()
        assert off == m.flat_params().numel() == L.query("ardae_cdae_param_floats", m._desc)


# ---- 4. configs and refusals -------------------------------------------------------------------------------------------------------
def test_config_and_network_must_belong_together():
    class OnDevice:                      # the checks come right after _require_gpu(): no device is touched before them
        def __init__(self, m):
            self._desc, self._require_gpu = m._desc, lambda: None
    kw = dict(h_dim=16, nonlinearity="softplus")
    for m, cfg in ((net.MLPGradCDAE(**kw), net.ScoreConfig()), (net.MLPResCDAE(**kw), net.ScoreConfig()),
                   (net.MLPGradCARDAE(**kw), net.DaeConfig()), (net.MLPResCARDAE(**kw), net.DaeConfig()), (net.MLPGradCDAE(**kw), net.TrainConfig())):
        with pytest.raises(TypeError, match="(?s)ScoreConfig.*DaeConfig|DaeConfig.*ScoreConfig"):
            net.ArdaeCondScoreEngine(OnDevice(m), cfg, 8, 4)
    for m in (net.MLPGradARDAE(h_dim=16), net.MLPResDAE(h_dim=16)):
        with pytest.raises(TypeError, match="conditional"):
            net.ArdaeCondScoreEngine(OnDevice(m), net.ScoreConfig(), 8, 4)
    # the unconditional engine and the VAE loop's engine keep refusing them
    for m in (net.MLPGradCDAE(**kw), net.MLPResCDAE(**kw)):
        with pytest.raises(TypeError, match="unconditional"):
            net.ArdaeScoreEngine(OnDevice(m), net.DaeConfig(), 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        net.ArdaeCondScoreEngine(net.MLPGradCDAE(**kw), net.DaeConfig(), 8, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        net.ArdaeCondScoreEngine(net.MLPResCARDAE(**kw), net.ScoreConfig(), 8, 4)


# ---- 5. the float64 restatement reproduces every fp64 fixture ----------------------------------------------------------------------
def test_restatement_reproduces_the_fp64_fixtures(golden_dir):
    for path in fixtures(golden_dir):
        fx = load(path)
        kind, act, S = str(fx["kind"]), str(fx["act"]), dims(fx)[1]
        p = {k: v.double() for k, v in state_dict_of(fx).items()}
        x, ctx, eps = inputs_of(fx, torch.float64)
        loss, grads = loss_and_grads(kind, p, act, x, std_of(fx, torch.float64), eps, False, ctx, S)
        assert abs(float(loss) - float(fx["loss_f64"])) <= 1e-12 * abs(float(fx["loss_f64"])), path
        for n, g in grads.items():
            if f"g_f64/{n}/none" in fx:
                assert g is None and n == "neglogprob.fc.bias", (path, n)
            else:
                assert rel(g, fx["g_f64/" + n]) <= 1e-12, (path, n, rel(g, fx["g_f64/" + n]))
        assert rel(score(kind, p, act, x, None, ctx, S).reshape(fx["glog_f64"].shape), fx["glog_f64"]) <= 1e-12, path
    assert sorted(load(p)["std"].ndim for p in fixtures(golden_dir)) == [0] * 6 + [2] * 4         # scalar and [B*S, 1] noise levels


def traj_step_inputs(fx, s, dtype):
    """(u rows [B*S*nsigma, d], ctx [B, c], eps) of step s: centre, scale, every sample nsigma times (ivae_ardae.py:753-767)"""
    c = {k[4:]: v for k, v in fx.items() if k.startswith("cfg/")}
    B, S, ns, d = int(c["B"]), int(c["S"]), int(c["nsigma"]), int(c["d"])
    latent, mean = torch.tensor(fx[f"{s}/latent"]).to(dtype), torch.tensor(fx[f"{s}/mean"]).to(dtype)
    u = float(c["std_scale"]) * (latent - mean[:, None, :])
    return u.unsqueeze(2).expand(B, S, ns, d).reshape(B * S * ns, d), torch.tensor(fx[f"{s}/ctx"]).to(dtype), torch.tensor(fx[f"{s}/eps"]).to(dtype)


def test_restatement_reproduces_the_fp64_trajectory(golden_dir):
    """The update restated (schedule, centring, broadcast, loss, torch.optim.Adam) in float64 on the fixture's samples / eps."""
    for kind in ("grad", "res"):
        fx = load(os.path.join(golden_dir, f"cdae_plain_traj_{kind}.npz"))
        c = {k[4:]: v for k, v in fx.items() if k.startswith("cfg/")}
        act, rows_per_ctx = str(c["act"]), int(c["S"]) * int(c["nsigma"])
        p = {k: v.double().requires_grad_(True) for k, v in state_dict_of(fx).items()}
        opt = torch.optim.Adam(list(p.values()), lr=float(c["lr"]))
        sigmas = []
        for s in range(int(c["steps"])):
            sigma = net.dae_sigma(float(c["sigma_max"]), float(c["sigma_min"]), int(c["sigma_annealing"]), s)
            assert sigma == float(fx[f"{s}/sigma"])
            sigmas.append(sigma)
            u, ctx, eps = traj_step_inputs(fx, s, torch.float64)
            xbar = (u + sigma * eps).requires_grad_(True)
            loss = torch.nn.functional.mse_loss(sigma * score(kind, p, act, xbar, None, ctx, rows_per_ctx, create_graph=True), -eps)
            opt.zero_grad()
            loss.backward()
            opt.step()
            assert abs(float(loss.detach()) - float(fx[f"{s}/loss_f64"])) <= 1e-12 * abs(float(fx[f"{s}/loss_f64"])), (kind, s)
            for n, v in p.items():
                assert rel(v.detach(), fx[f"{s}/p_f64/{n}"]) <= 1e-12, (kind, s, n)
        assert sigmas[-3:] == [float(c["sigma_min"])] * 3 and sigmas[0] > sigmas[1] > sigmas[2] > sigmas[3]      # the ramp ends inside the run
