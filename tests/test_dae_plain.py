"""Plain DAE score networks (ardae_cdae_desc.kind 6 / 7, notebooks/dae_toy.ipynb): layout, argument validation, the sigma schedule on
the host, module and engine surface, and the float64 restatement of the two networks that the GPU tests lean on (tests/score_restate.py) - pinned here to the
reference's fp64 fixtures.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import layout
from ardae_amd.engine_common import _FlatOpt
from score_restate import DAE, load, loss_and_grads, rel, score, state_dict_of, std_of

KIND_ID = DAE.kind_id
fixtures = DAE.fixtures
# parameter counts of the reference classes, (d, h, L) -> (grad, res)
REFERENCE_COUNTS = {(2, 128, 3): (33537, 33666), (2, 256, 3): (132609, 132866), (3, 100, 2): (10601, 10803), (2, 64, 3): (8577, 8642)}
# sigma_max 5.0, sigma_min 0.05, sigma_annealing 4000: i -> (the Python float, numpy.float32 of it)
SCHEDULE = {0: (4.998762500000001, 4.998762607574463), 1999: (2.525, 2.5250000953674316), 3998: (0.051237499999999866, 0.051237501204013824),
            3999: (0.05, 0.05000000074505806), 4000: (0.05, 0.05000000074505806), 123456: (0.05, 0.05000000074505806)}


# ---- 1. layout ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["grad", "res"])
def test_layout_totals_match_c_side_and_reference_counts(kind):
    for (d, h, nl), counts in REFERENCE_COUNTS.items():
        total = layout.offsets(layout.dae_plain_spec(kind, d, h, nl))[1]
        desc = L.CdaeDesc(KIND_ID[kind], d, 0, h, nl, L.ACT["softplus"])
        assert total == L.query("ardae_cdae_param_floats", desc) == counts[kind == "res"]
        # the AR-DAE sibling has the sigma column on top: h more parameters, and a packed copy of it
        sib = L.CdaeDesc(KIND_ID[kind] - 4, d, 0, h, nl, L.ACT["softplus"])
        assert L.query("ardae_cdae_param_floats", sib) == total + h
        assert total < L.query("ardae_cdae_packed_floats", desc) < L.query("ardae_cdae_packed_floats", sib)
        assert L.query("ardae_cdae_workspace_floats", desc, 16, 4, 1) > L.query("ardae_cdae_workspace_floats", desc, 16, 4, 0) > 0
        assert L.query("ardae_cdae_workspace_floats", desc, 16, 4, 1) == L.query("ardae_cdae_workspace_floats", desc, 64, 1, 1)    # N = B S in any factorisation
    # dae_spec is untouched: [h, d + 1] first layer
    assert layout.dae_spec(kind, 2, 64, 3)[0][1] == (64, 3) and layout.dae_plain_spec(kind, 2, 64, 3)[0][1] == (64, 2)


def test_layout_names_and_shapes_are_the_fixtures(golden_dir):
    for path in fixtures(golden_dir):
        fx = load(path)
        (_, d, h, nl), kind = (int(v) for v in fx["shape"]), str(fx["kind"])
        sd = state_dict_of(fx)
        assert [(n, tuple(s)) for n, s in layout.dae_plain_spec(kind, d, h, nl)] == [(k, tuple(v.shape)) for k, v in sd.items()], path
    for kind in ("grad", "res"):
        fx = load(os.path.join(golden_dir, f"dae_plain_traj_{kind}.npz"))
        spec = layout.dae_plain_spec(kind, int(fx["cfg/d"]), int(fx["cfg/h"]), int(fx["cfg/L"]))
        assert [(n, tuple(s)) for n, s in spec] == [(k, tuple(v.shape)) for k, v in state_dict_of(fx).items()]


# ---- 2. validation before any HIP call ---------------------------------------------------------------------------------------------
def test_argument_validation_of_the_plain_entry_points():
    lib = L.lib()
    one, big = ctypes.c_void_p(64), ctypes.c_size_t(1 << 40)      # any non-null address: validation must fail before it is dereferenced
    ref = ctypes.byref

    def fails(rc, fragment):
        assert rc < 0
        assert fragment.encode() in lib.ardae_last_error(), lib.ardae_last_error()

    for k in (6, 7):
        ok = L.CdaeDesc(k, 2, 0, 64, 3, 2)
        assert lib.ardae_cdae_param_floats(ref(ok)) > 0 and lib.ardae_cdae_packed_floats(ref(ok)) > 0 and lib.ardae_cdae_workspace_floats(ref(ok), 4, 8, 1) > 0
        # a context, or a context pointer, is an error
        bad = L.CdaeDesc(k, 2, 1, 64, 3, 2)
        assert lib.ardae_cdae_param_floats(ref(bad)) == lib.ardae_cdae_packed_floats(ref(bad)) == lib.ardae_cdae_workspace_floats(ref(bad), 4, 8, 1) == 0
        fails(lib.ardae_cdae_pack(ref(bad), one, one, None), "context_dim must be 0")
        fails(lib.ardae_cdae_loss_grads(ref(bad), one, one, one, one, one, None, 4, 8, one, big, one, one, None, None), "context_dim must be 0")
        fails(lib.ardae_cdae_loss_grads(ref(ok), one, one, one, one, one, one, 4, 8, one, big, one, one, None, None), "ctx must be NULL")
        fails(lib.ardae_cdae_score(ref(ok), one, one, one, None, one, 4, 8, one, big, one, None), "ctx must be NULL")
        # the loss needs its sigma; the score does not (the null workspace is the first thing it then misses)
        fails(lib.ardae_cdae_loss_grads(ref(ok), one, one, one, None, one, None, 4, 8, one, big, one, one, None, None), "null pointer")
        fails(lib.ardae_cdae_loss_grads(ref(ok), one, one, None, one, one, None, 4, 8, one, big, one, one, None, None), "null pointer")
        fails(lib.ardae_cdae_score(ref(ok), one, one, one, None, None, 4, 8, one, big, None, None), "score_out is NULL")
        fails(lib.ardae_cdae_loss_grads(ref(ok), one, one, one, one, one, None, 0, 8, one, big, one, one, None, None), "bad batch")
        fails(lib.ardae_cdae_loss_grads(ref(ok), one, one, one, one, one, None, 4, 8, one, ctypes.c_size_t(16), one, one, None, None), "workspace too small")
        fails(lib.ardae_cdae_score(ref(ok), one, one, one, None, None, 4, 8, one, ctypes.c_size_t(16), one, None), "workspace too small")
        # the AR-DAE front end refuses the plain kinds
        fails(lib.ardae_dae_perturb_loss_grads(ref(ok), one, one, one, 4, 8, 1.0, 7, 0, 1, None, 0, one, one, one, one, big, one, one, None), "not eligible")
        assert lib.ardae_dae_perturb_fused_ok(ref(ok), 10) == 0 and lib.ardae_cdae_perturb_fused_ok(ref(ok), 256, 1) == 0
    # kinds 4 / 5 are no kinds
    for k in (4, 5, 8, -1):
        bad = L.CdaeDesc(k, 2, 0, 64, 3, 2)
        assert lib.ardae_cdae_param_floats(ref(bad)) == lib.ardae_cdae_packed_floats(ref(bad)) == lib.ardae_cdae_workspace_floats(ref(bad), 4, 8, 1) == 0
        fails(lib.ardae_cdae_pack(ref(bad), one, one, None), "kind must be")
        fails(lib.ardae_cdae_score(ref(bad), one, one, one, one, None, 4, 8, one, big, one, None), "kind must be")
        assert lib.ardae_dae_perturb_fused_ok(ref(bad), 10) == 0
    # the unfused perturbation and the schedule
    pert = lambda x, eps, B, ns, d, xbar, sg: lib.ardae_dae_noise_perturb(x, eps, B, ns, d, 0.5, None, xbar, sg, None)
    fails(pert(None, one, 4, 8, 2, one, one), "null pointer")
    fails(pert(one, one, 4, 8, 2, one, None), "null pointer")
    fails(pert(one, one, 0, 8, 2, one, one), "bad batch")
    fails(pert(one, one, 4, 8, 0, one, one), "bad batch")
    fails(pert(one, one, 1 << 16, 1 << 13, 4, one, one), "bad batch")                        # 2^31 elements
    fails(lib.ardae_dae_state_advance(None, 16, 5e-3, 0.9, 0.999, 5.0, 0.05, 4000, None), "null state")
    fails(lib.ardae_dae_state_advance(None, 16, 5e-3, 0.9, 0.999, 5.0, 0.05, 0, None), "null state")


# ---- 3. the schedule on the host ---------------------------------------------------------------------------------------------------
def test_host_schedule_is_the_notebooks_bit_for_bit():
    for i, (as_double, as_float) in SCHEDULE.items():
        v = net.dae_sigma(5.0, 0.05, 4000, i)
        assert v == as_double and float(np.float32(v)) == as_float, (i, repr(v))
        # restated: the notebook's two lines
        perc = min((i + 1) / float(4000), 1.0)
        assert v == 5.0 * (1 - perc) + 0.05 * perc
    assert net.dae_sigma(5.0, 0.05, 0, 17) == net.dae_sigma(5.0, 0.05, -3, 0) == 0.05         # no ramp: the constant sigma_min
    assert [net.dae_sigma(1.0, 0.1, 4, i) for i in range(6)] == [0.775, 0.55, 0.325, 0.1, 0.1, 0.1]
    with pytest.raises(ValueError, match="whole number"):
        net.DaeConfig(sigma_annealing=2.5)


# ---- 4. modules and engine surface -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,names", [(net.MLPGradDAE, ["neglogprob.layers.0.weight", "neglogprob.layers.0.bias", "neglogprob.fc.weight", "neglogprob.fc.bias"]),
                                       (net.MLPResDAE, ["main.layers.0.weight", "main.layers.0.bias", "main.fc.weight", "main.fc.bias"])])
def test_module_defaults_are_the_references(cls, names):
    m = cls()
    assert (m.input_dim, m.h_dim, m.std, m.num_hidden_layers, m.nonlinearity, m.noise_type) == (2, 1000, 0.1, 1, "tanh", "gaussian")
    assert [n for n, _ in m.named_parameters()] == names
    assert m.state_dict()[names[0]].shape == (1000, 2)                       # no sigma column
    assert int(m._desc.kind) == (6 if cls is net.MLPGradDAE else 7) and int(m._desc.context_dim) == 0
    assert set(m._no_grad_names) == ({"neglogprob.fc.bias"} if cls is net.MLPGradDAE else set())
    with pytest.raises(NotImplementedError):
        cls(noise_type="laplace")
    with pytest.raises(NotImplementedError):
        cls(noise_type="uniform")
    with pytest.raises(NotImplementedError):
        cls(num_hidden_layers=0)
    with pytest.raises(NotImplementedError):
        cls(nonlinearity="gelu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        cls(h_dim=16)(torch.zeros(4, 2), 0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cls(h_dim=16).glogprob(torch.zeros(4, 2))


def test_load_state_dict_keeps_flat_views(golden_dir):
    for path in fixtures(golden_dir):
        fx = load(path)
        (_, d, h, nl), kind = (int(v) for v in fx["shape"]), str(fx["kind"])
        m = (net.MLPGradDAE if kind == "grad" else net.MLPResDAE)(input_dim=d, h_dim=h, num_hidden_layers=nl, nonlinearity=str(fx["act"]))
        sd = state_dict_of(fx)
        m.load_state_dict(sd)
        off = 0
        for n, p in m.named_parameters():
            assert p.data_ptr() == m.flat_params().data_ptr() + 4 * off and torch.equal(p, sd[n])
            off += p.numel()
        assert off == m.flat_params().numel() == L.query("ardae_cdae_param_floats", m._desc)


def test_config_and_network_must_belong_together():
    cfg = net.DaeConfig()
    assert (cfg.sigma_max, cfg.sigma_min, cfg.sigma_annealing, cfg.nsigma, cfg.lr, cfg.optimizer, cfg.beta1, cfg.momentum) == (5.0, 0.05, 4000, 10, 5e-3, "adam_torch", 0.9, 0.0)

    class OnDevice:                      # the check comes right after _require_gpu(): no device is touched before it
        def __init__(self, m):
            self._desc, self._require_gpu = m._desc, lambda: None
    for m, cfg in ((net.MLPGradDAE(h_dim=16), net.ScoreConfig()), (net.MLPResDAE(h_dim=16), net.ScoreConfig()),
                   (net.MLPGradARDAE(h_dim=16), net.DaeConfig()), (net.MLPResARDAE(h_dim=16), net.DaeConfig())):
        with pytest.raises(TypeError, match="(?s)ScoreConfig.*DaeConfig|DaeConfig.*ScoreConfig"):
            net.ArdaeScoreEngine(OnDevice(m), cfg, 8)
    with pytest.raises(TypeError, match="unconditional"):
        net.ArdaeScoreEngine(OnDevice(net.MLPGradCARDAE(h_dim=16, nonlinearity="softplus")), net.DaeConfig(), 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        net.ArdaeScoreEngine(net.MLPGradDAE(h_dim=16), net.DaeConfig(), 8)


def test_flat_opt_adam_torch_keeps_torchs_checkpoint_layout():
    m = net.MLPGradDAE(input_dim=3, h_dim=16, num_hidden_layers=2, nonlinearity="elu")
    opt = _FlatOpt("adam_torch", m.flat_params(), m.flat_params().numel() - 1, 5e-3, 0.9, 0.0, dae=(5.0, 0.05, 4000))      # construction launches nothing
    assert opt.adam and opt.state_names() == ("exp_avg", "exp_avg_sq") and len(opt.buffers()) == 2
    opt.steps = 3
    for k, b in enumerate(opt.buffers()):
        b.copy_(torch.arange(b.numel()) + 10000.0 * (k + 1))
    sd = opt.state_dict(m)
    params = [p for _, p in m.named_parameters()]
    ref = torch.optim.Adam(params, lr=5e-3)
    g = torch.Generator().manual_seed(1)
    for name, p in m.named_parameters():
        p.grad = None if name in m._no_grad_names else torch.randn(p.shape, generator=g)
    ref.step()
    want = ref.state_dict()
    assert list(sd["state"]) == list(want["state"]) == list(range(len(params) - 1))                     # no entry for the bias
    assert all(list(st) == list(want["state"][i]) == ["step", "exp_avg", "exp_avg_sq"] for i, st in sd["state"].items())
    assert {k: sd["param_groups"][0][k] for k in ("lr", "betas", "eps", "weight_decay", "amsgrad")} == {k: want["param_groups"][0][k] for k in ("lr", "betas", "eps", "weight_decay", "amsgrad")}
    # torch.optim.Adam's own file loads; RMSprop's does not
    opt2 = _FlatOpt("adam_torch", m.flat_params(), m.flat_params().numel() - 1, 5e-3, 0.9, 0.0)
    assert opt2.load_state_dict(m, want, "checkpoint") == 1
    assert torch.equal(m.param_views(opt2.a)[0], want["state"][0]["exp_avg"]) and torch.equal(m.param_views(opt2.b)[2], want["state"][2]["exp_avg_sq"])
    with pytest.raises(ValueError, match="written by optimiser 'rmsprop', but this engine was built with 'adam_torch'"):
        opt2.load_state_dict(m, torch.optim.RMSprop(params, lr=1e-3).state_dict(), "checkpoint")
    with pytest.raises(NotImplementedError, match="inside an engine's step"):
        opt2.apply(torch.zeros_like(m.flat_params()), False)


# ---- 5. the float64 restatement reproduces every fp64 fixture ----------------------------------------------------------------------
def test_restatement_reproduces_the_fp64_fixtures(golden_dir):
    for path in fixtures(golden_dir):
        fx = load(path)
        kind, act = str(fx["kind"]), str(fx["act"])
        p = {k: v.double() for k, v in state_dict_of(fx).items()}
        x, eps = (torch.tensor(fx[k]).double() for k in ("x", "eps"))
        loss, grads = loss_and_grads(kind, p, act, x, std_of(fx, torch.float64), eps, False)
        assert abs(float(loss) - float(fx["loss_f64"])) <= 1e-12 * abs(float(fx["loss_f64"])), path
        for n, g in grads.items():
            if f"g_f64/{n}/none" in fx:
                assert g is None and n == "neglogprob.fc.bias", (path, n)
            else:
                assert rel(g, fx["g_f64/" + n]) <= 1e-12, (path, n, rel(g, fx["g_f64/" + n]))
        assert rel(score(kind, p, act, x), fx["glog_f64"]) <= 1e-12, path
    assert sorted(load(p)["std"].ndim for p in fixtures(golden_dir)) == [0] * 6 + [2] * 4         # scalar and [N, 1] noise levels


def test_restatement_reproduces_the_fp64_trajectory(golden_dir):
    """The notebook's loop restated (schedule, broadcast, loss, torch.optim.Adam) in float64 on the fixture's x / eps."""
    for kind in ("grad", "res"):
        fx = load(os.path.join(golden_dir, f"dae_plain_traj_{kind}.npz"))
        c = {k[4:]: v for k, v in fx.items() if k.startswith("cfg/")}
        B, ns, d, act = int(c["B"]), int(c["nsigma"]), int(c["d"]), str(c["act"])
        p = {k: v.double().requires_grad_(True) for k, v in state_dict_of(fx).items()}
        opt = torch.optim.Adam(list(p.values()), lr=float(c["lr"]))
        for s in range(int(c["steps"])):
            sigma = net.dae_sigma(float(c["sigma_max"]), float(c["sigma_min"]), int(c["sigma_annealing"]), s)
            assert sigma == float(fx[f"{s}/sigma"])
            x = torch.tensor(fx[f"{s}/x"]).double().unsqueeze(1).expand(B, ns, d).contiguous().view(B * ns, d)
            eps = torch.tensor(fx[f"{s}/eps"]).double()
            xbar = (x + sigma * eps).requires_grad_(True)
            loss = torch.nn.functional.mse_loss(sigma * score(kind, p, act, xbar, create_graph=True), -eps)
            opt.zero_grad()
            loss.backward()
            opt.step()
            assert abs(float(loss.detach()) - float(fx[f"{s}/loss_f64"])) <= 1e-12 * abs(float(fx[f"{s}/loss_f64"])), (kind, s)
            for n, v in p.items():
                assert rel(v.detach(), fx[f"{s}/p_f64/{n}"]) <= 1e-12, (kind, s, n)
