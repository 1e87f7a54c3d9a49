"""The reconstruction DAEs of models/dae/mlp.py (net.MLPDAE, net.MLPCDAE; ardae_cdae_desc.kind 7 / 11 / 13) without a GPU: parameter layout
against the reference's fixtures, the test-side restatement pinned to them, the drop-in surface, refusals, and the ABI's declarations."""
import ctypes
import inspect
import os

import pytest
import torch

import ardae_amd as net
from ardae_amd import _lib as L
from ardae_amd import layout
from recon_restate import case, fixture_paths, forward, glogprob
from score_restate import LOSS_TOL, TENSOR_TOL, load, rel, state_dict_of

NEW_SYMBOLS = ("ardae_philox_uniform_at", "ardae_recon_perturb", "ardae_recon_perturb_draw", "ardae_latent_recon_perturb",
               "ardae_latent_recon_perturb_draw", "ardae_recon_score")


def spec_of(conditional, enc_input, d, c, h, nl):
    return layout.recon_cdae_spec(d, c, h, nl, enc_input) if conditional else layout.dae_plain_spec("res", d, h, nl)


def all_fixtures(golden_dir):
    u, c = fixture_paths(golden_dir)
    return u + c


def test_layout_names_and_shapes_are_the_fixtures(golden_dir):
    kinds = set()
    for path in all_fixtures(golden_dir):
        fx = load(path)
        conditional, _, _, enc_input, _, (d, c, h, nl), p, *_ = case(fx)
        spec = spec_of(conditional, enc_input, d, c, h, nl)
        assert [(n, tuple(s)) for n, s in spec] == [(n, tuple(v.shape)) for n, v in p.items()], path
        kind = 7 if not conditional else 11 if enc_input else 13
        kinds.add(kind)
        # the C side computes the same total (no GPU needed: the sizing entry points run on the host)
        assert L.query("ardae_cdae_param_floats", L.CdaeDesc(kind, d, c, h, nl, L.ACT["tanh"])) == layout.offsets(spec)[1], path
    assert kinds == {7, 11, 13}
    # enc_input=False: the last MLP's first layer is [h, d + h] = [W1x | W1c]; with one hidden layer ctx_encode is a single fc
    assert layout.recon_cdae_spec(3, 5, 16, 1, False) == [("ctx_encode.fc.weight", (16, 5)), ("ctx_encode.fc.bias", (16,)), ("dae.layers.0.weight", (16, 19)),
                                                           ("dae.layers.0.bias", (16,)), ("dae.fc.weight", (3, 16)), ("dae.fc.bias", (3,))]
    assert layout.recon_cdae_spec(3, 5, 16, 2, True) == layout.cdae_plain_spec("res", 3, 5, 16, 2)


def test_kind_13_sizes_and_refusals_on_the_host():
    lib = L.lib()
    ok = L.CdaeDesc(13, 2, 3, 64, 3, L.ACT["softplus"])
    assert L.query("ardae_cdae_packed_floats", ok) > 0 and L.query("ardae_cdae_workspace_floats", ok, 4, 16, 1) > L.query("ardae_cdae_workspace_floats", ok, 4, 16, 0) > 0
    # without an input encoder the arena is smaller than kind 11's at the same shape
    assert L.query("ardae_cdae_workspace_floats", ok, 4, 16, 1) < L.query("ardae_cdae_workspace_floats", L.CdaeDesc(11, 2, 3, 64, 3, L.ACT["softplus"]), 4, 16, 1)
    assert L.query("ardae_cdae_perturb_fused_ok", ok, 16, 1) == 0 and L.query("ardae_dae_perturb_fused_ok", ok, 4) == 0
    one = ctypes.c_void_p(64)

    def fails(rc, text):
        assert rc < 0 and text in lib.ardae_last_error().decode(), lib.ardae_last_error().decode()
    fails(lib.ardae_cdae_pack(ctypes.byref(L.CdaeDesc(13, 2, 0, 64, 3, 2)), one, one, None), "context_dim >= 1")
    for k in (4, 5, 8, 9, 12, 14):
        fails(lib.ardae_cdae_pack(ctypes.byref(L.CdaeDesc(k, 2, 3, 64, 3, 2)), one, one, None), "kind must be")
    # the new entry points validate before anything is dereferenced
    fails(lib.ardae_recon_perturb(one, one, 4, 2, 2, 2, 0.5, None, one, one, one, None), "noise must be 0 (gaussian) or 1 (uniform)")
    fails(lib.ardae_recon_perturb_draw(one, 4, 2, 2, 0, 0.5, None, 1, 1, 2, one, one, one, one, None), "first_row must be a multiple of 4")
    fails(lib.ardae_latent_recon_perturb(one, None, one, 4, 2, 1, 2, 1.0, 0, 0.5, None, one, one, one, None), "null pointer")
    fails(lib.ardae_latent_recon_perturb_draw(one, one, 0, 2, 1, 2, 1.0, 0, 0.5, None, 1, 1, 0, one, one, one, one, None), "bad batch")
    fails(lib.ardae_recon_score(one, None, 4, 2, 0.5, None, one, None), "null pointer")
    fails(lib.ardae_philox_uniform_at(None, 4, 1, 1, None, 0, None), "bad arguments")


def test_abi_version_and_new_symbols():
    assert L.CONSTANTS["ARDAE_ABI_VERSION"] == 1 and L.lib().ardae_abi_version() == 1
    for name in NEW_SYMBOLS:
        assert name in L.PROTOTYPES and hasattr(L.lib(), name), name
    names = lambda f: [n for n, _, _ in L.PROTOTYPES[f][1]]
    assert names("ardae_philox_uniform_at") == names("ardae_philox_normal_at")
    assert names("ardae_recon_perturb") == ["x", "draw", "B", "nsigma", "d", "noise", "sigma", "dae_state", "xbar", "sigma_out", "target_out", "stream"]
    assert names("ardae_recon_score") == ["recon", "x", "n", "d", "sigma", "dae_state", "out", "stream"]
    assert names("ardae_recon_perturb_draw")[-5:] == ["xbar", "sigma_out", "target_out", "draw_out", "stream"]
    assert names("ardae_latent_recon_perturb_draw")[-5:] == ["xbar", "sigma_out", "target_out", "draw_out", "stream"]


def test_restatement_reproduces_the_fixtures(golden_dir):
    """Pins tests/recon_restate.py: fp32 within the project's bars, float64 within 1e-12."""
    for path in all_fixtures(golden_dir):
        fx = load(path)
        for dtype, tag, ltol, ttol in ((torch.float32, "", LOSS_TOL, TENSOR_TOL), (torch.float64, "_f64", 1e-12, 1e-12)):
            _, act, noise, enc_input, _, _, p, x, ctx, std, draw = case(fx, dtype)
            xbar, recon, loss, grads = forward(p, act, noise, x, std, draw, ctx, enc_input)
            assert rel(xbar, fx["xbar" + tag]) <= (1e-12 if tag else 1e-6), path
            assert abs(float(loss) - float(fx["loss" + tag])) <= ltol * abs(float(fx["loss" + tag])), (path, tag)
            assert rel(recon, fx["x_recon" + tag]) <= ttol, (path, tag)
            for n, g in grads.items():
                assert rel(g, fx[f"g{tag}/{n}"]) <= ttol, (path, tag, n)
            glog = glogprob(p, act, x, std, ctx, enc_input).detach()
            assert glog.reshape(-1).shape == fx["glog" + tag].reshape(-1).shape
            assert rel(glog.reshape(-1), fx["glog" + tag].reshape(-1)) <= ttol, (path, tag)


def test_fixture_set_covers_what_it_should(golden_dir):
    u, c = (list(map(load, paths)) for paths in fixture_paths(golden_dir))
    assert sorted(str(f["noise"]) for f in u) == ["gaussian"] * 3 + ["uniform"] * 2
    assert sum(f["std"].ndim == 0 and float(f["std"]) >= 0.3 for f in u) == 3 and sum(f["std"].ndim == 2 and abs(f["std"]).min() >= 0.05 for f in u) == 2
    assert {(int(f["shape"][0]), int(f["shape"][1])) for f in u} >= {(60, 3), (64, 2), (96, 8)}
    assert sum(int(f["enc_input"]) for f in c) == len(c) // 2 and sum(int(f["rows"]) for f in c) == len(c) // 2
    assert sum(int(f["shape"][2]) != int(f["shape"][3]) for f in c) >= 4                      # c != d
    assert {int(f["enc_input"]) for f in c if int(f["shape"][5]) == 1} == {0, 1}              # L = 1: ctx_encode is one Linear
    for f in c:
        B, S = int(f["shape"][0]), int(f["shape"][1])
        repeated = bool((f["ctx"] == f["ctx"][:, :1]).all())
        assert f["ctx"].shape[:2] == (B, S) and repeated == (not int(f["rows"]))
    for name, cond in (("recon_dae_traj", False), ("recon_cdae_traj", True)):
        for noise in ("gaussian", "uniform"):
            t = load(os.path.join(golden_dir, f"{name}_{noise}.npz"))
            assert str(t["noise"]) == noise and int(t["cfg/steps"]) == 6 and int(t["cfg/sigma_annealing"]) < 6
            assert ("0/latent" in t) == cond and f"5/p_f64/{'dae' if cond else 'main'}.fc.bias" in t
            if noise == "uniform":
                assert 0.0 <= t["0/eps"].min() and t["0/eps"].max() < 1.0


def test_module_defaults_and_attributes_are_the_references():
    sig = lambda cls: {k: v.default for k, v in inspect.signature(cls.__init__).parameters.items() if k != "self"}
    assert sig(net.MLPDAE) == dict(input_dim=2, h_dim=1000, std=0.1, num_hidden_layers=1, nonlinearity="tanh", noise_type="gaussian")
    assert sig(net.MLPCDAE) == dict(input_dim=2, h_dim=128, context_dim=2, std=0.1, num_hidden_layers=1, nonlinearity="tanh", noise_type="gaussian",
                                    enc_input=False, enc_ctx=True)
    m = net.MLPDAE(h_dim=16)
    assert (m.input_dim, m.h_dim, m.std, m.num_hidden_layers, m.nonlinearity, m.noise_type) == (2, 16, 0.1, 1, "tanh", "gaussian")
    assert [n for n, _ in m.named_parameters()] == ["main.layers.0.weight", "main.layers.0.bias", "main.fc.weight", "main.fc.bias"]
    assert m._desc.kind == 7 and m._recon and isinstance(m, net.ReconDAE) and not isinstance(m, net.DAE)
    c = net.MLPCDAE()
    assert (c.input_dim, c.h_dim, c.context_dim, c.std, c.num_hidden_layers, c.nonlinearity, c.noise_type, c.enc_input, c.enc_ctx) == (
        2, 128, 2, 0.1, 1, "tanh", "gaussian", False, True)
    assert [n for n, _ in c.named_parameters()] == ["ctx_encode.fc.weight", "ctx_encode.fc.bias", "dae.layers.0.weight", "dae.layers.0.bias",
                                                    "dae.fc.weight", "dae.fc.bias"]
    assert c._desc.kind == 13 and c._recon
    assert tuple(dict(c.named_parameters())["dae.layers.0.weight"].shape) == (128, 2 + 128)
    e = net.MLPCDAE(h_dim=16, num_hidden_layers=2, enc_input=True, noise_type="uniform")
    assert e._desc.kind == 11 and e.noise_type == "uniform" and isinstance(e, net.ReconConditionalDAE) and not isinstance(e, net.ConditionalDAE)
    assert [n for n, _ in e.named_parameters()][:8:2] == ["ctx_encode.layers.0.weight", "ctx_encode.fc.weight", "inp_encode.layers.0.weight", "inp_encode.fc.weight"]
    assert not hasattr(net.MLPResDAE(h_dim=8), "_recon")


def test_state_dict_round_trips_the_fixtures(golden_dir):
    for path in all_fixtures(golden_dir):
        fx = load(path)
        conditional, act, noise, enc_input, _, (d, c, h, nl), *_ = case(fx)
        kw = dict(input_dim=d, h_dim=h, num_hidden_layers=nl, nonlinearity=act, noise_type=noise)
        m = net.MLPCDAE(context_dim=c, enc_input=enc_input, **kw) if conditional else net.MLPDAE(**kw)
        sd = state_dict_of(fx)
        m.load_state_dict(sd)
        assert list(m.state_dict()) == list(sd) and all(torch.equal(m.state_dict()[k], v) for k, v in sd.items())
        assert torch.equal(m.flat_params(), torch.cat([v.reshape(-1) for v in sd.values()]))      # the parameters stay views of the flat buffer


def test_refusals():
    for cls in (net.MLPDAE, net.MLPCDAE):
        with pytest.raises(NotImplementedError, match="gaussian.*uniform"):
            cls(noise_type="laplace")
        with pytest.raises(NotImplementedError, match="nonlinearity"):
            cls(nonlinearity="gelu")
        with pytest.raises(NotImplementedError, match="num_hidden_layers >= 1"):
            cls(num_hidden_layers=0)
        cls(h_dim=8, noise_type="uniform")
    with pytest.raises(NotImplementedError, match="enc_ctx=False is not built"):
        net.MLPCDAE(enc_ctx=False)
    # the existing score networks still refuse anything but gaussian noise
    for cls in (net.MLPResDAE, net.MLPResCDAE, net.MLPGradARDAE):
        with pytest.raises(NotImplementedError):
            cls(h_dim=8, noise_type="uniform")
    with pytest.raises(RuntimeError, match="no CPU path"):
        net.MLPDAE(h_dim=8)(torch.zeros(4, 2))


def test_config_and_network_must_belong_together():
    class OnDevice:                      # the check comes right after _require_gpu(): no device is touched before it
        def __init__(self, m):
            self._desc, self._require_gpu, self._recon, self.NOISE, self.noise_type = m._desc, lambda: None, True, m.NOISE, m.noise_type
    with pytest.raises(TypeError, match="(?s)DaeConfig.*ScoreConfig"):
        net.ArdaeScoreEngine(OnDevice(net.MLPDAE(h_dim=16)), net.ScoreConfig(), 8)
    for enc_input in (False, True):
        with pytest.raises(TypeError, match="(?s)DaeConfig.*ScoreConfig"):
            net.ArdaeCondScoreEngine(OnDevice(net.MLPCDAE(h_dim=16, enc_input=enc_input)), net.ScoreConfig(), 4, 8)
    with pytest.raises(TypeError, match="unconditional"):
        net.ArdaeScoreEngine(OnDevice(net.MLPCDAE(h_dim=16)), net.DaeConfig(), 8)
    with pytest.raises(TypeError, match="conditional"):
        net.ArdaeCondScoreEngine(OnDevice(net.MLPDAE(h_dim=16)), net.DaeConfig(), 4, 8)

    class OnDeviceGen(net.Generator):
        def _require_gpu(self, *t):
            pass
    # the energy-fitting engine runs the AR-DAE update (a ScoreConfig): a reconstruction DAE is refused there
    with pytest.raises(TypeError, match="(?s)DaeConfig.*ScoreConfig"):
        net.ArdaeFitEngine(OnDeviceGen(), OnDevice(net.MLPDAE(h_dim=16)), net.FitConfig(), 8)
